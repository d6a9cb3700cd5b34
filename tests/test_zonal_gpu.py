"""kernels.zonal_index / zonal_stats / zonal_paint and nd_amd.zonal on the GPU against the restatement
(tests/zonal_ref.py): float64 outputs bit for bit (as int64 views, NaN where it has NaN), counts equal, min / max by ==.
The shapes are the smallest at which the kernels can go wrong: planes of 70 x 150 or 131 x 257, zones one below, at
and one above every group size of the tree (the 8-lane group, the chunk of 64, the segment of 4096, two segments)."""
import numpy as np
import pytest

from tests import zonal_cases as cases
from tests import zonal_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K(device):
    from nd_amd import kernels
    return kernels


# ---- zone sizes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scattered', [True, False], ids=['scattered', 'runs'])
@pytest.mark.parametrize('layout', ['planar', 'pixel'])
def test_zone_sizes_around_every_group_size(K, layout, scattered):
    rng = np.random.default_rng([21, scattered, len(layout)])
    lab = cases.sized_zones(rng, (131, 257), cases.ZONE_SIZES, scattered=scattered)
    x = cases.speckle(rng, (3, 131, 257), 'float32')
    got, _ = cases.check_stats(K, x, lab, layout=layout)
    assert list(got['count'][0] + got['nan_count'][0]) == list(cases.ZONE_SIZES)


def test_one_zone_that_is_the_whole_plane(K):
    rng = np.random.default_rng(22)
    x = cases.speckle(rng, (2, 131, 257), 'float64')
    got, index = cases.check_stats(K, x, np.ones((131, 257), np.uint8))
    assert index.n == 1 and got['count'][0, 0] + got['nan_count'][0, 0] == 131 * 257


def test_every_pixel_its_own_zone(K):
    rng = np.random.default_rng(23)
    lab = (1 + rng.permutation(70 * 150)).reshape(70, 150).astype(np.int32)
    x = cases.speckle(rng, (3, 70, 150), 'float32')
    got, index = cases.check_stats(K, x, lab)
    assert index.n == 10500 and (got['count'] + got['nan_count'] == 1).all()
    assert (got['m2'][got['count'] == 1] == 0).all()


@pytest.mark.parametrize('connectivity', [4, 8])
def test_zones_from_label_regions(K, device, connectivity):
    import torch
    rng = np.random.default_rng([24, connectivity])
    mask = (rng.random((131, 257)) < 0.59).astype(np.uint8)
    labels, counts = K.label_regions(torch.from_numpy(mask).to(device), connectivity)
    index = K.zonal_index(labels)
    host = labels.cpu().numpy()
    cases.check_index(index, host)
    assert index.n == int(counts) > 10                  # (0.59 is far above the threshold at 8: few, long regions)
    x = cases.speckle(rng, (3, 131, 257), 'float32')
    got = cases.device_stats(K, x, index, 'pixel')
    want = cases.want_stats(x, host)
    ref.same_stats(got, want)
    sizes, _ = K.region_sizes(labels, counts)
    assert np.array_equal(got['count'][0] + got['nan_count'][0], sizes.cpu().numpy())


def test_one_zone_no_zone_and_no_zoned_pixel(K, device):
    import torch
    rng = np.random.default_rng(25)
    x = cases.speckle(rng, (3, 70, 150), 'float32')
    lab = np.zeros((70, 150), np.int32)
    lab[3, 5:9] = 1
    got, index = cases.check_stats(K, x, lab)                           # n = 1
    assert index.n == 1 and got['sum'].shape == (3, 1)
    got, index = cases.check_stats(K, x, np.zeros((70, 150), np.int32))  # n = 0
    assert index.n == 0 and got['sum'].shape == (3, 0) and got['count'].dtype == np.int64
    assert bool((index.keys == 0).all())
    got, index = cases.check_stats(K, x, lab, ids=[])
    assert index.n == 0
    got, index = cases.check_stats(K, x, lab, ids=[5, 6])                # zones, and no pixel in any
    assert (got['count'] == 0).all() and (got['sum'] == 0).all() and np.isnan(got['min']).all()
    assert np.isnan(got['mean']).all() and (got['m2'] == 0).all()
    painted = cases.check_paint(K, got['mean'], index, lab, x, ids=[5, 6], keep=True)
    ref.same(painted, x)
    # an empty plane
    e = K.zonal_index(torch.zeros((0, 7), dtype=torch.int32, device=device))
    assert e.n == 0 and e.keys.shape == (0, 7) and e.perm.numel() == 0 and e.offsets.tolist() == [0]
    st = K.zonal_stats(torch.zeros((2, 0, 7), device=device), K.zonal_index(
        torch.zeros((0, 7), dtype=torch.int32, device=device), ids=[1, 2]), stats=('count', 'min', 'sum'))
    assert st['count'].tolist() == [[0, 0], [0, 0]] and bool(torch.isnan(st['min']).all()) and not bool(st['sum'].any())


# ---- planes per call, types, layouts -----------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [1, 3, 65])        # 65: one more than the planes a wave keeps running sums of
@pytest.mark.parametrize('layout', ['planar', 'pixel'])
def test_planes_per_call(K, planes, layout):
    rng = np.random.default_rng([26, planes])
    lab = cases.sized_zones(rng, (70, 150), (4097, 65, 64, 8, 1, 5000))
    x = cases.speckle(rng, (planes, 70, 150), 'float32')
    cases.check_stats(K, x, lab, layout=layout)


@pytest.mark.parametrize('dtype', ['float32', 'float64', 'int32'])
def test_data_types(K, dtype):
    rng = np.random.default_rng([27, len(dtype), ord(dtype[0])])
    lab = cases.sized_zones(rng, (70, 150), (4097, 65, 9, 1, 700))
    if dtype == 'int32':
        x = rng.integers(-2 ** 31, 2 ** 31, size=(3, 70, 150)).astype(np.int32)
    else:
        x = cases.speckle(rng, (3, 70, 150), dtype) * 10.0 ** rng.integers(-3, 4, size=(3, 70, 150)).astype(dtype)
    for layout in cases.LAYOUTS:
        got, _ = cases.check_stats(K, x, lab, layout=layout)
    if dtype == 'int32':
        assert (got['nan_count'] == 0).all() and got['sum'].dtype == np.float64


@pytest.mark.parametrize('dtype', cases.LABEL_DTYPES)
@pytest.mark.parametrize('strided', [False, True], ids=['packed', 'strided'])
def test_label_types_and_strided_label_planes(K, dtype, strided):
    rng = np.random.default_rng([28, len(dtype), ord(dtype[0]), strided])
    x = cases.speckle(rng, (2, 70, 150), 'float32')
    if dtype == 'bool':
        lab = rng.random((70, 150)) < 0.3
    else:
        lab = cases.rcases.class_map(rng, (70, 150), 5, dtype)       # floats: NaN, -0.0 and 1.5 among the labels
    if dtype != 'int64':                                             # (its class map has labels beyond 2^53)
        cases.check_stats(K, x, lab, strided=strided)
    if dtype == 'int64':
        cases.check_stats(K, x, lab, ids=[-5, 7, 2 ** 53, 2 ** 53 + 1], strided=strided)
        lab = np.array([3, 100234, 2 ** 40 + 1, 2 ** 40, 0, -7], np.int64)[rng.integers(0, 6, size=(70, 150))]
        got, index = cases.check_stats(K, x, lab, ids=[3, 100234, 2 ** 40 + 1], strided=strided)
        assert index.n == 3 and (got['count'] > 0).all()
    if dtype in ('float32', 'float64'):
        lab = np.array([2.0, 2.5, np.nan, 1.0, np.inf, -0.0, 3.0, -1.0], dtype)[rng.integers(0, 8, size=(70, 150))]
        got, index = cases.check_stats(K, x, lab, strided=strided)
        assert index.n == 3
        cases.check_stats(K, x, lab, ids=[-1, 2], strided=strided)


def test_transposed_label_plane(K, device):
    import torch
    rng = np.random.default_rng(29)
    lab = cases.sized_zones(rng, (70, 150), (4097, 65, 9, 1, 700))
    index = K.zonal_index(torch.from_numpy(np.ascontiguousarray(lab.T)).to(device), dims=('x', 'y'))
    cases.check_index(index, lab)


# ---- values ----------------------------------------------------------------------------------------------------------
def test_special_values(K):
    rng = np.random.default_rng(30)
    lab = cases.sized_zones(rng, (70, 150), (4097, 65, 9, 1, 700, 64, 130, 5))
    x = cases.speckle(rng, (3, 70, 150), 'float64')
    x[0][lab == 1] = np.nan                                             # whole zones NaN: several segments, one chunk,
    x[:, lab == 3] = np.nan                                             # a group of lanes
    x[1][lab == 6] = np.nan
    x[2][lab == 4] = np.nan
    two = np.nonzero(lab.reshape(-1) == 2)[0]
    x[0].reshape(-1)[two[:3]] = [np.inf, -np.inf, np.inf]                # inf - inf inside a chunk
    x[1].reshape(-1)[two[5]] = np.inf
    seven = np.nonzero(lab.reshape(-1) == 7)[0]
    x[:, lab == 7] = 1e-30                                              # 1e-30 and 1e30 in one zone
    x[0].reshape(-1)[seven[64]] = 1e30
    x[1].reshape(-1)[seven[:2]] = [1e30, -1e30]
    x[:, lab == 8] = -0.0
    got, _ = cases.check_stats(K, x, lab)
    assert got['count'][0, 0] == 0 and got['nan_count'][0, 0] == 4097 and got['sum'][0, 0] == 0.0
    assert np.isnan(got['sum'][0, 1]) and got['sum'][1, 1] == np.inf and np.isnan(got['m2'][1, 1])
    assert got['max'][0, 6] == 1e30 and got['min'][0, 6] == 1e-30
    assert (got['sum'][:, 7] == 0).all() and np.signbit(got['sum'][:, 7]).all()      # -0.0 + -0.0, never + 0.0
    cases.check_stats(K, x.astype(np.float32), lab, layout='pixel')


# ---- repeatability ---------------------------------------------------------------------------------------------------
def test_repeatable_zone_local_and_date_order(K):
    rng = np.random.default_rng(31)
    lab = cases.sized_zones(rng, (131, 257), (8193, 4096, 65, 9, 1, 700, 5000))
    x = cases.speckle(rng, (3, 131, 257), 'float32')
    index = cases.device_index(K, lab)
    first = cases.device_stats(K, x, index)
    second = cases.device_stats(K, x, index, 'pixel')
    third = cases.device_stats(K, x, cases.device_index(K, lab))
    for name in cases.ALL:
        assert first[name].tobytes() == second[name].tobytes() == third[name].tobytes(), name
    # the other zones relabelled, merged and removed: zones 1, 3 and 7 keep their bytes
    other = lab.copy()
    other[lab == 2] = 40
    other[lab == 4] = 5
    other[lab == 6] = 0
    moved = cases.device_stats(K, x, cases.device_index(K, other))
    for name in cases.ALL:
        for z in (1, 3, 7):
            assert moved[name][:, z - 1].tobytes() == first[name][:, z - 1].tobytes(), (name, z)
        assert moved[name][:, 39].tobytes() == first[name][:, 1].tobytes(), name
    # the dates in reversed order give the reversed statistics
    back = cases.device_stats(K, x[::-1].copy(), index)
    for name in cases.ALL:
        assert back[name][::-1].tobytes() == first[name].tobytes(), name
    # one plane alone gives its row of the batch
    alone = cases.device_stats(K, x[1:2], index)
    for name in cases.ALL:
        assert alone[name][0].tobytes() == first[name][1].tobytes(), name


# ---- paint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', cases.LAYOUTS)
@pytest.mark.parametrize('strided', [False, True], ids=['packed', 'strided'])
def test_paint(K, layout, strided):
    rng = np.random.default_rng([32, len(layout), strided])
    lab = cases.sized_zones(rng, (70, 150), (4097, 65, 9, 1, 700))
    for dtype in ('float32', 'float64'):
        x = cases.speckle(rng, (3, 70, 150), dtype)
        got, index = cases.check_stats(K, x, lab, stats=('mean', 'max'))
        cases.check_paint(K, got['mean'], index, lab, x, layout=layout, strided=strided, keep=True)
        cases.check_paint(K, got['max'], index, lab, x, layout=layout, strided=strided, fill=-2.5)
        painted = cases.check_paint(K, got['mean'], index, lab, x, layout=layout, strided=strided)
        assert np.isnan(painted[:, lab == 0]).all()
        # paint(mean) -> stats gives the mean back
        again = cases.device_stats(K, painted, index, stats=('min', 'max'))
        want = got['mean'].astype(dtype).astype(np.float64)
        ref.same(again['min'], want)
        ref.same(again['max'], want)


def test_errors(K, device):
    import torch
    lab = torch.ones((4, 5), dtype=torch.int32, device=device)
    index = K.zonal_index(lab)
    x = torch.zeros((2, 4, 5), device=device)
    with pytest.raises(ValueError, match='planes of'):
        K.zonal_stats(torch.zeros((2, 4, 6), device=device), index)
    with pytest.raises(ValueError, match='stats'):
        K.zonal_stats(x, index, stats=('median',))
    with pytest.raises(TypeError, match='complex'):
        K.zonal_stats(x.to(torch.complex64), index)
    with pytest.raises(TypeError):
        K.zonal_index(lab.to(torch.int16))
    with pytest.raises(ValueError, match='increasing'):
        K.zonal_index(lab, ids=[2, 2])
    with pytest.raises(ValueError, match='one plane'):
        K.zonal_index(torch.ones((2, 4, 5), dtype=torch.int32, device=device))
    with pytest.raises(NotImplementedError, match='zones'):
        K.zonal_index(torch.full((4, 5), 2 ** 31, dtype=torch.int64, device=device))
    table = torch.zeros((2, 1), dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match='table'):
        K.zonal_paint(table[:1], index, like=x)
    with pytest.raises(ValueError, match='keep'):
        K.zonal_paint(table, index, out=x, keep=True)
    with pytest.raises(ValueError, match='overlap'):
        K.zonal_paint(table, index, like=x, out=x, keep=True)
    with pytest.raises(TypeError, match='float32 or float64'):
        K.zonal_paint(table, index, like=x.to(torch.int32))
    assert K.zonal_paint(table, index, like=x).shape == (2, 4, 5)


# ---- the container layer ---------------------------------------------------------------------------------------------
def test_parcels_end_to_end_on_device_and_numpy_datasets(device):
    import torch
    from nd_amd import vector, xr_lite, zonal
    rng = np.random.default_rng(33)
    k, ny, nx = 4, 70, 150
    coords = {'time': np.arange(k), 'y': 100.0 - np.arange(ny), 'x': 7.0 + np.arange(nx)}
    vv, vh = cases.speckle(rng, (k, ny, nx), 'float32'), cases.speckle(rng, (ny, nx, k), 'float64')
    shapes = []
    for i in range(12):
        cx, cy, r = rng.uniform(10, 140), rng.uniform(35, 95), rng.uniform(1, 18)
        ang = np.sort(rng.uniform(0, 2 * np.pi, size=6))
        shapes.append([np.stack([7.0 + cx + r * np.cos(ang), cy + r * np.sin(ang)], 1)])
    for on_device in (True, False):
        ds = xr_lite.Dataset(coords=coords, attrs={'crs': 'none'})
        ds['vv'] = (('time', 'y', 'x'), torch.from_numpy(vv).to(device) if on_device else vv)
        ds['vh'] = (('y', 'x', 'time'), torch.from_numpy(vh).to(device) if on_device else vh)
        ds['dates'] = (('time',), np.arange(k))
        zones = vector.rasterize_shapes(shapes, ds)
        lab = zones.values.cpu().numpy() if torch.is_tensor(zones.values) else np.asarray(zones.values)
        assert torch.is_tensor(zones.values) == on_device and 3 < len(np.unique(lab)) <= 13
        out = zonal.zonal_stats(ds, zones, ids=np.arange(1, 13), ddof=1)
        assert list(out.data_vars) == ['%s__%s' % (v, s) for v in ('vv', 'vh')
                                       for s in ('count', 'mean', 'std', 'min', 'max')]
        assert out['vv__mean'].dims == ('zone', 'time') and list(out.coords['zone']) == list(range(1, 13))
        host = {}
        for name, da in out.data_vars.items():
            assert torch.is_tensor(da.values) == on_device, name      # device in, device out
            host[name] = da.values.cpu().numpy() if on_device else da.values
        for v, planes in (('vv', vv), ('vh', np.moveaxis(vh, -1, 0))):
            want = ref.zonal_stats(planes, lab, np.arange(1, 13))[0]
            ref.same(host[v + '__count'], want['count'].T.copy())
            ref.same(host[v + '__mean'], ref.mean(want).T.copy())
            ref.same(host[v + '__std'], ref.std(want, 1).T.copy())
            ref.same_minmax(host[v + '__min'], want['min'].T.copy())
            ref.same_minmax(host[v + '__max'], want['max'].T.copy())
        painted = zonal.zonal_paint(ds, zones, 'mean', keep=True, ids=np.arange(1, 13))
        assert painted['dates'].values is ds['dates'].values and torch.is_tensor(painted['vh'].values) == on_device
        got = painted['vh'].values.cpu().numpy() if on_device else painted['vh'].values
        assert painted['vh'].dims == ('y', 'x', 'time') and got.dtype == np.float64
        if on_device:
            assert painted['vh'].values.stride() == ds['vh'].values.stride()
        want = ref.zonal_stats(np.moveaxis(vh, -1, 0), lab, np.arange(1, 13))[0]
        k_ = ref.keys(lab, np.arange(1, 13))[0]
        ref.same(np.ascontiguousarray(np.moveaxis(got, -1, 0)),
                 ref.paint(ref.mean(want), k_, np.float64, np.moveaxis(vh, -1, 0)))
        assert zonal.ZonalStatistics(zones, ids=np.arange(1, 13), ddof=1).apply(ds).equals(out)


def test_regions_over_time_end_to_end(device):
    import torch
    from nd_amd import regions, xr_lite, zonal
    rng = np.random.default_rng(34)
    k, ny, nx = 3, 70, 150
    change = np.stack([rng.random((ny, nx)) < d for d in (0.3, 0.59, 0.0)])
    vv = cases.speckle(rng, (k, ny, nx), 'float32')
    ds = xr_lite.Dataset(coords={'time': np.arange(k)})
    ds['vv'] = (('time', 'y', 'x'), torch.from_numpy(vv).to(device))
    zones = regions.label_regions(xr_lite.DataArray(torch.from_numpy(change).to(device), ('time', 'y', 'x')), 8)
    lab = zones.values.cpu().numpy()
    n = int(lab.max())
    assert zones.attrs['n_regions'][2] == 0 and n == max(zones.attrs['n_regions'])
    out = zonal.zonal_stats(ds, zones, stats=('count', 'sum', 'mean', 'var'))
    assert out['vv__sum'].shape == (n, k) and list(out.coords['zone']) == list(range(1, n + 1))
    for t in range(k):
        want = ref.zonal_stats(vv[t:t + 1], lab[t], np.arange(1, n + 1))[0]
        ref.same(out['vv__sum'].values[:, t].cpu().numpy(), want['sum'][0])
        ref.same(out['vv__count'].values[:, t].cpu().numpy(), want['count'][0])
        ref.same(out['vv__var'].values[:, t].cpu().numpy(), ref.var(want)[0])
    assert not bool(out['vv__count'].values[:, 2].any())               # a zone absent from a plane: count 0
    painted = zonal.zonal_paint(ds, zones, 'sum', fill=0.0)
    for t in range(k):
        want = ref.zonal_stats(vv[t:t + 1], lab[t], np.arange(1, n + 1))[0]
        ref.same(painted['vv'].values[t].cpu().numpy(),
                 ref.paint(want['sum'], ref.keys(lab[t], None, n)[0], np.float32, fill=0.0)[0])


# ---- under the canary: poisoned outputs and workspaces between guard bands -------------------------------------
@pytest.mark.parametrize('pattern', [0xFF, 0x55], ids=['ff', '55'])
@pytest.mark.parametrize('layout', ['planar', 'pixel'])
def test_under_the_canary(K, layout, pattern):
    from tests.canary import canary
    rng = np.random.default_rng([35, len(layout)])
    lab = cases.sized_zones(rng, (70, 150), (4097, 65, 9, 1, 700, 0, 3))
    x = cases.speckle(rng, (3, 70, 150), 'float32')
    plain, index = cases.check_stats(K, x, lab, layout=layout)
    with canary(pattern) as c:
        got, index = cases.check_stats(K, x, lab, layout=layout)
        c.check()
        painted = cases.check_paint(K, got['mean'], index, lab, x, layout=layout, fill=1.0)
        c.check()
        assert c.wrapped >= 8
    for name in cases.ALL:
        assert got[name].tobytes() == plain[name].tobytes(), name
    assert (painted[:, lab == 0] == 1.0).all()
