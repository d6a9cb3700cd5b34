"""kernels.speckle_lee / speckle_multitemporal and the filter classes on the device against tests/speckle_ref.py:
equal bit for bit, NaN positions included, no tolerance and no excluded pixel.  Outputs start from a sentinel, so an
unwritten element shows, and what surrounds a strided output must stay as it was (tests/speckle_cases.py).  The
planes are the smallest at which the tiled kernels can go wrong, built from the tile extents of the library."""
import numpy as np
import pytest

from tests import speckle_cases as cases
from tests import speckle_ref as ref

pytestmark = pytest.mark.gpu
SEED = 20261020


@pytest.fixture(scope='module')
def K(device):
    from nd_amd import kernels
    return kernels


def _stack(seed, k, ny, nx, dtype, seams=(), looks=4.0):
    rng = np.random.default_rng([SEED, seed])
    a = cases.speckle(rng, (k, ny, nx), dtype, looks)
    return cases.plant(a, rng, seams)


def _seams():
    (ty, tx), (hy, _) = cases.tiles()
    return [(ty, tx), (hy, tx), (2 * ty, tx)]


# ------------------------------------------------------------------ Lee / Kuan
def test_lee_every_width_on_the_seam_planes(K):
    (ty, tx), _ = cases.tiles()
    n = 0
    for w in cases.WIDTHS:
        for ny, nx in ((ty + 1, tx + 1), (2 * ty + 3, tx + w // 2)):
            dtype = (np.float32, np.float64)[n % 2]
            method = ('lee', 'kuan')[(n // 2) % 2]
            looks = (1.0, 4.4)[(n // 4) % 2] if w > 1 else (4.4, 1.0)[n % 2]
            cases.check_lee(K, _stack(n, 2, ny, nx, dtype, _seams()), w, looks, method)
            n += 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_lee_small_and_tile_sized_planes(K, dtype):
    (ty, tx), _ = cases.tiles()
    n = 100
    for ny, nx in cases.plane_shapes(ty, tx)[:6]:
        for w, method, looks in ((1, 'lee', 1.0), (3, 'kuan', 4.4), (7, 'lee', 4.4), (31, 'kuan', 1.0)):
            cases.check_lee(K, _stack(n, 3, ny, nx, dtype, _seams()), w, looks, method)
            n += 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('layout', cases.LAYOUTS)
@pytest.mark.parametrize('strided_out', [False, True])
def test_lee_layouts(K, dtype, layout, strided_out):
    (ty, tx), _ = cases.tiles()
    for n, (w, method) in enumerate(((5, 'lee'), (13, 'kuan'))):
        src = _stack(200 + n, 3, ty + 1, tx + 1, dtype, _seams())
        cases.check_lee(K, src, w, 4.4, method, layout=layout, strided_out=strided_out)


def test_lee_integers_two_axes_and_four(K, device):
    import torch
    src = _stack(300, 6, 9, 70, np.int16)
    got = cases.check_lee(K, src, 7, 4.4, 'lee')
    assert got.dtype == np.float64
    plane = _stack(301, 1, 33, 65, np.float32)[0]
    out = K.speckle_lee(torch.from_numpy(plane).to(device), 9, 1.0, 'kuan')
    cases.assert_same(out.cpu().numpy(), ref.lee(plane, 9, 1.0, 'kuan'))
    four = _stack(302, 6, 9, 70, np.float32).reshape(2, 3, 9, 70)
    out = K.speckle_lee(torch.from_numpy(four).to(device), 3, 2.0, dims=('band', 'time', 'y', 'x'))
    cases.assert_same(out.cpu().numpy(), ref.lee(four, 3, 2.0))


def test_lee_refuses_overlap_and_wrong_outputs(K, device):
    import torch
    t = torch.ones(2, 5, 6, device=device)
    with pytest.raises(ValueError, match='overlap'):
        K.speckle_lee(t, 3, 1.0, out=t)
    with pytest.raises(ValueError):
        K.speckle_lee(t, 3, 1.0, out=torch.empty(2, 5, 7, device=device))
    with pytest.raises(TypeError, match='complex'):
        K.speckle_lee(torch.ones(2, 5, 6, dtype=torch.complex64, device=device), 3, 1.0)


# ------------------------------------------------------------------ multitemporal
# (k, C): a few dates; the register form of 8 planes full; k * C at the limit of the one-launch form and one beyond
MT_FORMS = [(1, 1), (2, 1), (5, 1), (2, 4), (3, 4), (32, 1), (33, 1), (16, 2), (17, 2), (8, 4), (9, 4), (11, 3)]


@pytest.mark.parametrize('k,nvar', MT_FORMS)
def test_multitemporal_both_forms(K, k, nvar):
    from nd_amd import _lib
    (ty, tx), _ = cases.tiles()
    hot = k * nvar <= K.SPECKLE_HOT_MAX_PLANES
    assert (_lib.lib().nd_amd_speckle_multitemporal_workspace_bytes(ty + 1, tx + 1, k, nvar) == 0) == hot
    n = 400 + 10 * k + nvar
    widths = {(1, 1): (1, 3, 5, 7, 9, 11, 13, 31), (33, 1): (1, 3, 5, 7, 9, 11, 13, 31)}.get((k, nvar), (7, 13))
    for i, w in enumerate(widths):
        dtype = (np.float32, np.float64)[(i + k) % 2]
        ny, nx = ((ty + 1, tx + 1), (2 * ty + 3, tx + w // 2))[i % 2] if k * nvar < 30 else (ty + 1, tx + 1)
        variables = [_stack(n + 100 * c + i, k, ny, nx, dtype, _seams()) for c in range(nvar)]
        cases.check_multitemporal(K, variables, w)


@pytest.mark.parametrize('k', [2, 33])
def test_multitemporal_small_planes(K, k):
    (ty, tx), (hy, _) = cases.tiles()
    n = 600 + k
    for ny, nx in cases.plane_shapes(ty, tx)[:6] + [(hy - 1, tx - 1), (hy, tx), (hy + 1, tx + 1)]:
        for w in (7, 3) if ny > 3 else (7, 31):
            cases.check_multitemporal(K, [_stack(n, k, ny, nx, np.float32, _seams())], w)
            n += 1


@pytest.mark.parametrize('k,nvar', [(3, 2), (34, 1)])
@pytest.mark.parametrize('layout', cases.LAYOUTS)
@pytest.mark.parametrize('strided_out', [False, True])
def test_multitemporal_layouts(K, k, nvar, layout, strided_out):
    (ty, tx), _ = cases.tiles()
    dtype = np.float64 if strided_out else np.float32
    variables = [_stack(700 + c, k, ty + 1, tx + 1, dtype, _seams()) for c in range(nvar)]
    cases.check_multitemporal(K, variables, 5, layout=layout, strided_out=strided_out)


@pytest.mark.parametrize('k', [4, 40])
def test_multitemporal_date_with_a_zero_local_mean(K, k):
    """a date that is exactly 0 over more than a window: 0 / 0 enters r as it does, in both forms"""
    src = _stack(800, k, 40, 70, np.float32)
    src[1, 5:30, 10:50] = 0.0
    got = cases.check_multitemporal(K, [src], 7)[0]
    assert np.isnan(got[:, 10:25, 15:45]).all() and np.isfinite(got[:, 33:36, 52:62]).all()


def test_multitemporal_integers_and_variables_that_lie_differently(K, device):
    import torch
    a = _stack(900, 3, 20, 70, np.int16)
    got = cases.check_multitemporal(K, [a], 3)[0]
    assert got.dtype == np.float64
    # one variable planar, one a view of (y, x, time) memory: packed by the wrapper, same result
    u, v = _stack(901, 3, 20, 70, np.float32), _stack(902, 3, 20, 70, np.float32)
    tv = torch.from_numpy(np.ascontiguousarray(np.moveaxis(v, 0, -1))).to(device).permute(2, 0, 1)
    got = K.speckle_multitemporal([torch.from_numpy(u).to(device), tv], 5)
    for g, want in zip(got, ref.multitemporal([u, v], 5)):
        cases.assert_same(g.cpu().numpy(), want)
    with pytest.raises(NotImplementedError):
        K.speckle_multitemporal([tv] * 5, 3)
    with pytest.raises(NotImplementedError):
        K.speckle_multitemporal([tv, tv.double()], 3)
    with pytest.raises(ValueError, match='overlap'):
        K.speckle_multitemporal(tv, 3, out=tv)


# ------------------------------------------------------------------ class level
def _dataset(device, on_device, dims=('time', 'y', 'x'), shape=(3, 37, 20), dtype=np.float32, names=('VV', 'VH'),
             passthrough=True):
    import torch
    from nd_amd import xr_lite
    rng = np.random.default_rng([SEED, 1000])
    host = {}
    ds = xr_lite.Dataset()
    for name in names:
        host[name] = cases.speckle(rng, shape, dtype)
        ds[name] = (dims, torch.from_numpy(host[name]).to(device) if on_device else host[name])
    if not passthrough:
        return ds, host
    host['incidence'] = rng.random(5).astype(np.float32)            # no y / x: passes through
    ds['incidence'] = (('angle',), torch.from_numpy(host['incidence']).to(device) if on_device else host['incidence'])
    return ds, host


def _values(da):
    v = da.values
    return v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)


def _planar(a, dims):
    return np.ascontiguousarray(np.transpose(a, [dims.index(d) for d in ('time', 'y', 'x')]))


@pytest.mark.parametrize('on_device', [False, True])
@pytest.mark.parametrize('dims', [('time', 'y', 'x'), ('y', 'x', 'time')])
def test_filter_classes_on_datasets(device, on_device, dims):
    import torch
    from nd_amd.filters import LeeFilter, MultitemporalFilter, lee, multitemporal
    shape = tuple({'time': 3, 'y': 37, 'x': 20}[d] for d in dims)
    ds, host = _dataset(device, on_device, dims, shape)
    back = [('time', 'y', 'x').index(d) for d in dims]

    def same(result, name, want_planar):
        da = result[name]
        assert tuple(da.dims) == dims
        assert isinstance(da.values, torch.Tensor) == on_device
        cases.assert_same(_values(da), np.ascontiguousarray(np.transpose(want_planar, back)))

    for result in (LeeFilter(w=5, looks=4.4, method='kuan').apply(ds), lee(ds, w=5, looks=4.4, method='kuan')):
        for name in ('VV', 'VH'):
            same(result, name, ref.lee(_planar(host[name], dims), 5, 4.4, 'kuan'))
        assert np.array_equal(_values(result['incidence']), host['incidence'])
    for result in (MultitemporalFilter(w=5).apply(ds), multitemporal(ds, w=5)):
        for name in ('VV', 'VH'):
            same(result, name, ref.multitemporal(_planar(host[name], dims), 5))
        assert np.array_equal(_values(result['incidence']), host['incidence'])
    joint = ref.multitemporal([_planar(host['VV'], dims), _planar(host['VH'], dims)], 5)
    for result in (MultitemporalFilter(w=5, joint=True).apply(ds), multitemporal(ds, w=5, joint=True)):
        same(result, 'VV', joint[0])
        same(result, 'VH', joint[1])
        assert np.array_equal(_values(result['incidence']), host['incidence'])
    # the caller's data is as it was
    for name in ('VV', 'VH'):
        assert np.array_equal(_values(ds[name]), host[name])
    # a DataArray alone
    cases.assert_same(_values(LeeFilter(w=3).apply(ds['VV'])),
                      np.ascontiguousarray(np.transpose(ref.lee(_planar(host['VV'], dims), 3, 1.0), back)))
    cases.assert_same(_values(MultitemporalFilter(w=3).apply(ds['VH'])),
                      np.ascontiguousarray(np.transpose(ref.multitemporal(_planar(host['VH'], dims), 3), back)))


@pytest.mark.parametrize('on_device', [False, True])
def test_chunked_runs_equal_the_whole(device, on_device):
    """njobs=2 on a 37-row raster: the halo rows make the chunks' results those of the whole, bit for bit"""
    from nd_amd.filters import LeeFilter, MultitemporalFilter
    ds, host = _dataset(device, on_device)
    flat, flat_host = _dataset(device, on_device, dims=('y', 'x'), shape=(37, 20), passthrough=False)
    for filt, data, hosts, want in (
            (LeeFilter(w=7, looks=4.4), flat, flat_host, lambda a: ref.lee(a, 7, 4.4)),
            (MultitemporalFilter(w=7), ds, host, lambda a: ref.multitemporal(a, 7)),
            (MultitemporalFilter(w=7, joint=True), ds, host, None)):
        assert filt._parallel_dimension(data) == 'y'
        whole, parts = filt.apply(data, njobs=1), filt.apply(data, njobs=2)
        for name in ('VV', 'VH'):
            cases.assert_same(_values(parts[name]), _values(whole[name]))
            if want is not None:
                cases.assert_same(_values(whole[name]), want(hosts[name]))
        if 'incidence' in hosts:
            assert np.array_equal(_values(parts['incidence']), hosts['incidence'])


def test_pixel_major_variables_through_the_planar_layout(device):
    """a contiguous (y, x, time) variable large enough for the transpose kernels, and an integer one"""
    import torch
    from nd_amd import xr_lite
    from nd_amd.filters import LeeFilter, MultitemporalFilter
    rng = np.random.default_rng([SEED, 1100])
    for dtype in (np.float32, np.float64):
        host = cases.speckle(rng, (64, 130, 8), dtype)            # (y, x, time), 66560 elements
        ds = xr_lite.Dataset()
        ds['VV'] = (('y', 'x', 'time'), torch.from_numpy(host).to(device))
        planar = np.ascontiguousarray(np.moveaxis(host, -1, 0))
        got = _values(LeeFilter(w=7, looks=4.0).apply(ds)['VV'])
        cases.assert_same(got, np.ascontiguousarray(np.moveaxis(ref.lee(planar, 7, 4.0), 0, -1)))
        got = _values(MultitemporalFilter(w=7).apply(ds)['VV'])
        cases.assert_same(got, np.ascontiguousarray(np.moveaxis(ref.multitemporal(planar, 7), 0, -1)))
    counts = (cases.speckle(rng, (3, 20, 30), np.float32) * 40).astype(np.int32)
    ds = xr_lite.Dataset()
    ds['dn'] = (('time', 'y', 'x'), counts)
    got = LeeFilter(w=3, looks=4.0).apply(ds)['dn']
    assert got.values.dtype == np.float64
    cases.assert_same(_values(got), ref.lee(counts, 3, 4.0))
    got = MultitemporalFilter(w=3).apply(ds)['dn']
    cases.assert_same(_values(got), ref.multitemporal(counts, 3))
