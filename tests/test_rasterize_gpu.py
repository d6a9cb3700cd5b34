"""nd_amd_rasterize_polygons on the device against tests/rasterize_ref.py: equal everywhere, no tolerance and no
excluded pixels.  The shapes are the smallest at which the kernel can go wrong: box widths and edge counts around
the wave's 64 lanes, crossing counts on both sides of the LDS list's capacity, polygons off the raster, overlap
order, layers, strides, value bits."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import rasterize_cases as cases
from tests import rasterize_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K(device):
    from nd_amd import kernels
    return kernels


def burn(K, polys, values, ny, nx, **kw):
    """the device result as a numpy array (nlayers, ny, nx)"""
    verts, ro, po = ref.pack(polys)
    return K.rasterize_polygons(verts, ro, po, values, ny, nx, **kw).cpu().numpy()


def check(K, polys, ny, nx, values=None, **kw):
    values = np.arange(1, len(polys) + 1) if values is None else values
    got = burn(K, polys, values, ny, nx, **kw)
    want = ref.burn(polys, values, ny, nx, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    return got


def test_constants_agree(K):
    assert K.RASTERIZE_MAX_CROSSINGS == cases.MAX_CROSSINGS
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nd_amd.h')).read()
    assert int(re.search(r'#define ND_AMD_RASTERIZE_MAX_CROSSINGS (\d+)', hdr).group(1)) == cases.MAX_CROSSINGS


@pytest.mark.parametrize('width', [1, 63, 64, 65, 129])
def test_box_widths(K, width):
    """the lane stride over columns: a slanted quadrilateral whose clipped box is `width` columns wide (the host's
    box is the extent and a pixel beyond, so the raster itself sets the width)"""
    ny, nx = 7, width
    quad = [np.array([(-0.7, 0.8), (width + 0.4, 0.3), (width - 0.2, 6.1), (0.45, 5.7)])]
    got = check(K, [quad], ny, nx)
    assert got.any()
    # and strictly inside a wider raster, the box limited by the polygon
    inner = [np.array([(2.3, 0.8), (2.3 + width - 0.6, 0.3), (2.3 + width - 0.9, 6.1), (2.6, 5.7)])]
    check(K, [inner], ny, width + 6)


@pytest.mark.parametrize('m', [3, 64, 65, 200])
def test_edge_counts(K, m):
    """the lane stride over edges: rings of m edges, regular and star-shaped (several crossings a row)"""
    rng = np.random.default_rng(m)
    ny, nx = 37, 41
    polys = [[cases.regular_ring(m, 20.3, 18.1, 17.2)], [cases.star(rng, 19.0, 18.0, 18.0, m)],
             [cases.star(rng, 21.0, 17.0, 16.0, m), cases.star(rng, 21.0, 17.0, 5.0, m, spread=0.3)]]
    got = check(K, polys, ny, nx)
    assert len(np.unique(got)) == 4


@pytest.mark.parametrize('crossings', [cases.MAX_CROSSINGS - 2, cases.MAX_CROSSINGS, 2 * cases.MAX_CROSSINGS + 2])
def test_comb_list_and_fallback(K, crossings):
    """teeth 0.05 pixel wide: 2 * MAX + 2 crossings on every row of an 8 x 40 raster force the per-pixel walk,
    MAX - 2 (and MAX itself) stay in the list form; a plain polygon shares the launch"""
    polys = [cases.comb(crossings), [np.array([(3.2, 1.1), (30.0, 2.0), (17.0, 7.9)])]]
    x1, y1, x2, y2 = ref.edges(polys[0])
    assert int(((y1 <= 3.5) & ~(y2 <= 3.5)).sum()) == crossings
    got = check(K, polys, 8, 40)
    assert (got == 1).any() and (got == 2).any()
    check(K, polys[:1], 8, 40)


def test_outside_covering_and_thin_rasters(K):
    ny, nx = 9, 13
    everything = [np.array([(-3., -2.), (20., -2.), (20., 15.), (-3., 15.)])]
    polys = [[np.array([(-6., 2.), (4.5, 1.), (3., 7.5), (-2., 8.)])],            # partly outside, left
             [np.array([(9.5, -4.), (16., 3.), (10.5, 12.), (8., 4.)])],          # over three borders
             [np.array([(20., 20.), (30., 20.), (25., 28.)])],                    # wholly outside
             [np.array([(-9., -9.), (-1., -9.), (-1., -1.)])]]
    got = check(K, polys, ny, nx)
    assert not (got == 3).any() and not (got == 4).any() and (got == 1).any() and (got == 2).any()
    assert (check(K, [everything], ny, nx) == 1).all()
    got = check(K, polys + [everything], ny, nx)
    assert (got == 5).all()
    assert (check(K, [everything] + polys, ny, nx) == 1).any()
    thin = [[np.array([(0.2, -1.), (70.3, 0.2), (40., 3.)])], [np.array([(10.5, 0.5), (20.5, 0.5), (15., 0.6)])]]
    check(K, thin, 1, 77)
    check(K, [[r[:, ::-1] for r in g] for g in thin], 77, 1)
    check(K, [everything], 1, 1)


def test_zero_polygons_and_empty_rasters(K):
    got = burn(K, [], np.zeros(0, np.int64), 5, 6, fill=7)
    assert got.shape == (1, 5, 6) and got.dtype == np.int64 and (got == 7).all()
    got = burn(K, [], np.zeros(0), 5, 6, nlayers=2, fill=-1.5)
    assert got.shape == (2, 5, 6) and got.dtype == np.float64 and (got == -1.5).all()
    sq = [[np.array([(0., 0.), (2., 0.), (2., 2.)])]]
    assert burn(K, sq, [1], 0, 6).shape == (1, 0, 6)
    assert burn(K, sq, [1], 4, 0).shape == (1, 4, 0)
    assert burn(K, sq, [1], 4, 4, layer=None, nlayers=1).any()
    # polygons without rings, and rings too short to enclose anything
    got = check(K, [[], [np.array([(0., 0.), (4., 4.)])], sq[0], [np.zeros((0, 2))]], 4, 4)
    assert set(np.unique(got)) == {0, 3}


def test_overlap_order(K):
    """300 overlapping polygons on 64 x 64: the highest index wins everywhere; reversed, another exact result"""
    rng = np.random.default_rng(300)
    polys = cases.overlapping(rng, 300, 64, 64)
    values = np.arange(1, 301)
    fwd = check(K, polys, 64, 64, values=values)
    rev = check(K, polys[::-1], 64, 64, values=values[::-1])
    assert (fwd != rev).any()
    assert len(np.unique(fwd)) > 20


def test_waves_serve_several_items_in_turn(K):
    """More (polygon, row) items than the fill kernel's grid has waves (16 384 blocks x 4), so waves come round
    for a second item and reuse their crossing list: 600 tall few-edge polygons over most rows of a 128-row raster,
    with combs on both sides of the list's capacity first, in the middle and last, so that a wave meets the list
    form and the per-pixel walk back to back in either order, and rows without a crossing (the box's spare rows)
    in between."""
    rng = np.random.default_rng(600)
    ny, nx = 128, 56
    few, many = cases.MAX_CROSSINGS - 2, 2 * cases.MAX_CROSSINGS + 2
    polys = []
    for k in range(600):
        cx, w = rng.uniform(0, nx), rng.uniform(1.5, 9.0)
        y0, y1 = rng.uniform(-2, 6), rng.uniform(ny - 7, ny + 2)
        m = int(rng.integers(3, 7))
        ring = [(cx - w, y0), (cx + w * rng.uniform(-0.5, 1), y0 + rng.uniform(0, 3))]
        ring += [(cx + w * rng.uniform(0.2, 1), y) for y in np.sort(rng.uniform(y0 + 3, y1, m - 2))]
        ring += [(cx - w * rng.uniform(0.2, 1), y1)]
        polys.append([np.asarray(ring)])
    tall = dict(ytop=ny - 0.4)
    for at, crossings in ((0, many), (1, few), (300, many), (301, few)):
        polys.insert(at, cases.comb(crossings, **tall))
    polys += [cases.comb(few, **tall), cases.comb(many, **tall)]
    boxes, row_work = K.polygon_boxes(*ref.pack(polys), ny, nx)
    assert row_work[-1] > 16384 * 4 + 4000, row_work[-1]
    # second-round items 65 536 ... fall on the last eighty polygons; their waves' first items were the combs and
    # polygons at the front, and the per-pixel comb at the very end follows plain polygons
    assert row_work[2] == 2 * ny and row_work[-1] - row_work[-2] == ny
    values = rng.permutation(len(polys)) + 1
    got = check(K, polys, ny, nx, values=values)
    assert len(np.unique(got)) > 50


def test_device_argument_forms(K):
    """device='cuda' (no index) names the current device: the same result, on the device, one shared table"""
    import torch
    from nd_amd import vector
    host = stack()
    feats = world_features(host)
    want = vector.rasterize(feats, host)
    for device in ('cuda', torch.device('cuda'), 'cuda:0', torch.device('cuda', 0)):
        got = vector.rasterize(feats, host, device=device)
        for name in ('class', 'id'):
            assert got[name].values.is_cuda
            np.testing.assert_array_equal(got[name].values.cpu().numpy(), want[name].values)
    polys = [[np.array([(1., 1.), (5., 1.), (5., 5.)])]]
    table = K.PolygonTable(*ref.pack(polys), 6, 7, device='cuda')
    assert table.device == torch.device('cuda', torch.cuda.current_device())
    np.testing.assert_array_equal(K.rasterize_polygons(table, None, None, [3], 6, 7).cpu().numpy(),
                                  ref.burn(polys, [3], 6, 7))
    geometry = vector._Geometry(polys, 6, 7)
    a = vector._burn(geometry, np.array([3]), None, 1, 0, 'cuda')
    first = geometry._table
    b = vector._burn(geometry, np.array([4]), None, 1, 0, torch.device('cuda:0'))
    assert geometry._table is first and a.is_cuda and int(b.max()) == 4


def test_coordinate_cap(K):
    """coordinates up to 2^40 pixels are served exactly (a polygon reaching far off the raster), beyond they raise"""
    big = float(2 ** 40)
    polys = [[np.array([(-big, -3.0), (big, 2.5), (big * 0.5, 40.0), (-7.25, 12.0)])],
             [np.array([(3.0, -big), (9.5, big), (-big, 5.0)])]]
    got = check(K, polys, 17, 23)
    assert (got == 1).any() and (got == 2).any()
    bad = [[np.array([(0.0, 0.0), (big * 2, 1.0), (3.0, 9.0)])]]
    with pytest.raises(ValueError, match='2\\^40'):
        K.rasterize_polygons(*ref.pack(bad), [1], 17, 23)


def test_layers_into_a_strided_output(K):
    """three layers written into a (y, x, time) buffer through its permuted view; layer 0 never marks layer 1"""
    import torch
    rng = np.random.default_rng(8)
    ny, nx = 33, 47
    polys = cases.overlapping(rng, 40, ny, nx)
    layer = rng.integers(0, 3, len(polys))
    values = rng.integers(1, 1000, len(polys))
    want = ref.burn(polys, values, ny, nx, layer=layer, nlayers=3, fill=-4)
    buf = torch.full((ny, nx, 3), 99, dtype=torch.int64, device='cuda')
    out = K.rasterize_polygons(*ref.pack(polys), values, ny, nx, layer=layer, nlayers=3, fill=-4,
                               out=buf.permute(2, 0, 1))
    assert out.data_ptr() == buf.data_ptr()
    np.testing.assert_array_equal(buf.cpu().numpy(), np.moveaxis(want, 0, -1))
    assert (want[0] != want[1]).any() and (want[1] != want[2]).any()
    one = [[np.array([(1., 1.), (20., 1.), (20., 20.), (1., 20.)])]]
    got = check(K, one, ny, nx, values=[5], layer=[0], nlayers=2)
    assert (got[0] == 5).any() and not got[1].any()
    # a padded, offset view
    big = torch.zeros((3, ny + 2, nx + 5), dtype=torch.int64, device='cuda')
    K.rasterize_polygons(*ref.pack(polys), values, ny, nx, layer=layer, nlayers=3, fill=-4,
                         out=big[:, 1:ny + 1, 3:nx + 3])
    np.testing.assert_array_equal(big[:, 1:ny + 1, 3:nx + 3].cpu().numpy(), want)
    assert not big[:, 0].any() and not big[:, :, :3].any() and not big[:, :, nx + 3:].any()


def test_value_bits(K):
    rng = np.random.default_rng(9)
    ny, nx = 21, 19
    polys = cases.overlapping(rng, 6, ny, nx) + [[np.array([(0., 0.), (9., 0.), (9., 9.), (0., 9.)])]]
    ints = np.array([2 ** 53 + 1, -(2 ** 53) - 3, 2 ** 63 - 1, -2 ** 63, -1, 0, 2 ** 62 + 12345], dtype=np.int64)
    got = check(K, polys, ny, nx, values=ints, fill=-2 ** 60 - 1)
    assert (got == 2 ** 62 + 12345).any() and (got == -2 ** 60 - 1).any()
    nan_payload = np.frombuffer(np.uint64(0x7ff8000000abcdef).tobytes(), np.float64)[0]
    floats = np.array([np.nan, -0.0, np.inf, -np.inf, 5e-324, nan_payload, -0.0])
    for fill in (0.0, -0.0, np.nan, 2.5):
        want = ref.burn(polys, floats, ny, nx, fill=fill)
        got = burn(K, polys, floats, ny, nx, fill=fill)
        assert got.dtype == np.float64
        assert got.tobytes() == want.tobytes()
    assert np.signbit(got[0, 1, 1]) and got[0, 1, 1] == 0


def test_half_integer_snapped_cases(K):
    for name, rings, ny, nx in cases.snapped_cases():
        check(K, [rings], ny, nx)
    # and the hand-enumerated half-open square
    sq = [[np.array([(0.5, 0.5), (2.5, 0.5), (2.5, 2.5), (0.5, 2.5)])]]
    np.testing.assert_array_equal(burn(K, sq, [1], 4, 4)[0],
                                  [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])


def test_matplotlib_cases_on_the_device(K):
    for name, rings, ny, nx in cases.matplotlib_cases()[:12]:
        check(K, [rings], ny, nx)


@pytest.mark.parametrize('seed', [0, 1])
def test_tiling_fan_on_the_device(K, seed):
    rng = np.random.default_rng([78, seed])
    ny, nx = 70, 83
    hull, tris = cases.fan(rng, ny, nx, m=11)
    if seed:
        hull = [cases.snap(hull[0])]
        centre = cases.snap(tris[0][0][:1])[0]
        tris = [[np.stack([centre, hull[0][k], hull[0][(k + 1) % 11]])] for k in range(11)]
    # every triangle in a layer of its own: disjoint and complete
    layers = burn(K, tris, np.ones(11, np.int64), ny, nx, layer=np.arange(11), nlayers=11)
    assert layers.sum(0).max() == 1
    whole = burn(K, [hull], [1], ny, nx)[0]
    np.testing.assert_array_equal(layers.sum(0), whole)
    assert whole.sum() > 1000
    # and in one layer: nothing dropped whatever the order
    np.testing.assert_array_equal(burn(K, tris[::-1], np.ones(11, np.int64), ny, nx)[0], whole)


def test_two_runs_give_identical_bytes(K):
    rng = np.random.default_rng(11)
    polys = cases.overlapping(rng, 200, 64, 64)
    values = rng.standard_normal(200)
    a = burn(K, polys, values, 64, 64)
    b = burn(K, polys, values, 64, 64)
    assert a.tobytes() == b.tobytes()


def test_polygon_table_is_shared_and_tensors_are_accepted(K):
    import torch
    rng = np.random.default_rng(12)
    polys = cases.overlapping(rng, 30, 40, 48)
    verts, ro, po = ref.pack(polys)
    table = K.PolygonTable(verts, ro, po, 40, 48)
    values = np.arange(1, 31)
    want = ref.burn(polys, values, 40, 48)
    np.testing.assert_array_equal(K.rasterize_polygons(table, None, None, values, 40, 48).cpu().numpy(), want)
    fl = K.rasterize_polygons(table, None, None, torch.arange(1, 31, device='cuda').double(), 40, 48)
    np.testing.assert_array_equal(fl.cpu().numpy(), want.astype(np.float64))
    dv = K.rasterize_polygons(torch.from_numpy(verts).cuda(), ro, po, torch.arange(1, 31, device='cuda'), 40, 48)
    np.testing.assert_array_equal(dv.cpu().numpy(), want)
    with pytest.raises(ValueError, match='no CPU path'):
        K.rasterize_polygons(torch.from_numpy(verts), ro, po, values, 40, 48)
    with pytest.raises(ValueError, match='no CPU path'):
        K.rasterize_polygons(verts, ro, po, torch.arange(1, 31), 40, 48)
    with pytest.raises(ValueError, match='non-finite'):
        K.rasterize_polygons(np.where(verts == verts[3], np.nan, verts), ro, po, values, 40, 48)
    with pytest.raises(ValueError, match='one per polygon'):
        K.rasterize_polygons(verts, ro, po, values[:-1], 40, 48)
    with pytest.raises(ValueError, match='layer numbers'):
        K.rasterize_polygons(verts, ro, po, values, 40, 48, layer=np.full(30, 2), nlayers=2)
    with pytest.raises(ValueError, match='offsets'):
        K.rasterize_polygons(verts, ro[::-1].copy(), po, values, 40, 48)
    with pytest.raises(ValueError, match='2\\^32'):
        K.rasterize_polygons(verts, ro, po, values, 70000, 70000)


# ---- through the public call --------------------------------------------------------------------------------------
def stack(ny=40, nx=48, nt=3, on_device=False, seed=0):
    import torch
    from nd_amd import xr_lite
    rng = np.random.default_rng(seed)
    coords = {'y': 500.0 - 10.0 * np.arange(ny), 'x': 200.0 + 10.0 * np.arange(nx),
              'time': np.array(['2020-01-01', '2020-01-13', '2020-01-25'][:nt], dtype='datetime64[ns]')}
    data = {}
    for name in ('C11', 'C22'):
        a = rng.gamma(4.0, 0.25, (ny, nx, nt)).astype(np.float32)
        data[name] = (('y', 'x', 'time'), torch.from_numpy(a).cuda() if on_device else a)
    return xr_lite.Dataset(data, coords=coords)


def world_features(ds, n=14, seed=3):
    """n labelled parcels in world coordinates over the stack's grid -> (features, pixel polygons)"""
    from nd_amd import warp
    a, _, c, _, e, f = warp.get_transform(ds)
    rng = np.random.default_rng(seed)
    ny, nx = ds.sizes['y'], ds.sizes['x']
    polys = cases.overlapping(rng, n, ny, nx)
    feats = []
    for k, rings in enumerate(polys):
        world = [np.stack([c + a * r[:, 0], f + e * r[:, 1]], axis=1) for r in rings]
        feats.append({'type': 'Feature', 'properties': {'class': ('crop', 'forest', 'water')[k % 3], 'id': k + 1},
                      'geometry': {'type': 'Polygon', 'coordinates': [w.tolist() for w in world]}})
    return feats


def restated_labels(ds, feats, column_values):
    from nd_amd import warp
    t = warp.get_transform(ds)
    polys = [[ref.to_pixel(np.asarray(r), t) for r in f['geometry']['coordinates']] for f in feats]
    return ref.burn(polys, column_values, ds.sizes['y'], ds.sizes['x'])[0]


def test_public_call_residence(K):
    import torch
    from nd_amd import vector
    host, dev = stack(), stack(on_device=True)
    feats = world_features(host)
    a = vector.rasterize(feats, host)
    b = vector.rasterize(feats, dev)
    c = vector.rasterize(feats, host, device='cuda:0')
    assert isinstance(a['class'].values, np.ndarray) and a['class'].values.dtype == np.int64
    assert torch.is_tensor(b['class'].values) and b['class'].values.is_cuda and b['class'].values.dtype == torch.int64
    assert torch.is_tensor(c['id'].values) and c['id'].values.is_cuda
    assert a['class'].dims == ('y', 'x', 'time') and a['class'].shape == (40, 48, 1)
    for name in ('class', 'id'):
        np.testing.assert_array_equal(a[name].values, b[name].values.cpu().numpy())
        np.testing.assert_array_equal(a[name].values, c[name].values.cpu().numpy())
    codes = [{'crop': 1, 'forest': 2, 'water': 3}[f['properties']['class']] for f in feats]
    np.testing.assert_array_equal(a['class'].values[..., 0], restated_labels(host, feats, codes))
    np.testing.assert_array_equal(a['id'].values[..., 0], restated_labels(host, feats, np.arange(1, len(feats) + 1)))
    assert a['class'].attrs['legend'] == [(0, None), (1, 'crop'), (2, 'forest'), (3, 'water')]
    assert len(np.unique(a['class'].values)) == 4
    shapes = [[np.asarray(r) for r in f['geometry']['coordinates']] for f in feats]
    s_host = vector.rasterize_shapes(shapes, host)
    s_dev = vector.rasterize_shapes(shapes, dev)
    assert isinstance(s_host.values, np.ndarray) and s_dev.values.is_cuda and s_host.dims == ('y', 'x')
    np.testing.assert_array_equal(s_host.values, a['id'].values[..., 0])
    np.testing.assert_array_equal(s_dev.values.cpu().numpy(), s_host.values)


def test_labels_go_into_the_classifier_unchanged(K):
    """make_Xy with the device-resident int64 labels of rasterize equals make_Xy with the restatement's labels
    as a numpy array (40 x 48 x 3 dates)"""
    from sklearn.ensemble import RandomForestClassifier
    from nd_amd import vector
    from nd_amd.classify import Classifier
    ds = stack(on_device=True)
    feats = world_features(ds)
    labels = vector.rasterize(feats, ds)['class'].squeeze()
    assert labels.values.is_cuda and labels.dims == ('y', 'x')
    codes = [{'crop': 1, 'forest': 2, 'water': 3}[f['properties']['class']] for f in feats]
    want_labels = restated_labels(ds, feats, codes)
    clf = Classifier(RandomForestClassifier(5, random_state=0))
    X, y = clf.make_Xy(ds, labels)
    Xw, yw = clf.make_Xy(ds, want_labels)
    assert y.dtype == np.int64 and yw.dtype == np.int64 and len(y) == 3 * int((want_labels > 0).sum()) > 100
    np.testing.assert_array_equal(X, Xw)
    np.testing.assert_array_equal(y, yw)
    fitted = clf.fit(ds, labels)
    assert 0.0 <= fitted.score(ds, labels) <= 1.0
    assert fitted.score(ds, labels) == Classifier(RandomForestClassifier(5, random_state=0)).fit(
        ds, want_labels).score(ds, want_labels)


# ---- argument errors of the C entry ----------------------------------------------------------------------------------
def test_c_entry_argument_errors(K):
    """EINVAL with a message before any HIP call: the output stays as it was"""
    import torch
    from nd_amd import _lib
    L = _lib.lib()
    ny, nx = 6, 7
    polys = [[np.array([(1., 1.), (5., 1.), (5., 5.)])]]
    table = K.PolygonTable(*ref.pack(polys), ny, nx)
    vals = torch.tensor([3], dtype=torch.int64, device='cuda')
    out = torch.full((1, ny, nx), 42, dtype=torch.int64, device='cuda')
    need = L.nd_amd_rasterize_workspace_bytes(1, ny, nx)
    assert need >= 4 * ny * nx and need % 256 == 0
    assert L.nd_amd_rasterize_workspace_bytes(0, ny, nx) == 0
    assert L.nd_amd_rasterize_workspace_bytes(1, 65536, 65536) == 0
    assert L.nd_amd_rasterize_workspace_bytes(1, 65536, 65535) == 4 * 65536 * 65535
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    fill = C.c_int64(0)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(verts=p(table.verts), ro=p(table.ring_offsets), po=p(table.poly_offsets), layer=C.c_void_p(0),
                rw=p(table.row_work), boxes=p(table.boxes), values=p(vals), dtype=_lib.I64,
                fill=C.cast(C.pointer(fill), C.c_void_p), npolys=1, nlayers=1, ny=ny, nx=nx, out=p(out), sl=ny * nx,
                sy=nx, sx=1, ws=p(ws), wsb=need, stream=C.c_void_p(0))
    order = ('verts', 'ro', 'po', 'layer', 'rw', 'boxes', 'values', 'dtype', 'fill', 'npolys', 'nlayers', 'ny', 'nx',
             'out', 'sl', 'sy', 'sx', 'ws', 'wsb', 'stream')

    def call(**change):
        return L.nd_amd_rasterize_polygons(*[dict(good, **change)[k] for k in order])
    null = C.c_void_p(0)
    bad = [dict(verts=null), dict(ro=null), dict(po=null), dict(rw=null), dict(boxes=null), dict(values=null),
           dict(fill=null), dict(out=null), dict(ws=null), dict(dtype=_lib.F32), dict(dtype=7), dict(npolys=-1),
           dict(nlayers=-1), dict(ny=-1), dict(nx=-2), dict(npolys=2 ** 32 - 1), dict(npolys=2 ** 40),
           dict(ny=65536, nx=65536), dict(nlayers=2 ** 32), dict(ny=2 ** 62, nx=4), dict(wsb=need - 1), dict(wsb=0),
           dict(sy=-1), dict(ws=C.c_void_p(ws.data_ptr() + 8))]
    for change in bad:
        rc = call(**change)
        msg = L.nd_amd_last_error().decode()
        assert rc == _lib.EINVAL, (change, rc)
        assert 'nd_amd_rasterize_polygons' in msg, (change, msg)
    torch.cuda.synchronize()
    assert (out == 42).all()
    # empty rasters are fine without an output or a workspace; then the good call
    assert call(ny=0, out=null, ws=null, wsb=0) == _lib.OK
    assert call(nlayers=0, out=null, ws=null, wsb=0) == _lib.OK
    assert call() == _lib.OK
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), ref.burn(polys, [3], ny, nx))
    assert call(npolys=0, verts=null, ro=null, po=null, rw=null, boxes=null, values=null) == _lib.OK
    torch.cuda.synchronize()
    assert (out == 0).all()
