"""tests/resample_ref.py, the numpy restatement of the resampling definition (README.md "Resampling and
reprojection"), held to things it did not come from -- torch's interpolate(antialias=True), Pillow's resize, scipy's
map_coordinates, block means, conservation of mass, polynomial reproduction, hand-enumerated tables -- and
kernels.resample_axis held to the restatement's tables bit for bit.  Then the grid rules of Resample, Reprojection
and get_common_*.  No GPU."""
import warnings

import numpy as np
import pytest

from tests import resample_cases as cases
from tests import resample_ref as ref

NY, NX = 23, 31
# up, down, mixed, identity
SIZES = [(50, 70), (9, 11), (40, 13), (23, 31)]


@pytest.fixture(scope='module')
def raster():
    a = cases.source(np.random.default_rng(7), (NY, NX), np.float64)
    a.setflags(write=False)
    return a


def resize(raster, H, W, method):
    tr_s, tr_d = cases.whole_extent(NY, NX, H, W)
    return ref.regrid(raster, tr_s, tr_d, H, W, method)


# ---- torch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('method,mode', [('bilinear', 'bilinear'), ('cubic', 'bicubic')])
def test_against_torch_antialias(raster, H, W, method, mode):
    import torch
    import torch.nn.functional as F
    want = F.interpolate(torch.from_numpy(raster.copy())[None, None], size=(H, W), mode=mode, antialias=True,
                         align_corners=False)[0, 0].numpy()
    got = resize(raster, H, W, method)
    err = np.abs(got - want).max() / np.abs(raster).max()
    print('%s %dx%d: %.3g of max|src|' % (method, H, W, err))
    assert err <= 1e-12


@pytest.mark.parametrize('H,W', SIZES)
def test_nearest_against_torch_nearest_exact(raster, H, W):
    import torch
    import torch.nn.functional as F
    want = F.interpolate(torch.from_numpy(raster.copy())[None, None], size=(H, W), mode='nearest-exact')[0, 0].numpy()
    assert np.array_equal(resize(raster, H, W, 'nearest'), want)


# ---- Pillow ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('box', [None, (3.0, 2.0, 27.0, 20.0), (2.5, 1.25, 30.75, 22.5)])
@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('method', ['bilinear', 'cubic'])
def test_against_pillow(raster, H, W, method, box):
    Image = pytest.importorskip('PIL.Image')
    resample = {'bilinear': Image.BILINEAR, 'cubic': Image.BICUBIC}[method]
    img = Image.fromarray(raster.astype(np.float32))
    assert img.mode == 'F'
    want = np.asarray(img.resize((W, H), resample=resample, box=box), dtype=np.float64)
    left, upper, right, lower = box or (0.0, 0.0, float(NX), float(NY))
    tr_s = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    tr_d = ((right - left) / W, 0.0, left, 0.0, (lower - upper) / H, upper)
    got = ref.regrid(raster.astype(np.float32), tr_s, tr_d, H, W, method).astype(np.float64)
    err = np.abs(got - want).max() / np.abs(raster).max()
    print('%s %dx%d box=%s: %.3g of max|src|' % (method, H, W, box, err))
    assert err <= 1e-6


# ---- scipy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(50, 70), (23, 62), (46, 31)])
def test_upsampling_bilinear_against_map_coordinates(raster, H, W):
    from scipy.ndimage import map_coordinates
    v = (np.arange(H) + 0.5) * NY / H - 0.5
    u = (np.arange(W) + 0.5) * NX / W - 0.5
    want = map_coordinates(raster, np.meshgrid(v, u, indexing='ij'), order=1, mode='nearest')
    assert np.abs(resize(raster, H, W, 'bilinear') - want).max() <= 1e-12 * np.abs(raster).max()


# ---- average ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fy,fx', [(1, 1), (2, 2), (3, 5), (8, 1)])
def test_average_is_the_block_mean_at_integer_factors(fy, fx):
    src = cases.source(np.random.default_rng(fy * 10 + fx), (24, 30), np.float64)
    H, W = 24 // fy, 30 // fx
    got = ref.regrid(src, (10.0, 0.0, 5.0, 0.0, -10.0, 7.0), (10.0 * fx, 0.0, 5.0, 0.0, -10.0 * fy, 7.0), H, W, 'average')
    want = src.reshape(H, fy, W, fx).mean(axis=(1, 3))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(src).max()


@pytest.mark.parametrize('H,W', [(9, 11), (7, 30), (22, 3), (1, 1), (10, 13)])
def test_average_conserves_mass(raster, H, W):
    got = resize(raster, H, W, 'average')
    mass = got.sum() * (NX / W) * (NY / H)
    assert abs(mass - raster.sum()) <= 1e-12 * raster.sum()


@pytest.mark.parametrize('ratio,cx,cy', [(1.0, 0.3, 0.2), (2.0, 0.3, 0.2), (3.0, 0.0, 0.7), (4.0, 0.3, 0.2),
                                         (2.5, 0.25, 0.75)])
def test_average_reproduces_a_linear_ramp_inside(ratio, cx, cy):
    """The source is piecewise constant, so a window [lo, hi] that cuts its first pixel at t and its last at t' from
    their near edges is off the ramp by slope * (t' (1 - t') - t (1 - t)) / (2 rho): nothing where t' = t or 1 - t,
    which an integer ratio gives at any offset and 2.5 gives at offsets of a quarter pixel."""
    ny, nx = 40, 50
    i, j = np.meshgrid(np.arange(ny) + 0.5, np.arange(nx) + 0.5, indexing='ij')
    src = 2.0 + 3.0 * j + 5.0 * i
    H, W = int(ny / ratio) - 1, int(nx / ratio) - 1
    tr_d = (ratio, 0.0, cx, 0.0, ratio, cy)
    got = ref.regrid(src, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), tr_d, H, W, 'average')
    v = cy + ratio * (np.arange(H) + 0.5)
    u = cx + ratio * (np.arange(W) + 0.5)
    inside_y = (v - ratio / 2 >= 0) & (v + ratio / 2 <= ny)
    inside_x = (u - ratio / 2 >= 0) & (u + ratio / 2 <= nx)
    want = 2.0 + 3.0 * u[None, :] + 5.0 * v[:, None]
    sel = inside_y[:, None] & inside_x[None, :]
    assert sel.sum() > 10
    assert np.abs(got - want)[sel].max() <= 1e-12 * np.abs(src).max()


# ---- cubic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ratio,offset', [(1.0, 0.37), (0.4, 0.0), (0.73, 0.21), (1.0, 0.5)])
def test_cubic_reproduces_quadratics_inside(ratio, offset):
    ny, nx = 30, 36
    i, j = np.meshgrid(np.arange(ny) + 0.5, np.arange(nx) + 0.5, indexing='ij')
    quad = lambda v, u: 1.0 + 0.5 * u - 0.25 * v + 0.03 * u * u + 0.02 * v * v - 0.01 * u * v      # noqa: E731
    src = quad(i, j)
    H, W = int(ny / ratio) - 2, int(nx / ratio) - 2
    got = ref.regrid(src, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (ratio, 0.0, offset, 0.0, ratio, offset), H, W, 'cubic')
    v = offset + ratio * (np.arange(H) + 0.5)
    u = offset + ratio * (np.arange(W) + 0.5)
    sel = ((v >= 2) & (v <= ny - 2))[:, None] & ((u >= 2) & (u <= nx - 2))[None, :]
    assert sel.sum() > 100
    assert np.abs(got - quad(v[:, None], u[None, :]))[sel].max() <= 1e-12 * np.abs(src).max()


@pytest.mark.parametrize('method', ref.METHODS)
def test_zero_offset_returns_the_sample_itself(raster, method):
    assert np.array_equal(resize(raster, NY, NX, method), raster)
    f32 = raster.astype(np.float32)
    tr = (10.0, 0.0, 500.0, 0.0, -10.0, 900.0)
    assert np.array_equal(ref.regrid(f32, tr, tr, NY, NX, method), f32)


# ---- hand-enumerated tables ------------------------------------------------------------------------------------------
def table(n, m, src, dst, method):
    start, count, weights = ref.axis_table(n, m, src, dst, method)
    return start.tolist(), count.tolist(), weights


def test_inside_is_half_open_at_both_ends():
    start, count, w = table(4, 5, (1.0, 0.0), (1.0, -0.5), 'nearest')       # u = 0, 1, 2, 3, 4
    assert count == [1, 1, 1, 1, 0] and start == [0, 1, 2, 3, 0]
    start, count, w = table(4, 3, (1.0, 0.0), (1.0, -1.5), 'nearest')       # u = -1, 0, 1
    assert count == [0, 1, 1] and start == [0, 0, 1]
    start, count, w = table(4, 2, (1.0, 0.0), (1.0, float('nan')), 'bilinear')
    assert count == [0, 0]
    for method in ref.METHODS:                                              # u = -2^-50 ... 4 - 2^-50
        start, count, w = table(4, 5, (1.0, 0.0), (1.0, -0.5 - 2.0 ** -50), method)
        assert count[0] == 0 and count[4] >= 1 and start[4] + count[4] == 4


def test_negative_pixel_sizes_and_flips():
    # both sides run downwards: the same raster, the identity
    assert table(4, 4, (-1.0, 4.0), (-1.0, 4.0), 'nearest')[:2] == ([0, 1, 2, 3], [1, 1, 1, 1])
    # opposite signs: a flip
    assert table(4, 4, (1.0, 0.0), (-1.0, 4.0), 'nearest')[:2] == ([3, 2, 1, 0], [1, 1, 1, 1])
    assert table(4, 4, (-1.0, 4.0), (1.0, 0.0), 'nearest')[:2] == ([3, 2, 1, 0], [1, 1, 1, 1])
    # a flip at half the resolution: pairs of source samples from the far end
    start, count, w = table(4, 2, (-2.0, 8.0), (4.0, 0.0), 'average')
    assert (start, count) == ([2, 0], [2, 2]) and np.array_equal(w, [[0.5, 0.5], [0.5, 0.5]])
    for method in cases.WEIGHTED:
        a = ref.axis_table(9, 7, (2.0, 1.0), (-2.6, 19.0), method)
        b = ref.axis_table(9, 7, (2.0, 1.0), (2.6, 19.0 - 7 * 2.6), method)
        assert np.array_equal(a[0][::-1], b[0]) and np.array_equal(a[1][::-1], b[1])
        np.testing.assert_allclose(a[2][:, ::-1], b[2], rtol=0, atol=1e-14)


def test_one_sample_sources_and_outputs():
    for method in ref.METHODS:
        start, count, w = table(1, 3, (3.0, 0.0), (1.0, 0.0), method)
        assert (start, count) == ([0, 0, 0], [1, 1, 1]) and np.array_equal(w, [[1.0, 1.0, 1.0]])
    start, count, w = table(4, 1, (1.0, 0.0), (4.0, 0.0), 'average')
    assert (start, count) == ([0], [4]) and np.array_equal(w[:, 0], [0.25] * 4)
    start, count, w = table(4, 1, (1.0, 0.0), (4.0, 0.0), 'nearest')
    assert (start, count) == ([2], [1])
    start, count, w = table(4, 1, (1.0, 0.0), (4.0, 0.0), 'bilinear')       # u = 2, s = 4: every sample, a tent
    assert (start, count) == ([0], [4])
    np.testing.assert_allclose(w[:, 0], np.array([0.625, 0.875, 0.875, 0.625]) / 3.0, rtol=1e-15)


def test_output_wholly_outside():
    for method in ref.METHODS:
        start, count, w = table(4, 3, (1.0, 0.0), (1.0, 100.0), method)
        assert count == [0, 0, 0] and start == [0, 0, 0] and w.shape == (1, 3) and not w.any()
    out = ref.regrid(np.ones((4, 4), np.float32), (1.0, 0, 0, 0, 1.0, 0), (1.0, 0, 100.0, 0, 1.0, 0), 2, 3, 'cubic')
    assert out.dtype == np.float32 and np.isnan(out).all()
    out = ref.regrid(np.ones((4, 4), np.int32), (1.0, 0, 0, 0, 1.0, 0), (1.0, 0, 100.0, 0, 1.0, 0), 2, 3, 'nearest')
    assert out.dtype == np.int32 and not out.any()


def test_zero_weights_are_trimmed_at_the_ends_and_kept_inside():
    # cubic at integer offsets: (-0, 1, -0, 0) around the sample is trimmed to the sample
    for c in (0.0, 1.0, -2.0):
        start, count, w = table(6, 6, (1.0, 0.0), (1.0, c), 'cubic')
        inside = [0 <= j + c < 6 for j in range(6)]
        assert count == [int(v) for v in inside]
        assert [s for s, v in zip(start, inside) if v] == [int(j + c) for j, v in zip(range(6), inside) if v]
        assert w.shape == (1, 6) and np.array_equal(w[0], np.array(inside, float))
    # bilinear at integer offsets likewise; at a half-pixel shift two equal taps, one at the raster's edge
    start, count, w = table(4, 4, (1.0, 0.0), (1.0, 0.5), 'bilinear')       # u = 1, 2, 3, 4
    assert (start, count) == ([0, 1, 2, 0], [2, 2, 2, 0])
    assert np.array_equal(w, [[0.5, 0.5, 0.5, 0.0], [0.5, 0.5, 0.5, 0.0]])
    # cubic by 3 on aligned origins: zeros three samples from the centre stay inside the run of 11
    start, count, w = table(18, 6, (1.0, 0.0), (3.0, 0.0), 'cubic')
    assert (start[2], count[2]) == (2, 11)
    assert w[2, 2] == 0.0 and w[8, 2] == 0.0 and w[5, 2] > 0.3 and w[0, 2] < 0.0 and w[10, 2] < 0.0


def test_bilinear_downsampling_by_two_is_a_clipped_renormalised_tent():
    start, count, w = table(4, 2, (1.0, 0.0), (2.0, 0.0), 'bilinear')       # u = 1, 3; s = 2
    assert (start, count) == ([0, 1], [3, 3])
    np.testing.assert_allclose(w[:, 0], np.array([0.75, 0.75, 0.25]) / 1.75, rtol=1e-15)
    np.testing.assert_allclose(w[:, 1], np.array([0.25, 0.75, 0.75]) / 1.75, rtol=1e-15)


# ---- the library's table builder -------------------------------------------------------------------------------------
def test_resample_axis_equals_the_restatement_bit_for_bit():
    from nd_amd import kernels
    rng = np.random.default_rng(20261019)
    special = [(4, 5, (1.0, 0.0), (1.0, -0.5)), (4, 2, (1.0, 0.0), (1.0, float('nan'))), (1, 3, (3.0, 0.0), (1.0, 0.0)),
               (4, 3, (1.0, 0.0), (1.0, 100.0)), (18, 6, (1.0, 0.0), (3.0, 0.0)), (0, 3, (1.0, 0.0), (1.0, 0.0)),
               (5, 0, (1.0, 0.0), (1.0, 0.0)), (771, 3, (1.0, 0.0), (257.0, 0.0))]
    for it in range(400):
        n, m = (int(v) for v in rng.integers(1, 200, size=2))
        ratio = float(np.exp(rng.uniform(np.log(0.05), np.log(40.0))))
        if rng.random() < 0.3:
            ratio = float(rng.choice([0.25, 0.5, 1.0, 2.0, 2.5, 4.0, 16.0]))
        a_s = float(rng.choice([1.0, -1.0, 10.0, -0.3]))
        a_d = a_s * ratio * float(rng.choice([1.0, 1.0, -1.0]))
        c_s = float(rng.uniform(-5, 5))
        c_d = c_s + a_s * (float(rng.integers(-2, n)) if rng.random() < 0.3 else float(rng.uniform(-3, n + 3)))
        special.append((n, m, (a_s, c_s), (a_d, c_d)))
    for n, m, src, dst in special:
        for method in ref.METHODS:
            start, count, weights = ref.axis_table(n, m, src, dst, method)
            t = kernels.resample_axis(n, m, src, dst, method)
            assert (t.n, t.m, t.method, t.taps) == (n, m, method, weights.shape[0])
            assert t.start.dtype == np.int32 and t.count.dtype == np.int32 and t.weights.dtype == np.float64
            assert np.array_equal(t.start, start) and np.array_equal(t.count, count), (n, m, src, dst, method)
            assert t.weights.shape == weights.shape
            assert np.array_equal(t.weights.view(np.int64), weights.view(np.int64)), (n, m, src, dst, method)
    assert kernels.RESAMPLE_MAX_TAPS == 256


# ---- the grids of the public layer -----------------------------------------------------------------------------------
SRC = (10.0, 0.0, 500.0, 0.0, -10.0, 900.0)


def test_resample_grid():
    from nd_amd.warp import resample_grid
    assert resample_grid(SRC, 41, 67) == (SRC, 41, 67)
    # res wins over width / height; the extent is the raster's, the signs the source's
    assert resample_grid(SRC, 41, 67, res=25, width=3, height=4) == ((25.0, 0.0, 500.0, 0.0, -25.0, 900.0), 16, 27)
    assert resample_grid(SRC, 41, 67, res=(20.0, 5.0)) == ((20.0, 0.0, 500.0, 0.0, -5.0, 900.0), 82, 34)
    assert resample_grid(SRC, 41, 67, res=1e6) == ((1e6, 0.0, 500.0, 0.0, -1e6, 900.0), 1, 1)
    flipped = (-10.0, 0.0, 1170.0, 0.0, 10.0, 490.0)
    assert resample_grid(flipped, 41, 67, res=20) == ((-20.0, 0.0, 1170.0, 0.0, 20.0, 490.0), 21, 34)
    # width and height: the pixel size follows; one of them: the aspect ratio (nd/warp.py:635-638)
    t, H, W = resample_grid(SRC, 41, 67, width=30, height=20)
    assert (H, W) == (20, 30) and t == (10.0 * 67 / 30, 0.0, 500.0, 0.0, -10.0 * 41 / 20, 900.0)
    assert resample_grid(SRC, 41, 67, width=30)[1:] == (int(41 * 30 / 67), 30)
    assert resample_grid(SRC, 41, 67, height=20)[1:] == (20, int(67 * 20 / 41))
    with pytest.raises(ValueError, match='rotated'):
        resample_grid((10.0, 0.1, 500.0, 0.0, -10.0, 900.0), 41, 67, res=20)
    with pytest.raises(ValueError, match='positive'):
        resample_grid(SRC, 41, 67, res=-1)


def test_reproject_grid():
    from nd_amd.warp import reproject_grid
    given = (7.0, 0.0, 480.0, 0.0, -13.0, 930.0)
    assert reproject_grid(SRC, 41, 67, transform=given, width=66, height=37) == (given, 37, 66)
    with pytest.raises(ValueError, match='rotated'):
        reproject_grid(SRC, 41, 67, transform=(7.0, 0.0, 480.0, 0.5, -13.0, 930.0), width=66, height=37)
    with pytest.raises(ValueError, match='`width` and `height`'):
        reproject_grid(SRC, 41, 67, transform=given, width=66)
    # extent with res: nd/warp.py:668-671; the origin is the corner the source's signs start from
    extent = (400.0, 300.0, 1000.0, 800.0)
    assert reproject_grid(SRC, 41, 67, extent=extent, res=(20.0, 25.0)) == ((20.0, 0.0, 400.0, 0.0, -25.0, 800.0), 21, 31)
    assert reproject_grid(SRC, 41, 67, extent=extent, res=7.0)[1:] == (int(500 / 7.0) + 1, int(600 / 7.0) + 1)
    up = (-10.0, 0.0, 1170.0, 0.0, 10.0, 490.0)
    assert reproject_grid(up, 41, 67, extent=extent, res=20.0) == ((-20.0, 0.0, 1000.0, 0.0, 20.0, 300.0), 26, 31)
    # extent with width and height
    assert reproject_grid(SRC, 41, 67, extent=extent, width=60, height=25) == ((10.0, 0.0, 400.0, 0.0, -20.0, 800.0), 25, 60)
    with pytest.raises(ValueError, match='resolution'):
        reproject_grid(SRC, 41, 67, extent=extent, width=60)
    # neither transform nor extent: Resample's rule
    assert reproject_grid(SRC, 41, 67, res=25) == ((25.0, 0.0, 500.0, 0.0, -25.0, 900.0), 16, 27)


def lite(transform, ny, nx, nt=2, seed=0):
    from nd_amd import xr_lite
    a, _, c, _, e, f = transform
    ds = xr_lite.Dataset(coords={'x': c + a * np.arange(nx), 'y': f + e * np.arange(ny), 'time': np.arange(nt)})
    ds['C11'] = (('y', 'x', 'time'), cases.source(np.random.default_rng(seed), (ny, nx, nt), np.float32))
    return ds


def test_constructor_checks_and_transform_round_trip():
    from nd_amd import warp
    for name in ('src_crs', 'dst_crs', 'crs'):
        with pytest.raises(NotImplementedError, match=name):
            warp.Reprojection(**{name: 'EPSG:4326'})
    with pytest.raises(ValueError, match='`width` and `height`'):
        warp.Reprojection(transform=SRC, width=4)
    with pytest.raises(ValueError, match='resolution'):
        warp.Reprojection(extent=(0, 0, 1, 1), height=4)
    with pytest.raises(ValueError, match='rotated'):
        warp.Reprojection(transform=(1.0, 0.2, 0.0, 0.0, 1.0, 0.0), width=4, height=4)
    for cls in (warp.Resample, warp.Reprojection, warp.Alignment):
        with pytest.raises(NotImplementedError, match='lanczos'):
            cls(resampling='lanczos')
        with pytest.raises(ValueError, match='resampling'):
            cls(resampling='sharpest')
        assert cls(resampling='average').resampling == 'average'
    target = lite((20.0, 0.0, 440.0, 0.0, -20.0, 960.0), 12, 17)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        r = warp.Reprojection(target=target, res=5.0, width=3)
    assert sorted(str(w.message) for w in seen) == ['`res` is ignored if `target` is specified.',
                                                    '`width` is ignored if `target` is specified.']
    assert (r.transform, r.height, r.width, r.res, r.extent) == ((20.0, 0.0, 440.0, 0.0, -20.0, 960.0), 12, 17, None, None)
    # coordinates laid out as the result's are give the grid back
    for t in (SRC, (22.333333333333332, 0.0, 500.1, 0.0, -22.77777777777778, 900.7), (-0.3, 0.0, 7.0, 0.0, 0.3, -2.0)):
        np.testing.assert_allclose(warp.get_transform(lite(t, 18, 30)), t, rtol=1e-12, atol=1e-12)


def test_common_bounds_and_resolution():
    from nd_amd import warp
    a = lite((10.0, 0.0, 500.0, 0.0, -10.0, 900.0), 41, 67)              # x 500 .. 1170, y 490 .. 900
    b = lite((20.0, 0.0, 440.0, 0.0, -25.0, 960.0), 12, 17, seed=1)      # x 440 .. 780, y 660 .. 960
    c = lite((-5.0, 0.0, 1200.0, 0.0, 5.0, 400.0), 30, 40, seed=2)       # x 1000 .. 1200, y 400 .. 550
    assert warp.get_common_bounds([a, b]) == (440.0, 490.0, 1170.0, 960.0)
    assert warp.get_common_bounds([a, b, c]) == (440.0, 400.0, 1200.0, 960.0)
    assert warp.get_common_resolution([a, b, c]) == (5.0, 5.0)
    assert warp.get_common_resolution([a, b], mode='max') == (20.0, 25.0)
    assert warp.get_common_resolution([a, b], mode='mean') == (15.0, 17.5)
    with pytest.raises(ValueError, match='Unsupported mode'):
        warp.get_common_resolution([a, b], mode='median')
    with pytest.raises(NotImplementedError, match='files'):
        warp.Alignment().apply(['a.nc'])
    with pytest.raises(ValueError, match='No datasets'):
        warp.Alignment().apply([])
