"""nd_amd_resample / nd_amd_resample_nearest on the device against tests/resample_ref.py: bit for bit, NaN positions
and value bits included, no tolerance and no excluded pixel (tests/resample_cases.py assert_same).  The shapes are a
few thousand pixels: output widths around the wave's 64 lanes, inner lengths that do and do not divide it, tap counts
on both sides of the kernel's register forms (<= 2, <= 3, <= 4, any) and at the cap, grids that overhang, miss or flip
the source, crops and strided outputs, every element size of nearest, non-finite samples.  Then the public layer:
Resample, Reprojection and Alignment on host and device datasets."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import resample_cases as cases
from tests import resample_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = (np.float32, np.float64)


@pytest.fixture(scope='module')
def K(device):
    from nd_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def stack():
    """(3, 41, 67) float64 gamma speckle: every test that needs 'a source' takes this one (and casts it)"""
    a = cases.source(np.random.default_rng(20261019), (3, 41, 67), np.float64)
    a.setflags(write=False)
    return a


def test_header_constant(K):
    hdr = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    assert int(re.search(r'#define ND_AMD_RESAMPLE_MAX_TAPS (\d+)', hdr).group(1)) == K.RESAMPLE_MAX_TAPS == 256


@pytest.mark.parametrize('H', [1, 5])
@pytest.mark.parametrize('W', [1, 63, 64, 65, 129])
def test_output_widths(K, stack, W, H):
    """the lanes along x and along (x, time): widths around one and two waves, one row and more rows than a block"""
    tr_s, tr_d = cases.whole_extent(41, 67, H, W)
    for method in ref.METHODS:
        for dtype in FLOATS:
            for layout in cases.LAYOUTS:
                got = cases.check(K, stack.astype(dtype), tr_s, tr_d, H, W, method, layout)
                assert np.isfinite(got).all()


@pytest.mark.parametrize('L', [1, 3, 24, 65])
def test_inner_lengths(K, L):
    """(y, x, time) with the time axis shorter than, not dividing and longer than a wave"""
    src = cases.source(np.random.default_rng(L), (L, 13, 17), np.float64)
    for method, (H, W) in zip(ref.METHODS, [(9, 23), (20, 11), (5, 40), (6, 7)]):
        tr_s, tr_d = cases.whole_extent(13, 17, H, W)
        for dtype in FLOATS:
            cases.check(K, src.astype(dtype), tr_s, tr_d, H, W, method, 'pixel')


@pytest.mark.parametrize('ratio,offset', [(0.4, 0.0), (1.0, 0.5), (2.5, 0.0), (16.0, 0.0), (2.5, 0.3), (0.4, -0.7)])
def test_ratios(K, stack, ratio, offset):
    """up-sampling, a half-pixel shift at equal size, down-sampling by 2.5 and by 16 (32 and 64 taps for bilinear and
    cubic), on the source's extent and shifted by a fraction of a source pixel"""
    src = np.concatenate([stack, stack[:, ::-1]], axis=1)[:1]           # (1, 82, 67)
    ny, nx = src.shape[1:]
    tr_s = (10.0, 0.0, 500.0, 0.0, -10.0, 900.0)
    tr_d = (10.0 * ratio, 0.0, 500.0 + 10.0 * offset, 0.0, -10.0 * ratio, 900.0 - 10.0 * offset)
    H, W = max(1, int(ny / ratio)), max(1, int(nx / ratio))
    for method in ref.METHODS:
        for dtype in FLOATS:
            for layout in cases.LAYOUTS:
                cases.check(K, src.astype(dtype), tr_s, tr_d, H, W, method, layout)


@pytest.mark.parametrize('taps', [1, 2, 3, 4, 5, 255, 256])
def test_tap_counts_around_the_register_forms_and_at_the_cap(K, taps):
    """'average' by an integer factor on aligned origins has exactly that many taps: both sides of the <= 2, <= 3 and
    <= 4 forms, and the cap, along x and along y"""
    rng = np.random.default_rng(taps)
    for axis in ('x', 'y'):
        ny, nx = (4, 3 * taps + 1) if axis == 'x' else (3 * taps + 1, 4)
        src = cases.source(rng, (2, ny, nx), np.float64, nonfinite=0.01 if taps > 5 else 0.0)
        fy, fx = (2.0, float(taps)) if axis == 'x' else (float(taps), 2.0)
        tr_s, tr_d = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (fx, 0.0, 0.0, 0.0, fy, 0.0)
        H, W = (2, 3) if axis == 'x' else (3, 2)
        t = K.resample_axis(nx if axis == 'x' else ny, 3, (1.0, 0.0), (float(taps), 0.0), 'average')
        assert t.taps == taps and int(t.count.max()) == taps
        for dtype in FLOATS:
            for layout in cases.LAYOUTS:
                cases.check(K, src.astype(dtype), tr_s, tr_d, H, W, 'average', layout)


def test_one_more_tap_raises(K):
    import torch
    from nd_amd import _lib
    n = 3 * (K.RESAMPLE_MAX_TAPS + 1)
    few = K.resample_axis(4, 2, (1.0, 0.0), (2.0, 0.0), 'average')
    many = K.resample_axis(n, 3, (1.0, 0.0), (float(K.RESAMPLE_MAX_TAPS + 1), 0.0), 'average')
    assert many.taps == K.RESAMPLE_MAX_TAPS + 1
    for shape, ty, tx in (((4, n), few, many), ((n, 4), many, few)):
        t = torch.zeros(shape, dtype=torch.float32, device='cuda')
        with pytest.raises(_lib.NdAmdError, match='at most 256') as e:
            K.resample(t, ty, tx, dims=('y', 'x'))
        assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(ValueError, match='taps'):
        K.resample_axis(100000, 2, (1.0, 0.0), (40000.0, 0.0), 'bilinear')


PLACEMENTS = {
    'left': (10.0, 430.0, -10.0, 900.0), 'right': (10.0, 900.0, -10.0, 900.0),
    'top': (10.0, 500.0, -10.0, 960.0), 'bottom': (10.0, 500.0, -10.0, 600.0),
    'all_sides': (25.0, 380.0, -25.0, 1010.0), 'outside': (10.0, 5000.0, -10.0, 900.0),
    'outside_y': (10.0, 500.0, -10.0, -900.0),
    'flip_x': (-10.0, 1170.0, -10.0, 900.0), 'flip_y': (10.0, 500.0, 10.0, 490.0),
    'flip_both': (-7.0, 1100.0, 7.0, 520.0),
}


@pytest.mark.parametrize('where', sorted(PLACEMENTS))
def test_grid_placement(K, stack, where):
    """the source spans x 500 .. 1170 and y 900 .. 490; destination grids overhang it on each side, miss it, or run
    the other way along one axis or both"""
    a, c, e, f = PLACEMENTS[where]
    tr_s, tr_d = (10.0, 0.0, 500.0, 0.0, -10.0, 900.0), (a, 0.0, c, 0.0, e, f)
    H, W = 33, 70
    for method in ref.METHODS:
        for dtype, layout in ((np.float32, 'planar'), (np.float64, 'pixel')):
            got = cases.check(K, stack.astype(dtype), tr_s, tr_d, H, W, method, layout)
            if where.startswith('outside'):
                assert np.isnan(got).all()
            else:
                assert np.isfinite(got).any()
    cases.check(K, stack.astype(np.float32), tr_s, tr_d, H, W, 'bilinear', 'planar', fill=-5.0)


def test_one_by_one_source(K):
    src = np.array([[[2.5]]])
    for method in ref.METHODS:
        for dtype in FLOATS:
            for layout in cases.LAYOUTS + ('2d',):
                got = cases.check(K, src.astype(dtype), (4.0, 0.0, 0.0, 0.0, -4.0, 0.0),
                                  (1.0, 0.0, -2.0, 0.0, -1.0, 2.0), 8, 8, method, layout)
                assert (got[0, 2:6, 2:6] == 2.5).all() and np.isnan(got[0, :2]).all() and np.isnan(got[0, :, 6:]).all()


@pytest.mark.parametrize('layout', cases.LAYOUTS + ('2d',))
def test_strides(K, stack, layout):
    """crops of larger tensors as sources and a strided view as out; nothing around the view is written"""
    src = stack[:1] if layout == '2d' else stack
    tr_s, tr_d = (10.0, 0.0, 500.0, 0.0, -10.0, 900.0), (7.0, 0.0, 480.0, 0.0, -13.0, 930.0)
    for method in ref.METHODS:
        for dtype in FLOATS:
            cases.check(K, src.astype(dtype), tr_s, tr_d, 37, 66, method, layout, crop=True)
            cases.check(K, src.astype(dtype), tr_s, tr_d, 37, 66, method, layout, strided_out=True)
            cases.check(K, src.astype(dtype), tr_s, tr_d, 37, 66, method, layout, crop=True, strided_out=True)


def test_other_axis_orders_and_two_extra_axes(K, stack):
    """dims name the axes: (y, time, x), and a (variable, time, y, x) block in one call"""
    import torch
    tr_s, tr_d = cases.whole_extent(41, 67, 30, 80)
    ty = K.resample_axis(41, 30, ref.axis_of(tr_s, 'y'), ref.axis_of(tr_d, 'y'), 'cubic')
    tx = K.resample_axis(67, 80, ref.axis_of(tr_s, 'x'), ref.axis_of(tr_d, 'x'), 'cubic')
    want = ref.regrid(stack, tr_s, tr_d, 30, 80, 'cubic')
    t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(stack, 0, 1))).cuda()
    got = K.resample(t, ty, tx, dims=('y', 'time', 'x'))
    cases.assert_same(np.moveaxis(got.cpu().numpy(), 1, 0), want)
    block = np.stack([stack, stack[::-1] * 2.0])
    got = K.resample(torch.from_numpy(block).cuda(), ty, tx, dims=('variable', 'time', 'y', 'x'))
    cases.assert_same(got.cpu().numpy(), np.stack([want, ref.regrid(stack[::-1] * 2.0, tr_s, tr_d, 30, 80, 'cubic')]))
    with pytest.raises(ValueError, match='dims'):
        K.resample(t, ty, tx, dims=('time', 'y'))
    with pytest.raises(ValueError, match='built for'):
        K.resample(t, tx, ty, dims=('y', 'time', 'x'))


@pytest.mark.parametrize('dtype', [np.uint8, np.bool_, np.int16, np.int32, np.int64, np.float32, np.float64])
def test_nearest_keeps_every_element(K, dtype):
    """elements of 1, 2, 4 and 8 bytes keep type and bits: integers beyond 2^53, NaN payloads, -0.0"""
    rng = np.random.default_rng(5)
    if dtype == np.bool_:
        src = rng.random((3, 19, 23)) < 0.5
    elif np.dtype(dtype).kind == 'f':
        src = cases.source(rng, (3, 19, 23), dtype)
        u = cases.bits(src)
        u[:, ::3, ::4] = np.array(np.nan, dtype).view(u.dtype) | 0x1234           # quiet NaNs with a payload
        u[:, 1::5, 2::3] = np.array(-0.0, dtype).view(u.dtype)
        u[:, 2, 5] = np.array(np.nan, dtype).view(u.dtype) ^ (1 << (8 * u.itemsize - 1)) | 0x77
        src = u.view(dtype)
    else:
        info = np.iinfo(dtype)
        src = rng.integers(info.min, info.max, size=(3, 19, 23), dtype=dtype, endpoint=True)
    tr_s = (1.0, 0.0, 0.0, 0.0, -1.0, 0.0)
    for tr_d, H, W in (((0.4, 0.0, -1.3, 0.0, -0.4, 1.1), 50, 66), ((2.5, 0.0, 0.0, 0.0, -2.5, 0.0), 8, 9),
                       ((-1.0, 0.0, 23.0, 0.0, 1.0, -19.0), 19, 23)):
        for layout in cases.LAYOUTS:
            got = cases.check(K, src, tr_s, tr_d, H, W, 'nearest', layout)
            assert got.dtype == src.dtype
    fill = True if dtype == np.bool_ else 3
    cases.check(K, src, tr_s, (0.4, 0.0, -1.3, 0.0, -0.4, 1.1), 50, 66, 'nearest', 'planar', fill=fill)


def test_non_finite_samples_enter_the_sums(K):
    rng = np.random.default_rng(11)
    src = cases.source(rng, (2, 40, 50), np.float64, nonfinite=0.03)
    assert np.isnan(src).any() and np.isposinf(src).any() and np.isneginf(src).any()
    for (H, W) in ((90, 120), (40, 50), (13, 17)):
        tr_s, tr_d = cases.whole_extent(40, 50, H, W)
        for method in cases.WEIGHTED:
            for dtype in FLOATS:
                for layout in cases.LAYOUTS:
                    got = cases.check(K, src.astype(dtype), tr_s, tr_d, H, W, method, layout)
                    assert np.isnan(got).any() and np.isfinite(got).any()
    # cubic by 3 on aligned origins: the taps three source pixels from the centre weigh exactly 0 INSIDE the run, and a
    # NaN under them counts (0 * NaN); the zeros at the ends of a run are trimmed and do not
    one = np.ones((1, 18, 18))
    one[0, 10, 10] = np.nan
    got = cases.check(K, one, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (3.0, 0.0, 0.0, 0.0, 3.0, 0.0), 6, 6, 'cubic')
    want = np.zeros((6, 6), bool)
    want[2:5, 2:5] = True
    assert np.array_equal(np.isnan(got[0]), want)


@pytest.mark.parametrize('dtype', [np.uint8, np.int32, np.int64, np.bool_])
def test_integer_input_to_a_weighted_method_comes_back_float64(K, dtype):
    src = cases.source(np.random.default_rng(3), (2, 21, 30), np.int64).astype(dtype)
    tr_s, tr_d = cases.whole_extent(21, 30, 9, 50)
    for method in cases.WEIGHTED:
        for layout in cases.LAYOUTS:
            got = cases.check(K, src, tr_s, tr_d, 9, 50, method, layout)
            assert got.dtype == np.float64


def test_determinism_and_one_table_pair_for_several_variables(K, stack):
    import torch
    tr_s, tr_d = (10.0, 0.0, 500.0, 0.0, -10.0, 900.0), (23.0, 0.0, 470.0, 0.0, -17.0, 930.0)
    H, W = 28, 33
    ty = K.resample_axis(41, H, ref.axis_of(tr_s, 'y'), ref.axis_of(tr_d, 'y'), 'cubic').to('cuda')
    tx = K.resample_axis(67, W, ref.axis_of(tr_s, 'x'), ref.axis_of(tr_d, 'x'), 'cubic').to('cuda')
    assert ty.to('cuda') is ty and torch.is_tensor(ty.weights) and ty.weights.is_cuda
    variables = [stack.astype(np.float32), (stack * 3).astype(np.float32), stack[::-1].astype(np.float32)]
    tensors = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in variables]
    first = [o.cpu().numpy() for o in K.resample(tensors, ty, tx)]
    second = [o.cpu().numpy() for o in K.resample(tensors, ty, tx)]
    for v, a, b in zip(variables, first, second):
        assert a.tobytes() == b.tobytes()
        cases.assert_same(a, ref.regrid(v, tr_s, tr_d, H, W, 'cubic'))
    K.resample_check_table(ty)
    K.resample_check_table(tx)


# ---- the C entries ---------------------------------------------------------------------------------------------------
def _c_args(K, torch, **over):
    from nd_amd import _lib
    src = torch.zeros((4, 6), dtype=torch.float32, device='cuda')
    dst = torch.zeros((3, 5), dtype=torch.float32, device='cuda')
    ty = K.resample_axis(4, 3, (1.0, 0.0), (1.0, 0.0), 'bilinear').to('cuda')
    tx = K.resample_axis(6, 5, (1.0, 0.0), (1.0, 0.0), 'bilinear').to('cuda')
    a = dict(src=src.data_ptr(), dst=dst.data_ptr(), dtype=_lib.F32, nplanes=1, inner=1, sny=4, snx=6,
             ss=_lib.i64_array([0, 6, 1, 0]), dny=3, dnx=5, ds=_lib.i64_array([0, 5, 1, 0]),
             sy=ty.start.data_ptr(), cy=ty.count.data_ptr(), wy=ty.weights.data_ptr(), taps_y=ty.taps,
             sx=tx.start.data_ptr(), cx=tx.count.data_ptr(), wx=tx.weights.data_ptr(), taps_x=tx.taps)
    a.update(over)
    keep = (src, dst, ty, tx)
    return a, keep


def _call(L, a, nearest=False, fill=None):
    p = lambda v: C.c_void_p(v)                 # noqa: E731
    head = [p(a['src']), p(a['dst']), a['dtype'], a['nplanes'], a['inner'], a['sny'], a['snx'], a['ss'], a['dny'],
            a['dnx'], a['ds']]
    if nearest:
        fill = C.cast(C.pointer(C.c_uint64(0)), C.c_void_p) if fill is None else fill
        return L.nd_amd_resample_nearest(*head, p(a['sy']), p(a['cy']), p(a['sx']), p(a['cx']), fill, None)
    return L.nd_amd_resample(*head, p(a['sy']), p(a['cy']), p(a['wy']), a['taps_y'], p(a['sx']), p(a['cx']),
                             p(a['wx']), a['taps_x'], float('nan'), None)


def test_c_entry_argument_errors(K):
    import torch
    from nd_amd import _lib
    L = _lib.lib()
    a, keep = _c_args(K, torch)
    assert _call(L, a) == _lib.OK
    torch.cuda.synchronize()
    bad = [(dict(dtype=7), _lib.EINVAL, b'dtype'), (dict(src=None), _lib.EINVAL, b'null'),
           (dict(dst=None), _lib.EINVAL, b'null'), (dict(sy=None), _lib.EINVAL, b'null'),
           (dict(cx=None), _lib.EINVAL, b'null'), (dict(wy=None), _lib.EINVAL, b'weights'),
           (dict(ss=None), _lib.EINVAL, b'strides'), (dict(ds=None), _lib.EINVAL, b'strides'),
           (dict(nplanes=-1), _lib.EINVAL, b'negative'), (dict(dnx=-5), _lib.EINVAL, b'negative'),
           (dict(sny=-4), _lib.EINVAL, b'negative'), (dict(inner=-1), _lib.EINVAL, b'negative'),
           (dict(taps_x=-1), _lib.EINVAL, b'negative'),
           (dict(ss=_lib.i64_array([0, -6, 1, 0])), _lib.EINVAL, b'negative stride'),
           (dict(taps_y=257), _lib.EUNSUPPORTED, b'at most 256'), (dict(taps_x=257), _lib.EUNSUPPORTED, b'at most 256'),
           (dict(sny=1 << 16, snx=1 << 15), _lib.EUNSUPPORTED, b'2^31 pixels'),
           (dict(dny=1 << 20, dnx=1 << 11), _lib.EUNSUPPORTED, b'2^31 pixels'),
           (dict(nplanes=1 << 16, inner=1 << 15), _lib.EUNSUPPORTED, b'reaches 2^31')]
    for over, code, word in bad:
        b, _ = _c_args(K, torch, **over)
        assert _call(L, b) == code, over
        assert word in L.nd_amd_last_error(), (over, L.nd_amd_last_error())
    # an empty destination is served: nothing is written, nothing is looked at
    b, _ = _c_args(K, torch, dny=0, src=None, dst=None)
    assert _call(L, b) == _lib.OK
    # the nearest entry: element sizes
    for size in (0, 3, 16, -1):
        b, _ = _c_args(K, torch, dtype=size)
        assert _call(L, b, nearest=True) == _lib.EINVAL
        assert b'elem_size' in L.nd_amd_last_error()
    b, _ = _c_args(K, torch, dtype=4)
    assert _call(L, b, nearest=True, fill=C.c_void_p(0)) == _lib.EINVAL and b'fill' in L.nd_amd_last_error()
    b, _ = _c_args(K, torch, dtype=4, sx=None)
    assert _call(L, b, nearest=True) == _lib.EINVAL and b'null' in L.nd_amd_last_error()
    b, _ = _c_args(K, torch, dtype=8, src=a['src'] + 4)
    assert _call(L, b, nearest=True) == _lib.EINVAL and b'aligned' in L.nd_amd_last_error()
    b, _ = _c_args(K, torch, dtype=4, sny=1 << 16, snx=1 << 15)
    assert _call(L, b, nearest=True) == _lib.EUNSUPPORTED
    del keep


def test_tables_that_point_outside_are_refused_and_never_followed(K):
    """count / start out of range: nd_amd_resample_check_table returns EINVAL with a message, and the kernels
    themselves give fill for such an entry instead of reading there"""
    import torch
    from nd_amd import _lib
    src = cases.source(np.random.default_rng(2), (1, 6, 8), np.float32)
    t = torch.from_numpy(src).cuda()
    good_y = K.resample_axis(6, 6, (1.0, 0.0), (1.0, 0.0), 'bilinear')
    for field, at, value in (('start', 2, -1), ('start', 7, 8), ('count', 0, 5), ('count', 3, -2)):
        tx = K.resample_axis(8, 8, (1.0, 0.0), (1.0, 0.0), 'bilinear')
        assert tx.taps == 1
        getattr(tx, field)[at] = value
        with pytest.raises(_lib.NdAmdError, match='count / start out of range') as e:
            K.resample_check_table(tx)
        assert e.value.code == _lib.EINVAL
        got = K.resample(t, good_y, tx).cpu().numpy()
        want = src.copy()
        want[:, :, at] = np.nan
        cases.assert_same(got, want)
    L = _lib.lib()
    assert L.nd_amd_resample_check_table(None, None, 4, 4, 1, None) == _lib.EINVAL and b'null' in L.nd_amd_last_error()
    assert L.nd_amd_resample_check_table(None, None, -1, 4, 1, None) == _lib.EINVAL
    assert L.nd_amd_resample_check_table(None, None, 4, 4, 257, None) == _lib.EUNSUPPORTED
    assert L.nd_amd_resample_check_table(None, None, 0, 4, 1, None) == _lib.OK


def test_cpu_tensors_and_odd_types_are_refused(K):
    import torch
    ty = K.resample_axis(4, 3, (1.0, 0.0), (1.0, 0.0), 'bilinear')
    tx = K.resample_axis(6, 5, (1.0, 0.0), (1.0, 0.0), 'bilinear')
    with pytest.raises(ValueError, match='ROCm device'):
        K.resample(torch.zeros((4, 6)), ty, tx, dims=('y', 'x'))
    with pytest.raises(TypeError, match='float32, float64 and integers'):
        K.resample(torch.zeros((4, 6), dtype=torch.float16, device='cuda'), ty, tx, dims=('y', 'x'))
    with pytest.raises(ValueError, match='out must be'):
        K.resample(torch.zeros((4, 6), device='cuda'), ty, tx, dims=('y', 'x'), out=torch.zeros((4, 6), device='cuda'))
    with pytest.raises(ValueError, match='method'):
        K.resample_axis(4, 3, (1.0, 0.0), (1.0, 0.0), 'lanczos')
    with pytest.raises(ValueError, match='pixel size'):
        K.resample_axis(4, 3, (0.0, 0.0), (1.0, 0.0), 'bilinear')


# ---- the public layer ------------------------------------------------------------------------------------------------
SRC = (10.0, 0.0, 500.0, 0.0, -10.0, 900.0)


def make_dataset(transform, ny, nx, nt=3, seed=0, on_device=False):
    """C11 (y, x, time) float32, C12 complex64, a float64 (time, y, x) plane, an odd order, integer and bool maps, and
    two variables without y and x"""
    import torch
    from nd_amd import xr_lite
    rng = np.random.default_rng(seed)
    a, _, c, _, e, f = transform
    ds = xr_lite.Dataset(coords={'x': c + a * np.arange(nx), 'y': f + e * np.arange(ny),
                                 'time': np.arange(nt) * 12.0},
                         attrs={'lines': ny, 'samples': nx, 'orbit': 'ASCENDING'})
    ds['C11'] = (('y', 'x', 'time'), cases.source(rng, (ny, nx, nt), np.float32), {'units': 'gamma0'})
    ds['C12'] = (('y', 'x', 'time'), (cases.source(rng, (ny, nx, nt), np.float32)
                                      + 1j * cases.source(rng, (ny, nx, nt), np.float32)).astype(np.complex64))
    ds['dem'] = (('time', 'y', 'x'), cases.source(rng, (nt, ny, nx), np.float64, nonfinite=0.01))
    ds['odd'] = (('x', 'time', 'y'), cases.source(rng, (nx, nt, ny), np.float32))
    ds['labels'] = (('y', 'x'), rng.integers(-5, 2 ** 40, size=(ny, nx), dtype=np.int64))
    ds['change'] = (('y', 'x', 'time'), rng.random((ny, nx, nt)) < 0.3)
    ds['doy'] = (('time',), np.arange(nt, dtype=np.int32))
    ds['bias'] = ((), np.float32(0.5))
    if on_device:
        for n in list(ds.data_vars):
            da = ds[n]
            ds[n] = (tuple(da.dims), torch.from_numpy(np.array(da.values)).cuda(), da.attrs)
    return ds


def host_values(da):
    v = da.values
    return v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)


def planes_of(values, dims):
    """(..., y, x) view of a variable's array"""
    order = [i for i, d in enumerate(dims) if d not in ('y', 'x')] + [dims.index('y'), dims.index('x')]
    return np.transpose(values, order)


def assert_regridded(src_ds, out, dst, H, W, resampling=None):
    """every variable of `out` is the restatement of its source on the grid; residence, dims, coordinates, attributes"""
    import torch
    from nd_amd import warp
    assert sorted(out.data_vars) == ['C11', 'C12__im', 'C12__re', 'bias', 'change', 'dem', 'doy', 'labels', 'odd']
    for n in out.data_vars:
        name, part = (n[:-4], n[-2:]) if n.endswith(('__re', '__im')) else (n, None)
        sda, oda = src_ds[name], out[n]
        sv = host_values(sda)
        sv = sv if part is None else (sv.real if part == 're' else sv.imag)
        assert tuple(oda.dims) == tuple(sda.dims)
        assert torch.is_tensor(oda.values) == torch.is_tensor(sda.values), n
        if torch.is_tensor(oda.values):
            assert oda.values.is_cuda
        if 'y' not in sda.dims:
            assert np.array_equal(host_values(oda), sv)
            continue
        method = resampling or ('nearest' if sv.dtype.kind in 'biu' else 'bilinear')
        want = ref.regrid(planes_of(sv, tuple(sda.dims)), SRC, dst, H, W, method)
        got = planes_of(host_values(oda), tuple(oda.dims))
        cases.assert_same(np.ascontiguousarray(got), want, payloads=method == 'nearest')
        if method == 'nearest':
            assert got.dtype == sv.dtype
    assert out['C11'].attrs['units'] == 'gamma0'
    assert np.array_equal(out.coords['x'], dst[2] + dst[0] * np.arange(W))
    assert np.array_equal(out.coords['y'], dst[5] + dst[4] * np.arange(H))
    assert np.array_equal(out.coords['time'], src_ds.coords['time'])
    assert tuple(out.attrs['transform']) == tuple(dst)
    assert (out.attrs['lines'], out.attrs['samples'], out.attrs['orbit']) == (H, W, 'ASCENDING')
    np.testing.assert_allclose(warp.get_transform(out), dst, rtol=1e-12, atol=1e-9)
    assert (out.sizes['y'], out.sizes['x']) == (H, W)


@pytest.mark.parametrize('on_device', [False, True])
def test_resample_public(K, on_device):
    from nd_amd import warp
    ds = make_dataset(SRC, 41, 67, on_device=on_device)
    out = warp.Resample(res=25.0).apply(ds)
    assert_regridded(ds, out, (25.0, 0.0, 500.0, 0.0, -25.0, 900.0), 16, 27)
    out = warp.resample(ds, width=100)
    assert_regridded(ds, out, (6.7, 0.0, 500.0, 0.0, -10.0 * 41 / 61, 900.0), 61, 100)
    out = warp.resample(ds, res=(4.0, 30.0), resampling='average')
    assert_regridded(ds, out, (4.0, 0.0, 500.0, 0.0, -30.0, 900.0), 14, 168, 'average')
    assert host_values(out['labels']).dtype == np.float64           # a weighted method on integers
    same = warp.Resample().apply(ds)
    assert_regridded(ds, same, SRC, 41, 67)
    assert 'C12' in ds.data_vars and 'transform' not in ds.attrs     # the input is left as it was


@pytest.mark.parametrize('on_device', [False, True])
def test_reprojection_public(K, on_device):
    from nd_amd import warp
    ds = make_dataset(SRC, 41, 67, seed=1, on_device=on_device)
    grid = (20.0, 0.0, 440.0, 0.0, -25.0, 960.0)
    target = make_dataset(grid, 19, 40, nt=1, seed=2)
    out = warp.Reprojection(target=target).apply(ds)
    assert_regridded(ds, out, grid, 19, 40)
    out = warp.reproject(ds, extent=(400.0, 300.0, 1000.0, 800.0), res=(20.0, 25.0), resampling='cubic')
    assert_regridded(ds, out, (20.0, 0.0, 400.0, 0.0, -25.0, 800.0), 21, 31, 'cubic')
    out = warp.reproject(ds, transform=(-7.0, 0.0, 1100.0, 0.0, 7.0, 520.0), width=33, height=20, resampling='nearest')
    assert_regridded(ds, out, (-7.0, 0.0, 1100.0, 0.0, 7.0, 520.0), 20, 33, 'nearest')
    # a DataArray comes back as one
    da = warp.reproject(ds['C11'], extent=(400.0, 300.0, 1000.0, 800.0), width=60, height=25)
    assert da.dims == ('y', 'x', 'time') and da.shape == (25, 60, 3)
    want = ref.regrid(planes_of(host_values(ds['C11']), ('y', 'x', 'time')), SRC,
                      (10.0, 0.0, 400.0, 0.0, -20.0, 800.0), 25, 60, 'bilinear')
    cases.assert_same(np.ascontiguousarray(planes_of(host_values(da), ('y', 'x', 'time'))), want)


def test_variables_with_one_of_y_and_x_are_refused(K):
    from nd_amd import warp
    ds = make_dataset(SRC, 9, 11)
    ds['profile'] = (('x',), np.zeros(11, np.float32))
    with pytest.raises(NotImplementedError, match='profile'):
        warp.resample(ds, res=20.0)


def test_alignment_feeds_the_omnibus_test(K):
    """two dual-pol stacks of different resolution and extent onto their common grid, and the aligned stack into
    OmnibusTest as it comes"""
    from nd_amd import warp, xr_lite
    from nd_amd.change import OmnibusTest
    from tests import synth

    def stack(transform, ny, nx, seed):
        planes = synth.omnibus_stack(seed=seed, k=6, ny=ny, nx=nx, dtype=np.float32, change_frac=0.1)
        a, _, c, _, e, f = transform
        ds = xr_lite.Dataset(coords={'x': c + a * np.arange(nx), 'y': f + e * np.arange(ny), 'time': np.arange(6)})
        for v, p in zip(('C11', 'C12__re', 'C12__im', 'C22'), planes):
            ds[v] = (('y', 'x', 'time'), np.ascontiguousarray(np.moveaxis(p, 0, -1)))
        return ds

    fine = stack((10.0, 0.0, 500.0, 0.0, -10.0, 900.0), 40, 60, 1)         # x 500 .. 1100, y 500 .. 900
    coarse = stack((20.0, 0.0, 440.0, 0.0, -20.0, 960.0), 18, 25, 2)       # x 440 .. 940, y 600 .. 960
    assert warp.get_common_bounds([fine, coarse]) == (440.0, 500.0, 1100.0, 960.0)
    assert warp.get_common_resolution([fine, coarse]) == (10.0, 10.0)
    aligned = warp.Alignment().apply([fine, coarse])
    grid, H, W = (10.0, 0.0, 440.0, 0.0, -10.0, 960.0), 47, 67
    assert len(aligned) == 2
    for src_ds, tr, out in ((fine, (10.0, 0.0, 500.0, 0.0, -10.0, 900.0), aligned[0]),
                            (coarse, (20.0, 0.0, 440.0, 0.0, -20.0, 960.0), aligned[1])):
        assert tuple(out.attrs['transform']) == grid and (out.sizes['y'], out.sizes['x']) == (H, W)
        for v in ('C11', 'C12__re', 'C12__im', 'C22'):
            want = ref.regrid(np.moveaxis(src_ds[v].values, -1, 0), tr, grid, H, W, 'bilinear')
            cases.assert_same(np.ascontiguousarray(np.moveaxis(out[v].values, -1, 0)), want)
    # onto a target instead
    onto = warp.align([coarse], target=fine)[0]
    assert (onto.sizes['y'], onto.sizes['x']) == (40, 60)
    np.testing.assert_allclose(warp.get_transform(onto), warp.get_transform(fine), rtol=1e-12)
    # the part both cover has no NaN; it goes into the omnibus test unchanged
    both = aligned[0].isel(y=slice(6, 36), x=slice(6, 50))
    assert all(np.isfinite(both[v].values).all() for v in both.data_vars)
    change = OmnibusTest(n=9, alpha=0.95).apply(both)
    assert change.dims == ('y', 'x', 'time') and change.shape == (30, 44, 6)
    assert np.array_equal(change.values, OmnibusTest(n=9, alpha=0.95).apply(fine.isel(y=slice(0, 30), x=slice(0, 44))).values)
