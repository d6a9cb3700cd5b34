"""to_rgb without a GPU: the numpy restatement (tests/rgb_ref.py) against np.nanpercentile and against
numpy 2.2.6's recorded output (tests/golden/to_rgb_numpy.npz), the composite restatement against
numpy's own evaluation of the stretch, the C ABI declarations, and argument errors."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from tests import rgb_cases, rgb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'to_rgb_numpy.npz')
NAMES = tuple(rgb_cases.planes(np.float32))
NEW_SYMBOLS = ('nd_amd_rgb_limits_workspace_bytes', 'nd_amd_rgb_limits', 'nd_amd_rgb_compose')


def same(a, b):
    """value ==, NaN where NaN, same dtype"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def numpy_percentile(a, p):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                   # all-NaN slice
        with np.errstate(all='ignore'):
            return np.nanpercentile(a, p)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def golden_planes(g, dtype):
    tag = np.dtype(dtype).name
    return {n: g['%s/%s/plane' % (tag, n)] for n in NAMES}


def test_golden_is_numpy_2_2_6_and_covers_the_cases(golden):
    assert str(golden['numpy_version']) == '2.2.6'
    assert tuple(golden['percentiles']) == rgb_cases.PERCENTILES
    for dt in rgb_cases.DTYPES:
        p = golden_planes(golden, dt)
        assert np.isnan(p['all_nan']).all() and np.isnan(p['some_nan']).any()
        assert np.isposinf(p['infinities']).any() and np.isneginf(p['infinities']).any()
        d = p['denormal_zero']
        assert (np.abs(d[d != 0]) < np.finfo(dt).tiny).all() and np.signbit(d[d == 0]).any()
        assert len(np.unique(p['ties16'])) == 16 and len(np.unique(p['constant'])) == 1
        assert p['size1'].size == 1 and p['size2'].size == 2 and p['odd'].size % 2 == 1
        assert (p['negative'] < 0).any()


@pytest.mark.parametrize('dtype', rgb_cases.DTYPES)
@pytest.mark.parametrize('name', NAMES)
def test_restatement_matches_numpy_and_golden(golden, dtype, name):
    a = golden_planes(golden, dtype)[name]
    assert a.dtype == dtype
    np.testing.assert_array_equal(a, rgb_cases.planes(dtype)[name])
    rec = golden['%s/%s/pct' % (np.dtype(dtype).name, name)]
    for j, p in enumerate(rgb_cases.PERCENTILES):
        got = rgb_ref.nanpercentile(a, p)
        assert same(got, numpy_percentile(a, p)), (name, p, got)
        assert same(got, rec[j]), (name, p, got, rec[j])


def test_restatement_beyond_2_24_values():
    """4100 x 4100 float32: n - 1 is not a float32, the virtual index is coarse, and numpy is followed."""
    a = np.random.default_rng(5).exponential(size=(4100, 4100)).astype(np.float32)
    a[::1000, ::5] = np.nan
    for p in (2, 98, 99.9, 100):
        assert same(rgb_ref.nanpercentile(a, p), numpy_percentile(a, p)), p
    b = a[~np.isnan(a)]
    assert b.size > 2 ** 24
    for p in (2, 50, 100):
        assert same(rgb_ref.nanpercentile(b, p), numpy_percentile(b, p)), p


def _trio(g, dtype):
    p = golden_planes(g, dtype)
    return [p['exponential'][:32, :32], p['scaled_1e6'], p['one_binade'][:32, :32]]


@pytest.mark.parametrize('dtype', rgb_cases.DTYPES)
def test_composite_restatement_matches_numpy(golden, dtype):
    tag = np.dtype(dtype).name
    planes = golden_planes(golden, dtype)
    for name, a in planes.items():
        got = rgb_ref.composite([a])
        np.testing.assert_array_equal(got, rgb_ref.numpy_composite([a]), err_msg=name)
        np.testing.assert_array_equal(got, golden['%s/%s/grey' % (tag, name)], err_msg=name)
    tri = _trio(golden, dtype)
    np.testing.assert_array_equal(rgb_ref.composite(tri), golden['%s/rgb' % tag])
    mask = np.random.default_rng(2).random(tri[0].shape) < 0.5
    for kw in (dict(), dict(vmin=0.25, vmax=2.5), dict(vmin=[0.1, 3e5, 1.2], vmax=[2, 4e6, 1.7]),
               dict(vmin=0.5), dict(vmax=[1.5, 2e6, 1.9]), dict(vmin=1, vmax=1), dict(vmin=5, vmax=2),
               dict(vmin=1e30), dict(pmin=98, pmax=2), dict(pmin=2.5, pmax=99.9), dict(mask=mask),
               dict(vmin=0.1, mask=mask)):
        np.testing.assert_array_equal(rgb_ref.composite(tri, **kw), rgb_ref.numpy_composite(tri, **kw), err_msg=str(kw))
        np.testing.assert_array_equal(rgb_ref.composite(tri[:1], **{k: (v[0] if isinstance(v, list) else v)
                                                                    for k, v in kw.items()}),
                                      rgb_ref.numpy_composite(tri[:1], **{k: (v[0] if isinstance(v, list) else v)
                                                                  for k, v in kw.items()}), err_msg=str(kw))
    ints = [(a * 40).astype(np.uint8) for a in tri]
    np.testing.assert_array_equal(rgb_ref.composite(ints), rgb_ref.numpy_composite(ints))


def test_bool_plane_raises_in_numpy():
    with pytest.raises(TypeError):
        np.nanpercentile(np.zeros((4, 4), bool), 2)


def test_header_and_binding_declare_the_new_symbols():
    from nd_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    for s in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, header), s
        assert s in _lib.SYMBOLS
    assert _lib.KERNEL_NAMES[15] == 'rgb_limits' and _lib.KERNEL_NAMES[16] == 'rgb_compose'
    assert re.search(r'#define\s+ND_AMD_KERNEL_RGB_LIMITS\s+15\b', header)
    assert re.search(r'#define\s+ND_AMD_KERNEL_RGB_COMPOSE\s+16\b', header)


def _call_limits(L, dtype=0, nchan=1, nframes=1, ny=4, nx=4, strides=(16, 4, 1), pmin=2.0, pmax=98.0):
    vp = ctypes.c_void_p
    num = (vp * 3)(256, 256, 256)
    return L.nd_amd_rgb_limits(num, None, nchan, dtype, nframes, ny, nx, *strides, pmin, pmax, vp(256), vp(256),
                               vp(256), 1 << 30, None)


def _call_compose(L, dtype=0, nchan=1, nframes=1, ny=4, nx=4, strides=(16, 4, 1), limits=256, vmin=None):
    vp = ctypes.c_void_p
    num = (vp * 3)(256, 256, 256)
    return L.nd_amd_rgb_compose(num, None, nchan, dtype, nframes, ny, nx, *strides, vp(limits), vmin, None, None,
                                vp(256), None)


def test_bad_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call, so it needs no device (the pointers are never read)."""
    from nd_amd import _lib
    L = _lib.lib()
    msg = lambda: L.nd_amd_last_error().decode()
    for call in (_call_limits, _call_compose):
        assert call(L, dtype=7) == _lib.EINVAL and 'dtype' in msg()
        assert call(L, ny=-1) == _lib.EINVAL and 'shape' in msg()
        assert call(L, nframes=-2) == _lib.EINVAL and 'shape' in msg()
        for nchan in (0, 2, 4):
            assert call(L, nchan=nchan) == _lib.EINVAL and 'channels' in msg()
        assert call(L, strides=(16, -4, 1)) == _lib.EINVAL and 'stride' in msg()
    for kw in (dict(pmin=-0.5), dict(pmax=100.5), dict(pmin=float('nan'))):
        assert _call_limits(L, **kw) == _lib.EINVAL and '[0, 100]' in msg()
    assert _call_compose(L, limits=0) == _lib.EINVAL and 'vmin' in msg()
    assert L.nd_amd_rgb_limits_workspace_bytes(7, 3) == 0
    assert L.nd_amd_rgb_limits_workspace_bytes(0, 0) == 0
    assert L.nd_amd_rgb_limits_workspace_bytes(0, 72) >= 72 * 3 * 4 * 2048 * 4
    assert L.nd_amd_rgb_limits_workspace_bytes(1, 72) >= 72 * 6 * 4 * 2048 * 4
    vp = ctypes.c_void_p
    num = (vp * 3)(256, 256, 256)
    rc = L.nd_amd_rgb_limits(num, None, 1, 0, 1, 4, 4, 16, 4, 1, 2.0, 98.0, vp(256), vp(256), vp(256), 16, None)
    assert rc == _lib.EWORKSPACE and 'workspace' in msg()


def test_to_rgb_argument_errors_need_no_gpu():
    from nd_amd import visualize
    a = np.ones((4, 5), np.float32)
    with pytest.raises(ValueError, match='two-dimensional'):
        visualize.to_rgb(np.ones((2, 4, 5), np.float32))
    with pytest.raises(ValueError):
        visualize.to_rgb('nothing')
    for kw in (dict(output='x.png'), dict(categorical=True), dict(cmap='jet'), dict(shape=(8, 10))):
        with pytest.raises(NotImplementedError, match='cv2'):
            visualize.to_rgb(a, **kw)
    with pytest.raises(ValueError):
        visualize.to_rgb([a, a])
