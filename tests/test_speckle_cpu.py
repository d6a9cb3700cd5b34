"""CPU tests of the speckle filters: they hold the restatement tests/speckle_ref.py (which the GPU tests compare the
kernels with, bit for bit) to things outside itself -- scipy's uniform_filter, an independent implementation of the
two formulas, the statistics the filters are known for -- and check the host logic of LeeFilter and
MultitemporalFilter.  Figures quoted as "measured" come from numpy.random.default_rng(0), gamma(L, 1/L) speckle
with L = 4 on 256 x 256."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import speckle_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 4.0


@pytest.fixture(scope='module')
def plane():
    return np.random.default_rng(0).gamma(L, 1.0 / L, size=(256, 256))


def enl(a):
    return float(a.mean() ** 2 / a.var())


# ------------------------------------------------------------------ the window sums
@pytest.mark.parametrize('shape', [(256, 256), (1, 1), (1, 2), (2, 5), (3, 3)])
def test_moments_against_uniform_filter(plane, shape):
    """S1 / N and S2 / N are scipy's uniform_filter with mode='reflect', also where the window (7) is larger than
    the plane.  Measured <= 3.8e-15 on the speckle plane and <= 4.5e-16 on the small ones."""
    x = plane[:shape[0], :shape[1]]
    w = 7
    s1, s2 = ref.moments(x, w)
    for got, src in ((s1 / (w * w), x), (s2 / (w * w), x * x)):
        want = ndimage.uniform_filter(src, w, mode='reflect')
        err = np.abs(got - want).max()
        print(shape, 'max abs difference', err)
        assert err <= 1e-12 * np.abs(src).max()


def test_moments_of_a_float32_plane_are_those_of_its_float64_copy(plane):
    x32 = plane.astype(np.float32)
    for a, b in zip(ref.moments(x32, 5), ref.moments(x32.astype(np.float64), 5)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ Lee / Kuan
def _direct(x, w, looks, method):
    """the two formulas from uniform_filter, float64"""
    cu2 = 1.0 / looks
    m = ndimage.uniform_filter(x, w, mode='reflect')
    v = ndimage.uniform_filter(x * x, w, mode='reflect') - m ** 2
    with np.errstate(all='ignore'):
        b = 1.0 - m ** 2 * cu2 / v
        if method == 'kuan':
            b = b / (1.0 + cu2)
    b = np.where((v > 0) & (b > 0), b, 0.0)
    return m + b * (x - m), m, v


@pytest.mark.parametrize('method', ['lee', 'kuan'])
@pytest.mark.parametrize('w', [3, 7])
def test_lee_against_direct_formula(plane, method, w):
    got = ref.lee(plane, w, L, method)
    want, m, v = _direct(plane, w, L, method)
    ok = v > 1e-6 * m ** 2
    assert ok.mean() > 0.99
    rel = np.abs(got - want)[ok] / np.abs(want)[ok]
    print(method, w, 'max relative difference', rel.max())
    assert rel.max() <= 1e-9


def test_lee_fixed_points(plane):
    ones = np.ones((9, 13))
    for method in ('lee', 'kuan'):
        assert np.array_equal(ref.lee(ones, 7, L, method), ones)                 # b = 0, m = 1 exactly
        assert np.array_equal(ref.lee(plane, 1, L, method), plane)               # w = 1: the input, bit for bit
        x32 = plane.astype(np.float32)
        assert np.array_equal(ref.lee(x32, 1, 1.0, method), x32)
        _, b = ref.lee_weight(plane, 7, L, method)
        assert b.min() >= 0.0 and b.max() < 1.0


def test_lee_returns_the_data_type():
    x = np.random.default_rng(1).gamma(L, 1.0 / L, size=(6, 7))
    assert ref.lee(x.astype(np.float32), 3, L).dtype == np.float32
    assert ref.lee(x, 3, L).dtype == np.float64
    assert ref.lee((x * 40).astype(np.int16), 3, L).dtype == np.float64


def test_lee_on_homogeneous_speckle(plane):
    """mean kept within 1e-3 (measured <= 3e-4); ENL at w = 7: 101 (lee) and 121 (kuan) against 3.99 in"""
    for method in ('lee', 'kuan'):
        out = ref.lee(plane, 7, L, method)
        print(method, 'mean', out.mean(), 'against', plane.mean(), 'ENL', enl(out), 'against', enl(plane))
        assert abs(out.mean() - plane.mean()) <= 1e-3 * plane.mean()
        assert enl(out) > 10 * enl(plane)


def test_lee_keeps_an_edge(plane):
    """a 1 : 100 step under speckle, w = 7: the last dark column has mean 7.0 filtered, 43.5 boxcar, 0.99 input"""
    x = plane.copy()
    x[:, 128:] *= 100.0
    out = ref.lee(x, 7, L, 'lee')
    box = ndimage.uniform_filter(x, 7, mode='reflect')
    print('last dark column: filtered', out[:, 127].mean(), 'boxcar', box[:, 127].mean(), 'input', x[:, 127].mean())
    assert out[:, 127].mean() < 0.5 * box[:, 127].mean()


def test_lee_keeps_a_point_target(plane):
    """a target of 1000 on unit speckle: Lee keeps 994, Kuan 800"""
    x = plane.copy()
    x[100, 90] = 1000.0
    lee, kuan = ref.lee(x, 7, L, 'lee')[100, 90], ref.lee(x, 7, L, 'kuan')[100, 90]
    print('point target of 1000: lee', lee, 'kuan', kuan)
    assert lee > 900 and kuan > 700


# ------------------------------------------------------------------ multitemporal
@pytest.mark.parametrize('w', [3, 7])
@pytest.mark.parametrize('k', [2, 5, 10])
def test_multitemporal_looks_on_homogeneous_speckle(w, k):
    """output ENL against M N L / (M + N - 1): measured 0.2 to 0.7 % below theory; mean kept within 1e-3"""
    from nd_amd.filters import multitemporal_looks
    x = np.random.default_rng(0).gamma(L, 1.0 / L, size=(k, 256, 256))
    out = ref.multitemporal(x, w)
    theory = multitemporal_looks(L, k, w)
    assert theory == ref.multitemporal_looks(L, k, w) == k * w * w * L / (k + w * w - 1.0)
    print('w', w, 'k', k, 'ENL', enl(out), 'theory', theory, 'mean', out.mean(), 'against', x.mean())
    assert abs(enl(out) - theory) <= 0.05 * theory
    assert abs(out.mean() - x.mean()) <= 1e-3 * x.mean()


def test_multitemporal_looks_counts_the_variables():
    from nd_amd.filters import multitemporal_looks
    assert multitemporal_looks(4, 6, 7, variables=2) == multitemporal_looks(4, 12, 7)
    assert multitemporal_looks(1, 1, 1) == 1.0


def test_multitemporal_of_identical_dates_is_the_input(plane):
    x = np.repeat(plane[None], 4, axis=0)
    out = ref.multitemporal(x, 7)
    assert np.abs(out - x).max() <= 1e-12 * np.abs(x).max()
    assert (np.abs(out - x) / x).max() <= 1e-12


def test_multitemporal_joint_is_the_interleaved_single_filter():
    rng = np.random.default_rng(3)
    a, b = rng.gamma(L, 1.0 / L, size=(2, 5, 20, 23)).astype(np.float32)
    ja, jb = ref.multitemporal([a, b], 5)
    inter = np.empty((10, 20, 23), np.float32)
    inter[0::2], inter[1::2] = a, b                      # (t, c) order
    one = ref.multitemporal(inter, 5)
    assert np.array_equal(ja, one[0::2]) and np.array_equal(jb, one[1::2])


# ------------------------------------------------------------------ host logic
def test_constructor_errors():
    from nd_amd.filters import LeeFilter, MultitemporalFilter
    for bad in (0, 2, 8, 33, -3, 2.5):
        with pytest.raises(ValueError):
            LeeFilter(w=bad)
        with pytest.raises(ValueError):
            MultitemporalFilter(w=bad)
    for w in (1, 3, 31):
        assert LeeFilter(w=w).w == w and MultitemporalFilter(w=w).w == w
    for looks in (0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            LeeFilter(looks=looks)
    assert LeeFilter(looks=4.4).looks == 4.4
    with pytest.raises(ValueError):
        LeeFilter(method='frost')
    with pytest.raises(ValueError):
        MultitemporalFilter(dims=('y', 'time'))


def _dataset(variables, dims=('time', 'y', 'x'), shape=(3, 6, 7), dtype=np.float32):
    from nd_amd import xr_lite
    rng = np.random.default_rng(5)
    ds = xr_lite.Dataset()
    for name in variables:
        ds[name] = (dims, rng.gamma(L, 1.0 / L, size=shape).astype(dtype))
    return ds


def test_apply_errors_need_no_gpu():
    from nd_amd import xr_lite
    from nd_amd.filters import LeeFilter, MultitemporalFilter, lee, multitemporal
    ds = _dataset(['VV', 'VH'])
    ds['C12'] = (('time', 'y', 'x'), np.ones((3, 6, 7), np.complex64))
    for call in (LeeFilter().apply, MultitemporalFilter().apply, lambda d: lee(d, w=3), lambda d: multitemporal(d)):
        with pytest.raises(TypeError, match='complex'):
            call(ds)
    assert sorted(ds.data_vars) == ['C12', 'VH', 'VV']                  # nothing was split on the way
    with pytest.raises(TypeError, match='complex'):
        LeeFilter().apply(xr_lite.DataArray(np.ones((6, 7), np.complex64), ('y', 'x')))
    # a complex variable the filter does not touch is no error of its own
    flat = _dataset(['VV'], dims=('y', 'x'), shape=(6, 7))
    with pytest.raises(KeyError, match='time'):
        MultitemporalFilter().apply(flat)
    with pytest.raises(KeyError, match='time'):
        MultitemporalFilter().apply(flat['VV'])
    with pytest.raises(NotImplementedError, match='at most 4'):
        MultitemporalFilter(joint=True).apply(_dataset(['a', 'b', 'c', 'd', 'e']))
    mixed = _dataset(['VV'])
    mixed['VH'] = (('time', 'y', 'x'), np.ones((3, 6, 7), np.float64))
    with pytest.raises(NotImplementedError, match='one type, shape and dims'):
        MultitemporalFilter(joint=True).apply(mixed)
    turned = _dataset(['VV'], shape=(6, 6, 6))
    turned['VH'] = (('y', 'x', 'time'), np.ones((6, 6, 6), np.float32))
    with pytest.raises(NotImplementedError, match='one type, shape and dims'):
        MultitemporalFilter(joint=True).apply(turned)


def test_kernel_wrappers_refuse_what_is_not_served():
    import torch
    from nd_amd import kernels as K
    x = torch.ones(3, 5, 6)
    for bad in (0, 4, 33):
        with pytest.raises(ValueError):
            K.speckle_lee(x, bad, 1.0)
        with pytest.raises(ValueError):
            K.speckle_multitemporal(x, bad)
    with pytest.raises(ValueError):
        K.speckle_lee(x, 3, 0.0)
    with pytest.raises(ValueError):
        K.speckle_lee(x, 3, 1.0, method='gamma-map')
    with pytest.raises(ValueError, match='no CPU path'):
        K.speckle_lee(x, 3, 1.0)
    with pytest.raises(ValueError, match='no CPU path'):
        K.speckle_multitemporal(x, 3)
    with pytest.raises(NotImplementedError, match='2\\^31'):
        K._speckle_plane_limit(65536, 32768)
    K._speckle_plane_limit(65536, 32767)


def test_c_entries_validate_before_any_hip_call():
    import ctypes as C
    from nd_amd import _lib
    lib = _lib.lib()
    st = _lib.i64_array([20, 5, 1])
    lee = lambda **kw: lib.nd_amd_speckle_lee(      # noqa: E731
        kw.get('src', 8), kw.get('dst', 16), kw.get('dtype', _lib.F32), 1, kw.get('ny', 4), kw.get('nx', 5), st, st,
        kw.get('w', 3), kw.get('cu2', 1.0), kw.get('method', 0), None)
    assert lee(dtype=7) == _lib.EINVAL and b'dtype' in lib.nd_amd_last_error()
    assert lee(method=2) == _lib.EINVAL
    assert lee(cu2=0.0) == _lib.EINVAL and lee(cu2=float('nan')) == _lib.EINVAL
    assert lee(w=0) == _lib.EINVAL
    assert lee(src=None) == _lib.EINVAL
    assert lee(w=4) == _lib.EUNSUPPORTED and lee(w=33) == _lib.EUNSUPPORTED
    assert lee(ny=65536, nx=32768) == _lib.EUNSUPPORTED and b'2^31' in lib.nd_amd_last_error()
    assert lee(ny=0) == _lib.OK
    ptrs = (C.c_void_p * 5)(8, 16, 24, 32, 40)
    mt = lambda **kw: lib.nd_amd_speckle_multitemporal(     # noqa: E731
        ptrs, ptrs, kw.get('nvar', 1), _lib.F32, kw.get('k', 3), kw.get('ny', 4), kw.get('nx', 5), st, st,
        kw.get('w', 3), None, 0, None)
    assert mt(nvar=0) == _lib.EINVAL
    assert mt(nvar=5) == _lib.EUNSUPPORTED
    assert mt(w=2) == _lib.EUNSUPPORTED
    assert mt(ny=65536, nx=32768) == _lib.EUNSUPPORTED
    assert mt(k=0) == _lib.OK
    assert mt(k=33) == _lib.EWORKSPACE and mt(k=17, nvar=2) == _lib.EWORKSPACE
    ws = lib.nd_amd_speckle_multitemporal_workspace_bytes
    assert ws(4, 5, 32, 1) == 0 and ws(4, 5, 16, 2) == 0 and ws(4, 5, 8, 4) == 0
    assert ws(4, 5, 33, 1) == ws(4, 5, 17, 2) == ws(4, 5, 11, 3) == 4 * 5 * 8


def test_buffer_and_parallel_dimension():
    from nd_amd.filters import LeeFilter, MultitemporalFilter
    for f in (LeeFilter(w=7), MultitemporalFilter(w=7)):
        assert f._buffer('y') == 3 and f._buffer('x') == 3 and f._buffer('time') == 0 and f._buffer('band') == 0
    assert LeeFilter(w=1)._buffer('y') == 0
    ds = _dataset(['VV'], shape=(40, 6, 9))                       # time is the longest dimension
    f = MultitemporalFilter(w=3)
    assert f.dims == ('y', 'x', 'time')
    assert f._parallel_dimension(ds) == 'x' != 'time'
    assert MultitemporalFilter(w=3)._parallel_dimension(_dataset(['VV'], shape=(40, 9, 6))) == 'y'
    assert LeeFilter()._parallel_dimension(ds) == 'time'         # planes are independent for Lee


def test_public_names_header_and_build():
    import nd_amd
    from nd_amd import _lib, build, filters, kernels
    for name in ('LeeFilter', 'lee', 'MultitemporalFilter', 'multitemporal', 'multitemporal_looks'):
        assert name in filters.__all__ and hasattr(filters, name)
    assert nd_amd.filters.LeeFilter is filters.LeeFilter
    header = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry in ('nd_amd_speckle_lee', 'nd_amd_speckle_multitemporal', 'nd_amd_speckle_multitemporal_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % entry, code) and entry in _lib.SYMBOLS
    for macro, value in (('MAX_W', _lib.SPECKLE_MAX_W), ('MAX_VARIABLES', _lib.SPECKLE_MAX_VARIABLES),
                         ('HOT_MAX_PLANES', _lib.SPECKLE_HOT_MAX_PLANES), ('TILE_Y', _lib.SPECKLE_TILE_Y),
                         ('TILE_X', _lib.SPECKLE_TILE_X), ('HOT_TILE_Y', _lib.SPECKLE_HOT_TILE_Y),
                         ('LEE', _lib.SPECKLE_METHODS['lee']), ('KUAN', _lib.SPECKLE_METHODS['kuan'])):
        assert re.search(r'#define\s+ND_AMD_SPECKLE_%s\s+%d\b' % (macro, value), header), macro
    assert kernels.SPECKLE_TILE == (_lib.SPECKLE_TILE_Y, _lib.SPECKLE_TILE_X)
    assert _lib.KERNEL_NAMES[29] == 'speckle' and re.search(r'#define\s+ND_AMD_KERNEL_SPECKLE\s+29\b', header)
    assert build.NO_SCRATCH['speckle.hip'] == 'speckle_'
    assert _lib.lib().nd_amd_abi_version() == 1


def test_the_accessor_lists_both_filters():
    from nd_amd import _xarray
    assert _xarray._METHODS['lee'] == ('filters', 'lee')
    assert _xarray._METHODS['multitemporal'] == ('filters', 'multitemporal')


def test_cases_module_is_seeded():
    from tests import speckle_cases as cases
    a = cases.random_case(np.random.default_rng([1, 2]))
    b = cases.random_case(np.random.default_rng([1, 2]))
    assert cases.describe(a) == cases.describe(b)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a['variables'], b['variables']))
    seen = [cases.random_case(np.random.default_rng([7, i])) for i in range(60)]
    assert {c['filter'] for c in seen} == {'lee', 'multitemporal'}
    assert {c['layout'] for c in seen} == set(cases.LAYOUTS)
    assert any(len(c['variables']) * c['variables'][0].shape[0] > 32 for c in seen)
    assert all(1 <= n <= 150 for c in seen for n in c['variables'][0].shape[1:])
