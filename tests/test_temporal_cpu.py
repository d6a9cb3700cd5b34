"""Statistics along time without a GPU: the restatement (tests/temporal_ref.py) held to things outside it -- numpy
2.2.6's nanpercentile / percentile, nanmedian / median, nanmin / nanmax / nanargmin / nanargmax by ==, exact arithmetic
for the sums -- then the header, the entry's argument checks before it touches the device, and the host logic of
nd_amd.temporal with the restatement standing in for the kernels."""
import contextlib
import ctypes
import fractions
import math
import os
import re
import warnings

import numpy as np
import pytest

from tests import temporal_cases as cases
from tests import temporal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 3, 7, 8, 9, 17, 24, 33, 64, 65, 130)
PS = (0, 2, 25, 33.3, 50, 98, 100)
U = 2.0 ** -53                  # the unit roundoff of float64


def _series(rng, k, dtype, plane=(6, 11)):
    """finite gamma speckle, 15 % NaN, 10 % of one constant, one all-NaN pixel, one pixel with a single valid date"""
    return cases.with_special_pixels(cases.speckle(rng, (k,) + plane, dtype, nan=0.15, ties=0.1))


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert (got[ok] == want[ok]).all(), '%s: %d of %d differ' % (what, (got[ok] != want[ok]).sum(), ok.sum())


# ---- the restatement against numpy -----------------------------------------------------------------------------------
@pytest.mark.parametrize('skipna', [True, False])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_order_statistics_are_numpys(dtype, skipna):
    """no pixel excluded: the all-NaN pixel is NaN in both, with skipna=False every pixel with a NaN is"""
    rng = np.random.default_rng(20261022)
    for k in KS:
        x = _series(rng, k, dtype)
        got = ref.stats(x, 0, skipna, 0, PS)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                 # all-NaN slices
            for p in PS:
                want = (np.nanpercentile if skipna else np.percentile)(x, p, axis=0)
                _equal(got[ref.name(p)], want, 'k = %d, p = %g' % (k, p))
            _equal(got['median'], (np.nanmedian if skipna else np.median)(x, axis=0), 'k = %d, median' % k)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_extremes_are_numpys(dtype):
    rng = np.random.default_rng(20261023)
    for k in KS:
        x = _series(rng, k, dtype)
        got = ref.stats(x)
        has = got['count'] > 0
        assert not has.all() and (got['argmin'][~has] == -1).all() and np.isnan(got['min'][~has]).all()
        sub = x[:, has]
        assert (got['min'][has] == np.nanmin(sub, 0)).all() and (got['max'][has] == np.nanmax(sub, 0)).all()
        assert (got['argmin'][has] == np.nanargmin(sub, 0)).all() and (got['argmax'][has] == np.nanargmax(sub, 0)).all()
        assert np.array_equal(got['count'], (~np.isnan(x)).sum(0)) and got['count'].dtype == np.int32
        assert np.array_equal(got['nan_count'], np.isnan(x).sum(0))
        full = ref.stats(x, skipna=False)
        dirty = np.isnan(x).any(0)
        assert (full['count'] == k).all() and np.isnan(full['min'][dirty]).all() and np.isnan(full['sum'][dirty]).all()
        assert (full['argmax'][dirty] == np.isnan(x).argmax(0)[dirty]).all()
        assert (full['argmin'][~dirty] == x[:, ~dirty].argmin(0)).all()


# ---- the moments -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_sums_against_exact_arithmetic(dtype):
    """sum against math.fsum and m2 against the exact sum of the squares around the restatement's own mean, on a
    handful of pixels: both within k * u * (the sum of the terms' magnitudes).  The sequential sum of k terms errs by
    at most (k - 1) * u of that and a term of m2 by 3 u of itself, so series of 8 dates and more are taken."""
    rng = np.random.default_rng(20261024)
    for k in (8, 24, 130):
        x = _series(rng, k, dtype, plane=(2, 4))
        got = ref.stats(x)
        for iy, ix in ((0, 2), (0, 3), (1, 0), (1, 3)):
            v = [float(t) for t in x[:, iy, ix] if t == t]
            assert len(v) == got['count'][iy, ix] and len(v) > 1
            assert abs(got['sum'][iy, ix] - math.fsum(v)) <= k * U * math.fsum(abs(t) for t in v)
            mean = fractions.Fraction(float(got['mean'][iy, ix]))
            terms = [(fractions.Fraction(t) - mean) ** 2 for t in v]
            assert abs(fractions.Fraction(float(got['m2'][iy, ix])) - sum(terms)) <= fractions.Fraction(k * U) * sum(terms)


def test_derived_moments_and_the_ddof_edge():
    rng = np.random.default_rng(20261025)
    x = _series(rng, 9, 'float32')
    for ddof in (0, 1, 2):
        got = ref.stats(x, ddof=ddof)
        n, m2, mean = got['count'].astype(np.float64), got['m2'], got['mean']
        with np.errstate(all='ignore'):
            assert np.array_equal(mean, got['sum'] / n, equal_nan=True)
            ok = got['count'] - ddof > 0
            assert np.isnan(got['var'][~ok]).all() and np.isnan(got['std'][~ok]).all() and np.isnan(got['cv'][~ok]).all()
            assert (~ok).any() and ok.any()
            assert np.array_equal(got['var'][ok], (m2 / (n - ddof))[ok])
            assert np.array_equal(got['std'][ok], np.sqrt(m2 / (n - ddof))[ok])
            assert np.array_equal(got['cv'][ok], (np.sqrt(m2 / (n - ddof)) / mean)[ok])
    # the single valid date: n = 1
    one = ref.stats(x, ddof=1)
    assert one['count'][0, 1] == 1 and np.isnan(one['var'][0, 1]) and ref.stats(x)['var'][0, 1] == 0.0
    assert ref.stats(x)['count'][0, 0] == 0 and np.isnan(ref.stats(x)['mean'][0, 0]) and ref.stats(x)['sum'][0, 0] == 0.0


def test_other_types_are_computed_as_float64():
    rng = np.random.default_rng(20261026)
    change = rng.random((24, 3, 5)) < 0.2
    got = ref.stats(change, q=(50,))
    assert got['sum'].dtype == np.float64 and got['median'].dtype == np.float64 and got['p50'].dtype == np.float64
    assert np.array_equal(got['sum'], change.sum(0))
    dn = rng.integers(-300, 300, size=(7, 3, 5)).astype(np.int16)
    assert np.array_equal(ref.stats(dn)['max'], dn.max(0)) and np.array_equal(ref.stats(dn)['median'], np.median(dn, 0))


# ---- the header and the entry ----------------------------------------------------------------------------------------
def test_exports_and_header():
    from nd_amd import _lib, _xarray, temporal
    from nd_amd import kernels as K
    hdr = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bnd_amd_temporal_stats\s*\(', code) and 'nd_amd_temporal_stats' in _lib.SYMBOLS
    assert 'in_form' not in hdr and 'TEMPORAL_FORM' not in hdr      # the tests' entry is no part of the C ABI
    assert hasattr(_lib.lib(), 'nd_amd_temporal_stats')
    assert 'Statistics along time' in hdr
    assert _lib.KERNEL_NAMES[32] == 'temporal' and re.search(r'#define\s+ND_AMD_KERNEL_TEMPORAL\s+32\b', hdr)
    import torch
    for name, table in (('REG', K.TEMPORAL_REG_MAX), ('LDS', K.TEMPORAL_LDS_MAX)):
        for suffix, t in (('F32', torch.float32), ('F64', torch.float64)):
            m = re.search(r'#define\s+ND_AMD_TEMPORAL_%s_MAX_%s\s+(\d+)' % (name, suffix), hdr)
            assert m and int(m.group(1)) == table[t]
    assert all(K.TEMPORAL_REG_MAX[t] < K.TEMPORAL_LDS_MAX[t] for t in K.TEMPORAL_REG_MAX)
    assert temporal.STATS == K.TEMPORAL_STATS == ref.STATS
    assert set(temporal.__all__) == {'temporal_stats', 'composite', 'TemporalStatistics', 'temporal_statistics', 'STATS'}
    assert _xarray._METHODS['temporal_stats'] == ('temporal', 'temporal_stats')
    assert _xarray._METHODS['composite'] == ('temporal', 'composite')
    src = open(os.path.join(ROOT, 'nd_amd', 'csrc', 'temporal.hip')).read()
    assert not re.search(r'getenv|env_int|env_double|atomic', src)
    from nd_amd import build
    assert build.NO_SCRATCH['temporal.hip'] == 'temporal_'


def _call(L, ptr=None, dtype=0, k=9, ny=4, nx=5, strides=(20, 5, 1), skipna=1, ddof=0, q=(), out=None, form=0):
    from nd_amd import _lib
    outs = [out] + [None] * 12 + [out if q else None]
    qs = (ctypes.c_double * len(q))(*q) if q else None
    args = (ptr, dtype, k, ny, nx, _lib.i64_array(strides), skipna, ddof, qs, len(q)) + tuple(outs)
    if not form:
        return L.nd_amd_temporal_stats(*args, None)
    fn = L.nd_amd_temporal_stats_in_form                    # the tests' entry: in no header, bound here
    fn.restype, fn.argtypes = ctypes.c_int, list(L.nd_amd_temporal_stats.argtypes[:-1]) + [ctypes.c_int, ctypes.c_void_p]
    return fn(*args, form, None)


def test_argument_validation_without_gpu():
    """every refusal below comes before the first HIP call"""
    from nd_amd import _lib
    L = _lib.lib()
    dummy = ctypes.c_void_p(4096)
    assert _call(L, dummy, dtype=4, out=dummy) == _lib.EINVAL and b'dtype' in L.nd_amd_last_error()
    assert _call(L, dummy, k=0, out=dummy) == _lib.EINVAL and b'dates' in L.nd_amd_last_error()
    assert _call(L, dummy, k=-3, out=dummy) == _lib.EINVAL
    assert _call(L, dummy, ny=-1, out=dummy) == _lib.EINVAL
    for bad in ((-20, 5, 1), (20, -5, 1), (20, 5, -1)):
        assert _call(L, dummy, strides=bad, out=dummy) == _lib.EINVAL and b'negative stride' in L.nd_amd_last_error()
    assert _call(L, dummy, ddof=-1, out=dummy) == _lib.EINVAL and b'ddof' in L.nd_amd_last_error()
    for bad in ((-0.5,), (50.0, 100.5), (float('nan'),)):
        assert _call(L, dummy, q=bad, out=dummy) == _lib.EINVAL and b'[0, 100]' in L.nd_amd_last_error()
    assert _call(L, dummy, form=7, out=dummy) == _lib.EINVAL and b'form' in L.nd_amd_last_error()
    assert _call(L, None, out=dummy) == _lib.EINVAL and b'null' in L.nd_amd_last_error()
    assert _call(L, dummy, ny=1 << 16, nx=1 << 15, out=dummy) == _lib.EUNSUPPORTED
    # 2^27 rows of two pixels that do not lie back to back: more blocks than a launch holds
    assert _call(L, dummy, ny=1 << 27, nx=2, strides=(1 << 29, 4, 1), out=dummy) == _lib.EUNSUPPORTED
    assert b'blocks' in L.nd_amd_last_error()
    # order statistics beyond the LDS form, and a named form that does not serve the length
    assert _call(L, dummy, k=_lib.TEMPORAL_LDS_MAX[_lib.F32] + 1, q=(50.0,), out=dummy) == _lib.EUNSUPPORTED
    assert b'not served' in L.nd_amd_last_error()
    assert _call(L, dummy, dtype=1, k=_lib.TEMPORAL_LDS_MAX[_lib.F64] + 1, q=(50.0,), out=dummy) == _lib.EUNSUPPORTED
    assert _call(L, dummy, k=_lib.TEMPORAL_REG_MAX[_lib.F32] + 1, out=dummy, form=1) == _lib.EUNSUPPORTED
    assert _call(L, dummy, q=(50.0,), out=dummy, form=3) == _lib.EUNSUPPORTED
    # nothing to do: an empty plane (the pointers are not looked at), no output asked for
    assert _call(L, None, ny=0, out=dummy) == _lib.OK and _call(L, None, nx=0) == _lib.OK
    assert _call(L, dummy) == _lib.OK


def test_python_errors_without_gpu():
    import torch
    from nd_amd import kernels as K
    from nd_amd import temporal, xr_lite
    ds = xr_lite.Dataset(coords={'time': np.arange(3), 'y': np.arange(4), 'x': np.arange(5)})
    ds['a'] = (('time', 'y', 'x'), np.zeros((3, 4, 5), np.float32))
    with pytest.raises(ValueError, match='stats'):
        temporal.temporal_stats(ds, ('mode',))
    with pytest.raises(ValueError, match='stats'):
        temporal.composite(ds, 'mode')
    for bad in (-1, 100.5, (2, 101), 'p2', float('nan')):
        with pytest.raises(ValueError, match=r'\[0, 100\]'):
            temporal.temporal_stats(ds, q=bad)
    with pytest.raises(ValueError, match=r'\[0, 100\]'):
        temporal.composite(ds, 120)
    with pytest.raises(ValueError, match='ddof'):
        temporal.TemporalStatistics(ddof=-1)
    with pytest.raises(ValueError, match='no variable has'):
        temporal.temporal_stats(ds, dim='date')
    with pytest.raises(ValueError, match='no variable has'):
        temporal.composite(ds['a'], dim='band')
    cplx = xr_lite.Dataset()
    cplx['c'] = (('time', 'y', 'x'), np.zeros((3, 4, 5), np.complex64))
    with pytest.raises(TypeError, match='complex'):
        temporal.temporal_stats(cplx)
    deep = xr_lite.Dataset()
    deep['d'] = (('time', 'band', 'y', 'x'), np.zeros((3, 2, 4, 5), np.float32))
    with pytest.raises(NotImplementedError, match='dims besides'):
        temporal.temporal_stats(deep)
    with pytest.raises(ValueError, match='ROCm device'):
        K.temporal_stats(torch.zeros((3, 4, 5)))
    with pytest.raises(TypeError, match='complex'):
        K.temporal_stats(torch.zeros((3, 4, 5), dtype=torch.complex64))
    with pytest.raises(ValueError, match='three axes'):
        K.temporal_stats(torch.zeros((3, 4)))
    assert K.temporal_percentiles(None) == () and K.temporal_percentiles(2) == (2.0,)
    assert K.temporal_percentiles([2, 97.5]) == (2.0, 97.5)
    for twice in ((2, 50, 2.0), (33.33333, 33.333334)):
        with pytest.raises(ValueError, match='share a name'):
            temporal.temporal_stats(ds, q=twice)
    assert [K.temporal_percentile_name(p) for p in (2.0, 97.5, 33.3, 100.0, 0.0)] == ['p2', 'p97.5', 'p33.3', 'p100', 'p0']


# ---- nd_amd.temporal's host logic, with the restatement standing in for the kernel -----------------------------------
@pytest.fixture
def on_the_restatement(monkeypatch):
    import torch
    from nd_amd import kernels as K
    from nd_amd import temporal

    def stats(x, stats=('mean', 'std'), q=(), skipna=True, ddof=0, axis=0, _form='auto'):
        stats = (stats,) if isinstance(stats, str) else tuple(stats)
        got = ref.stats(x.numpy(), axis, skipna, ddof, q)
        return {s: torch.from_numpy(np.ascontiguousarray(got[s])) for s in stats + tuple(ref.name(p) for p in q)}

    monkeypatch.setattr(K, 'temporal_stats', stats)
    monkeypatch.setattr(temporal._device, 'device_of', lambda *a, **k: torch.device('cpu'))
    monkeypatch.setattr(temporal, '_on', lambda dev: contextlib.nullcontext())
    return temporal


def test_names_dims_coords_and_pass_through(on_the_restatement):
    from nd_amd import xr_lite
    temporal = on_the_restatement
    rng = np.random.default_rng(20261027)
    vv = cases.speckle(rng, (9, 4, 5), 'float32')
    vh = cases.speckle(rng, (4, 5, 9), 'float64')
    ds = xr_lite.Dataset(coords={'time': np.arange(9), 'y': np.arange(4) * 2.0, 'x': np.arange(5)}, attrs={'sensor': 'S1'})
    ds['VV'] = (('time', 'y', 'x'), vv, {'units': 'linear'})
    ds['VH'] = (('y', 'x', 'time'), vh)
    ds['line'] = (('time', 'x'), vv[:, 0])
    ds['dem'] = (('y', 'x'), np.ones((4, 5)))
    out = temporal.temporal_stats(ds, ('mean', 'argmax'), q=(2, 97.5, 33.3))
    keys = ['mean', 'argmax', 'p2', 'p97.5', 'p33.3']
    assert sorted(out.data_vars) == sorted(['dem'] + ['%s__%s' % (v, s) for v in ('VV', 'VH', 'line') for s in keys])
    assert list(out.coords) == ['y', 'x'] and out.attrs == {'sensor': 'S1'}
    assert out['VV__p97.5'].dims == ('y', 'x') and out['VH__mean'].dims == ('y', 'x') and out['line__p2'].dims == ('x',)
    assert out['VV__mean'].attrs == {'units': 'linear'} and out['dem'].values is ds['dem'].values
    want = ref.stats(np.moveaxis(vh, 2, 0), q=(33.3,))
    assert np.array_equal(out['VH__p33.3'].values, want['p33.3'], equal_nan=True)
    assert np.array_equal(out['line__mean'].values, ref.stats(vv[:, :1])['mean'][0], equal_nan=True)
    assert out['VV__argmax'].values.dtype == np.int32 and out['VV__p2'].values.dtype == np.float32
    assert temporal.TemporalStatistics(('mean', 'argmax'), (2, 97.5, 33.3)).apply(ds).equals(out)
    assert temporal.temporal_statistics(ds, ('mean', 'argmax'), q=(2, 97.5, 33.3)).equals(out)
    comp = temporal.composite(ds, 'median')
    assert sorted(comp.data_vars) == ['VH', 'VV', 'dem', 'line'] and comp['VH'].dims == ('y', 'x')
    assert np.array_equal(comp['VV'].values, ref.stats(vv)['median'], equal_nan=True)
    p = temporal.composite(ds['VV'], 97.5, skipna=False)
    assert isinstance(p, xr_lite.DataArray) and p.name == 'VV' and p.dims == ('y', 'x')
    assert np.array_equal(p.values, ref.stats(vv, skipna=False, q=(97.5,))['p97.5'], equal_nan=True)
    one = temporal.temporal_stats(ds['VV'], 'cv', ddof=1)
    assert list(one.data_vars) == ['VV__cv']
    assert np.array_equal(one['VV__cv'].values, ref.stats(vv, ddof=1)['cv'], equal_nan=True)


def test_the_accessor_methods_forward_to_the_module(on_the_restatement):
    """xarray is not installed where the suite runs: the two new accessor methods are built the way register() builds
    them and called on an object that stands in for the accessor"""
    from nd_amd import _xarray, xr_lite
    temporal = on_the_restatement
    rng = np.random.default_rng(20261028)
    vv = cases.speckle(rng, (9, 4, 5), 'float32')
    ds = xr_lite.Dataset(coords={'time': np.arange(9)})
    ds['VV'] = (('time', 'y', 'x'), vv)

    class Accessor(object):
        _obj = ds
    for name, (module, function) in _xarray._METHODS.items():
        if module == 'temporal':
            setattr(Accessor, name, _xarray._forward(getattr(temporal, function)))
    out = Accessor().temporal_stats(('median',), q=2)
    assert sorted(out.data_vars) == ['VV__median', 'VV__p2'] and Accessor.temporal_stats.__doc__ == temporal.temporal_stats.__doc__
    assert np.array_equal(out['VV__median'].values, ref.stats(vv)['median'], equal_nan=True)
    assert np.array_equal(Accessor().composite('max')['VV'].values, ref.stats(vv)['max'], equal_nan=True)
