"""Statistics along time on the device against tests/temporal_ref.py: float64 outputs bit for bit (as int64 views, NaN
where the restatement has NaN), integer outputs equal, the T-typed order statistics by == with NaN at the same places;
no tolerance and no excluded pixel.  Series lengths below, at and above every padded register length and every
exported boundary, planes that are no multiple of a wave, every layout, both kernel forms where both serve a length,
NaN patterns, ties, infinities, both zeros, every request alone and together, the Python layer and the pipeline from
OmnibusTest; and cases 0 - 7 of the fuzz generator on poisoned, guard-banded scratch memory (tests/canary.py).  The
held-stream run of the same cases is tests/test_held_temporal_gpu.py."""
import warnings
from collections import OrderedDict

import numpy as np
import pytest

from tests import temporal_cases as cases
from tests import temporal_ref as ref
from tests.canary import PATTERNS, canary

pytestmark = pytest.mark.gpu
DTYPES = ('float32', 'float64')
KS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65, 100, 130)
Q3 = (2, 50, 98)
Q5 = (0, 2, 33.3, 97.5, 100)
FUZZ_SEED = 20261022            # tests/test_temporal_fuzz_gpu.py


@pytest.fixture(scope='module')
def K(device):
    from nd_amd import kernels
    return kernels


def _torch_dtype(dtype):
    import torch
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _lengths(K, dtype):
    """KS and every exported boundary with its successor, each with whether order statistics are served there"""
    t = _torch_dtype(dtype)
    ks = set(KS) | {K.TEMPORAL_REG_MAX[t], K.TEMPORAL_REG_MAX[t] + 1, K.TEMPORAL_LDS_MAX[t], K.TEMPORAL_LDS_MAX[t] + 1}
    return [(k, k <= K.TEMPORAL_LDS_MAX[t]) for k in sorted(ks)]


def _same_dicts(a, b, what):
    assert set(a) == set(b)
    for key in a:
        ref.same_bits(a[key], b[key], '%s %s' % (what, key))


# ---- series lengths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_every_series_length(K, dtype):
    rng = np.random.default_rng(1)
    for k, order in _lengths(K, dtype):
        x = cases.with_special_pixels(cases.speckle(rng, (k, 5, 7), dtype))
        stats = cases.ALL if order else tuple(s for s in cases.ALL if s not in cases.ORDER)
        q = Q3 if order else ()
        for skipna in (True, False):
            want = cases.want_stats(x, stats, q, skipna)
            for layout in ('tyx', 'yxt'):
                cases.check(K, x, stats, q, skipna, layout=layout, want=want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_above_the_lds_limit_raises(K, dtype):
    import torch
    k = K.TEMPORAL_LDS_MAX[_torch_dtype(dtype)] + 1
    x = torch.zeros((k, 2, 3), dtype=_torch_dtype(dtype), device='cuda')
    with pytest.raises(NotImplementedError, match='TEMPORAL_LDS_MAX'):
        K.temporal_stats(x, ('median',))
    with pytest.raises(NotImplementedError, match='TEMPORAL_LDS_MAX'):
        K.temporal_stats(x, ('mean',), q=(50,))
    assert float(K.temporal_stats(x, ('count',))['count'].sum()) == 6 * k        # the moments are served


# ---- planes and layouts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('plane', [(1, 1), (5, 7), (70, 150), (1, 257)], ids=lambda p: '%dx%d' % p)
def test_planes_in_every_layout(K, dtype, plane):
    """the same data give the same bits in every layout: register form (24 dates) and LDS form (100)"""
    rng = np.random.default_rng(2)
    for k in (24, 100):
        x = cases.with_special_pixels(cases.speckle(rng, (k,) + plane, dtype))
        want = cases.want_stats(x, cases.ALL, Q3)
        first = None
        for layout in cases.LAYOUTS:
            got = cases.check(K, x, cases.ALL, Q3, layout=layout, want=want)
            if first is None:
                first = got
            _same_dicts(got, first, layout)


def test_a_time_x_variable_is_one_row(K):
    import torch
    rng = np.random.default_rng(3)
    x = cases.speckle(rng, (9, 1, 257), 'float32')
    t = torch.from_numpy(x[:, 0]).cuda()                    # (time, x)
    got = K.temporal_stats(t[:, None, :], ('median', 'sum'), axis=0)
    want = cases.want_stats(x, ('median', 'sum'))
    ref.same({s: v.cpu().numpy() for s, v in got.items()}, want)


def test_an_empty_plane_returns_empty_outputs(K):
    import torch
    for shape, axis in (((5, 0, 7), 0), ((0, 7, 5), 2), ((5, 3, 0), 0)):
        got = K.temporal_stats(torch.zeros(shape, device='cuda'), ('mean', 'median', 'argmax'), q=(2,), axis=axis)
        kept = tuple(n for i, n in enumerate(shape) if i != axis)
        assert {s: tuple(v.shape) for s, v in got.items()} == {s: kept for s in ('mean', 'median', 'argmax', 'p2')}
        assert got['mean'].dtype == torch.float64 and got['argmax'].dtype == torch.int32


# ---- the forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_the_forms_give_the_same_bits(K, dtype):
    """register and LDS form wherever both serve a length, the streaming form for the moments"""
    rng = np.random.default_rng(4)
    reg = K.TEMPORAL_REG_MAX[_torch_dtype(dtype)]
    moments = tuple(s for s in cases.ALL if s not in cases.ORDER)
    for k in sorted({1, 2, 8, 9, 24, 33, reg}):
        x = cases.with_special_pixels(cases.speckle(rng, (k, 5, 70), dtype))
        for skipna in (True, False):
            want = cases.want_stats(x, cases.ALL, Q3, skipna)
            for layout in ('tyx', 'yxt', 'crop'):
                a = cases.check(K, x, cases.ALL, Q3, skipna, layout=layout, form='register', want=want)
                b = cases.check(K, x, cases.ALL, Q3, skipna, layout=layout, form='lds', want=want)
                _same_dicts(a, b, 'register against lds, k = %d' % k)
                c = cases.check(K, x, moments, (), skipna, layout=layout, form='stream',
                                want={s: want[s] for s in moments})
                _same_dicts(c, {s: a[s] for s in moments}, 'stream against register, k = %d' % k)
    with pytest.raises(Exception, match='not served'):
        cases.device_stats(K, np.zeros((reg + 1, 2, 2), dtype), ('mean',), form='register')


# ---- NaN patterns and values -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('skipna', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_nan_patterns(K, dtype, skipna):
    """per pixel: no NaN, one, k - 1, all; NaN first and NaN last"""
    rng = np.random.default_rng(5)
    for k in (1, 2, 9, 24, 65):
        x = cases.speckle(rng, (k, 1, 6), dtype, nan=0.0)
        x[rng.integers(0, k), 0, 1] = np.nan
        x[:, 0, 2] = np.nan
        x[rng.integers(0, k), 0, 2] = 0.75
        x[:, 0, 3] = np.nan
        x[0, 0, 4] = np.nan
        x[k - 1, 0, 5] = np.nan
        for layout in ('tyx', 'yxt'):
            cases.check(K, x, cases.ALL, Q5, skipna, ddof=1, layout=layout)


@pytest.mark.parametrize('dtype', DTYPES)
def test_ties_infinities_and_zeros(K, dtype):
    rng = np.random.default_rng(6)
    for k in (4, 9, 24, 70):
        x = cases.speckle(rng, (k, 1, 8), dtype, nan=0.0, ties=0.0)
        x[:, 0, 0] = 2.5                                    # all dates equal
        x[:, 0, 1] = np.where(np.arange(k) % 2, 1.0, 3.0)   # ties across the middle ranks
        x[::2, 0, 2] = np.inf
        x[1::2, 0, 3] = -np.inf
        x[0, 0, 4], x[k - 1, 0, 4] = -np.inf, np.inf
        x[:, 0, 5] = np.where(np.arange(k) % 2, 0.0, -0.0)  # both zeros, equal under ==
        x[:, 0, 6] = np.inf
        x[0, 0, 7] = np.nan
        for skipna in (True, False):
            for layout in ('tyx', 'yxt'):
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    cases.check(K, x, cases.ALL, Q5, skipna, layout=layout)


# ---- requests --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_each_statistic_alone_and_all_at_once(K, dtype):
    rng = np.random.default_rng(7)
    nine = (0, 2, 5, 25, 33.3, 50, 75, 98, 100)             # more percentiles than one launch takes
    for k in (7, 24, 100):
        x = cases.with_special_pixels(cases.speckle(rng, (k, 5, 70), dtype))
        for ddof in (0, 1):
            both = cases.check(K, x, cases.ALL, Q5, ddof=ddof)
            for s in cases.ALL:
                alone = cases.device_stats(K, x, (s,), ddof=ddof)
                assert list(alone) == [s]
                ref.same_bits(alone[s], both[s], s)
            for p in Q5:
                alone = cases.device_stats(K, x, (), (p,))
                ref.same_bits(alone[ref.name(p)], both[ref.name(p)], ref.name(p))
        many = cases.check(K, x, ('median',), nine, layout='yxt')
        assert list(many) == ['median'] + [ref.name(p) for p in nine]


# ---- the Python layer ------------------------------------------------------------------------------------------------
def _dataset(rng, device_data=False, dims=('time', 'y', 'x'), sizes=(9, 6, 11)):
    import torch
    from nd_amd import xr_lite
    coords = OrderedDict((d, np.arange(n) * 1.5) for d, n in zip(dims, sizes))
    ds = xr_lite.Dataset(coords=coords, attrs={'sensor': 'S1'})
    vv = cases.speckle(rng, sizes, 'float32')
    vh = cases.speckle(rng, sizes, 'float64')
    order = ('y', 'x', 'time')
    vh_yxt = np.ascontiguousarray(vh.transpose([dims.index(d) for d in order]))
    dem = rng.random((sizes[dims.index('y')], sizes[dims.index('x')]))
    up = (lambda a: torch.from_numpy(a).cuda()) if device_data else (lambda a: a)
    ds['VV'] = (dims, up(vv), {'units': 'linear'})
    ds['VH'] = (order, up(vh_yxt))
    ds['dem'] = (('y', 'x'), up(dem))
    return ds, vv, np.moveaxis(vh_yxt, 2, 0), dem


def _host(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


@pytest.mark.parametrize('device_data', [False, True], ids=['host', 'device'])
def test_python_layer(device, device_data):
    import torch
    from nd_amd import temporal, xr_lite
    from nd_amd.visualize import to_rgb
    rng = np.random.default_rng(8)
    ds, vv, vh, dem = _dataset(rng, device_data)
    out = temporal.temporal_stats(ds, ('mean', 'cv', 'argmax', 'median'), q=(2, 97.5), ddof=1)
    keys = ('mean', 'cv', 'argmax', 'median', 'p2', 'p97.5')
    assert sorted(out.data_vars) == sorted(['dem'] + ['%s__%s' % (v, s) for v in ('VV', 'VH') for s in keys])
    assert out.attrs == ds.attrs and 'time' not in out.coords and list(out.coords) == ['y', 'x']
    assert out['VV__mean'].attrs == {'units': 'linear'}
    for name, x in (('VV', vv), ('VH', vh)):
        want = ref.stats(x, 0, True, 1, (2, 97.5))
        for s in keys:
            da = out['%s__%s' % (name, s)]
            assert da.dims == ('y', 'x') and torch.is_tensor(da.values) == device_data
            ref.same({s: _host(da.values)}, {s: want[s]}, name)
    assert out['VV__median'].values.dtype in (np.float32, torch.float32)
    assert out['VH__median'].values.dtype in (np.float64, torch.float64)
    assert out['dem'].values is ds['dem'].values            # untouched
    assert temporal.TemporalStatistics(('mean', 'cv', 'argmax', 'median'), (2, 97.5), ddof=1).apply(ds).equals(out)
    assert temporal.temporal_statistics(ds, ('mean', 'cv', 'argmax', 'median'), q=(2, 97.5), ddof=1).equals(out)
    comp = temporal.composite(ds, 'median')
    assert sorted(comp.data_vars) == ['VH', 'VV', 'dem'] and comp['VV'].dims == ('y', 'x')
    ref.same({'median': _host(comp['VV'].values)}, {'median': ref.stats(vv)['median']})
    p90 = temporal.composite(ds['VV'], 90)
    assert isinstance(p90, xr_lite.DataArray) and p90.name == 'VV' and p90.dims == ('y', 'x')
    ref.same({'p90': _host(p90.values)}, {'p90': ref.stats(vv, q=(90,))['p90']})
    rgb = to_rgb([comp['VV'], comp['VV'], comp['VV']])
    assert tuple(rgb.shape) == (6, 11, 3)
    line = xr_lite.Dataset(coords={'x': np.arange(66)})
    line['a'] = (('time', 'x'), (lambda a: torch.from_numpy(a).cuda() if device_data else a)(vv.reshape(9, -1)[:, :66]))
    got = temporal.temporal_stats(line, 'sum')
    assert got['a__sum'].dims == ('x',)
    ref.same({'sum': _host(got['a__sum'].values)}, {'sum': ref.stats(vv.reshape(9, 1, -1)[:, :, :66])['sum'][0]})


def test_the_xarray_accessor(device):
    xr = pytest.importorskip('xarray')
    from nd_amd import _xarray
    assert _xarray.register()
    rng = np.random.default_rng(9)
    x = cases.speckle(rng, (9, 6, 11), 'float32')
    ds = xr.Dataset({'VV': (('time', 'y', 'x'), x)}, coords={'time': np.arange(9), 'y': np.arange(6), 'x': np.arange(11)})
    out = ds.nd_amd.temporal_stats(('median',), q=2)
    assert out['VV__median'].dims == ('y', 'x') and 'VV__p2' in out
    ref.same({'median': out['VV__median'].values}, {'median': ref.stats(x)['median']})
    assert ds.nd_amd.composite('max')['VV'].dims == ('y', 'x')


def test_integer_and_bool_inputs(device):
    from nd_amd import temporal, xr_lite
    rng = np.random.default_rng(10)
    change = rng.random((24, 7, 9)) < 0.2
    counts = rng.integers(-300, 300, size=(7, 9, 24)).astype(np.int16)
    ds = xr_lite.Dataset()
    ds['change'] = (('time', 'y', 'x'), change)
    ds['dn'] = (('y', 'x', 'time'), counts)
    out = temporal.temporal_stats(ds, ('sum', 'max', 'median', 'argmin'))
    assert out['change__sum'].values.dtype == np.float64 and out['dn__max'].values.dtype == np.float64
    assert np.array_equal(out['change__sum'].values, change.sum(0))
    for name, x in (('change', change), ('dn', np.moveaxis(counts, 2, 0))):
        want = ref.stats(x)
        for s in ('sum', 'max', 'median', 'argmin'):
            ref.same({s: out['%s__%s' % (name, s)].values}, {s: want[s]}, name)


def test_from_the_omnibus_test_to_a_change_count(device):
    from tests import synth
    from nd_amd import temporal, xr_lite
    from nd_amd.change import OmnibusTest
    c11, c12re, c12im, c22 = synth.omnibus_stack(11, 24, 70, 150, change_frac=0.2)
    ds = xr_lite.Dataset()
    for name, a in (('C11', c11), ('C12__re', c12re), ('C12__im', c12im), ('C22', c22)):
        ds[name] = (('time', 'y', 'x'), a)
    change = OmnibusTest(n=9, alpha=0.01).apply(ds)
    count = temporal.temporal_stats(change, 'sum')['change__sum']
    assert count.dims == tuple(d for d in change.dims if d != 'time') and count.shape == (70, 150)
    want = np.asarray(change.values).sum(change.dims.index('time'))
    assert np.array_equal(count.values, want) and want.max() >= 1


# ---- poisoned scratch memory -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', PATTERNS, ids=['0x%02X' % p for p in PATTERNS])
def test_fuzz_cases_on_poisoned_memory(K, pattern):
    """every output of kernels.temporal_stats is the wrapper's own uninitialised memory: cases 0 - 7 of the fuzz
    generator with it filled with `pattern` and guard-banded, against the restatement"""
    fails = []
    with canary(pattern) as c:
        for i in range(8):
            why = None
            try:
                cases.run_case(K, cases.random_case(np.random.default_rng([FUZZ_SEED, i]), K))
            except AssertionError as e:
                why = str(e) or 'assertion'
            try:
                c.check()
            except AssertionError as e:
                why = '%s%s' % (why + '; ' if why else '', e)
            if why:
                fails.append((i, why))
        seen = c.wrapped
    assert seen > 0, 'the canary saw no allocation: the test checks nothing'
    assert not fails, '%d of 8 cases fail on memory filled with 0x%02X: %s' % (len(fails), pattern, fails[:3])
