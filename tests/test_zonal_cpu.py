"""Statistics of zones without a GPU: the restatement (tests/zonal_ref.py) held to things outside it -- scipy.ndimage,
math.fsum and exact rational arithmetic with error bounds that follow from the number format --, hand-enumerated cases
of the definition, zone-locality, the header, the entries' argument checks and the host logic of nd_amd.zonal (run
on the restatement in place of the kernels)."""
import contextlib
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import zonal_cases as cases
from tests import zonal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


# ---- the restatement against scipy, fsum and exact arithmetic -------------------------------------------------------
def bound_plane():
    """one 300 x 257 plane: zones of 1, 63, 64, 65, 4096 and 4097 pixels, 392 random small ones and one of 51 400"""
    rng = np.random.default_rng(20261021)
    lab = np.zeros((300, 257), np.int32)
    lab[:200, :] = 1                                                            # 51 400
    flat = lab.reshape(-1)
    at = 200 * 257
    for z, m in enumerate((1, 63, 64, 65, 4096, 4097)):
        flat[at:at + m] = 2 + z
        at += m
    rest = flat[at:]
    rest[:] = rng.integers(8, 400, size=rest.size)
    return rng, lab, np.arange(1, 400)


def exact_sums(c):
    """-> (sum, sum of |c|, m2) of the float64 values c as Fractions, through integers scaled by a power of two"""
    scale = 1 << 1100
    ints = [int(Fraction(float(v)) * scale) for v in c]
    s, q = sum(ints), sum(i * i for i in ints)
    m = len(ints)
    return (Fraction(s, scale), Fraction(sum(abs(i) for i in ints), scale), Fraction(m * q - s * s, m * scale * scale))


@pytest.fixture(scope='module', params=['float32', 'float64'])
def bound_case(request):
    rng, lab, ids = bound_plane()
    x = cases.speckle(rng, lab.shape, request.param, 0.01)
    st, got_ids = ref.zonal_stats(x[None], lab, ids)
    assert np.array_equal(got_ids, ids)
    zones = []
    for z, i in enumerate(ids):
        c = x[lab == i].astype(np.float64)
        zones.append(c[~np.isnan(c)])
    return x, lab, ids, {k: v[0] for k, v in st.items()}, zones


def test_counts_min_max_equal_scipy(bound_case):
    import scipy.ndimage as ndi
    x, lab, ids, st, zones = bound_case
    valid = ~np.isnan(x)
    assert np.array_equal(st['count'], ndi.sum_labels(valid, lab, ids).astype(np.int64))
    assert np.array_equal(st['nan_count'], ndi.sum_labels(~valid, lab, ids).astype(np.int64))
    assert st['nan_count'].sum() > 0
    for z, c in enumerate(zones):                       # with NaNs: the same on each zone's non-NaN values
        assert st['count'][z] == len(c)
        if len(c):
            assert st['min'][z] == c.min() and st['max'][z] == c.max()
        else:
            assert np.isnan(st['min'][z]) and np.isnan(st['max'][z]) and st['sum'][z] == 0.0
    clean = np.where(valid, x, 1.0).astype(np.float64)  # NaN-free data: scipy's minimum / maximum directly
    st2 = ref.zonal_stats(clean[None], lab, ids)[0]
    assert np.array_equal(st2['min'][0], ndi.minimum(clean, lab, ids))
    assert np.array_equal(st2['max'][0], ndi.maximum(clean, lab, ids))
    assert np.array_equal(st2['count'][0], ndi.sum_labels(np.ones(lab.shape), lab, ids).astype(np.int64))
    assert (st2['nan_count'] == 0).all()


def test_sum_and_m2_within_the_bounds_and_so_is_scipy(bound_case):
    """|sum - exact| <= m 2^-52 sum|c| (the first-order bound for any order of m terms is (m - 1) 2^-53 sum|c|; the
    factor of two absorbs the second-order term and fsum's own rounding) and |m2 - exact| <= 2 [(m + 3) 2^-53 exact +
    m ((m + 1) 2^-53 sum|c| / m)^2] (per-term roundings and summation, plus the quadratic effect of the mean's error).
    scipy.ndimage.mean / variance sit inside the same bounds, so both sides do."""
    import scipy.ndimage as ndi
    x, lab, ids, st, zones = bound_case
    filled = np.where(np.isnan(x), 0.0, x).astype(np.float64)
    checked = 0
    for z, c in enumerate(zones):
        m = len(c)
        if m == 0:
            continue
        fs, fa = math.fsum(c), math.fsum(np.abs(c))
        sbound = m * 2.0 ** -52 * fa
        assert abs(st['sum'][z] - fs) <= sbound, (z, m)
        if m > 70000:
            continue
        es, ea, em2 = exact_sums(c)
        assert abs(Fraction(st['sum'][z]) - es) <= Fraction(sbound)
        b2 = 2 * ((m + 3) * Fraction(U) * em2 + m * ((m + 1) * Fraction(U) * ea / m) ** 2)
        assert abs(Fraction(st['m2'][z]) - em2) <= b2, (z, m, float(b2))
        assert abs(Fraction(st['sum'][z] / st['count'][z]) - es / m) <= Fraction(sbound) / m
        # scipy on the same values
        mask = (lab == ids[z]) & ~np.isnan(x)
        sm, sv = float(ndi.mean(filled, mask, 1)), float(ndi.variance(filled, mask, 1))
        assert abs(Fraction(sm) - es / m) <= Fraction(sbound) / m, (z, m)
        assert abs(Fraction(sv) - em2 / m) <= b2 / m, (z, m)
        checked += 1
    assert checked > 390
    sizes = sorted(len(c) for c in zones)
    assert sizes[-1] > 50000 and {1, 4096, 4097} <= {int((lab == i).sum()) for i in ids[1:7]}


# ---- hand-enumerated cases ------------------------------------------------------------------------------------------
def test_which_pixels_belong_to_a_zone():
    lab = np.array([[0, 1, 2, -1], [3, 4, 2, 1]], np.int32)
    k, n, ids = ref.keys(lab, None, 3)
    assert n == 3 and list(ids) == [1, 2, 3]
    assert np.array_equal(k, [[3, 0, 1, 3], [2, 3, 1, 0]])       # 0, negative and above n: nowhere
    assert ref.default_n(lab) == 4 and ref.default_n(np.zeros((2, 2), np.int32)) == 0
    assert ref.default_n(np.array([[-3, -1]], np.int64)) == 0
    f = np.array([[2.0, 2.5, np.nan, 1.0, np.inf, -0.0]], np.float64)
    k, n, _ = ref.keys(f)
    assert n == 2 and list(k[0]) == [1, 2, 2, 0, 2, 2]           # 2.0 is zone 2; 2.5, NaN, inf and 0 are nowhere
    b = np.array([[True, False, True]])
    k, n, _ = ref.keys(b)
    assert n == 1 and list(k[0]) == [0, 1, 0]
    perm, offsets = ref.index(np.array([[2, 0, 1], [0, 2, 0]], np.int32), 2)
    assert list(perm) == [1, 3, 5, 2, 0, 4] and list(offsets) == [0, 3, 4]


def test_sparse_int64_ids_compared_as_int64():
    ids = np.array([3, 100234, 2 ** 40 + 1, 2 ** 53, 2 ** 53 + 1], np.int64)
    lab = np.array([[3, 100234, 2 ** 40 + 1, 2 ** 40, 2 ** 53 + 1, 2 ** 53, 0, 4]], np.int64)
    k, n, _ = ref.keys(lab, ids)
    assert n == 5 and list(k[0]) == [0, 1, 2, 5, 4, 3, 5, 5]
    x = np.arange(8, dtype=np.float64)[None, None]
    st, _ = ref.zonal_stats(x, lab, ids)
    assert list(st['sum'][0]) == [0.0, 1.0, 2.0, 5.0, 4.0] and list(st['count'][0]) == [1] * 5
    # a float64 label cannot tell 2^53 + 1 from 2^53: it is the int64 it equals
    k, n, _ = ref.keys(lab.astype(np.float64), ids)
    assert list(k[0]) == [0, 1, 2, 5, 3, 3, 5, 5]


def test_absent_all_nan_and_infinite_zones():
    lab = np.array([[1, 1, 3, 3, 4, 4, 4]], np.int32)
    x = np.array([[[1.0, 2.0, np.nan, np.nan, np.inf, 1.0, -0.0]]], np.float32)
    st, ids = ref.zonal_stats(x, lab)
    assert list(ids) == [1, 2, 3, 4]
    assert list(st['count'][0]) == [2, 0, 0, 3] and list(st['nan_count'][0]) == [0, 0, 2, 0]
    assert list(st['sum'][0]) == [3.0, 0.0, 0.0, np.inf]
    mean = ref.mean(st)[0]
    assert mean[0] == 1.5 and np.isnan(mean[1]) and np.isnan(mean[2]) and mean[3] == np.inf
    for z in (1, 2):                                             # absent, and all NaN
        assert np.isnan(st['min'][0, z]) and np.isnan(st['max'][0, z]) and st['m2'][0, z] == 0.0
    assert st['min'][0, 3] == 0.0 and st['max'][0, 3] == np.inf and np.isnan(st['m2'][0, 3])
    assert st['m2'][0, 0] == 0.5
    assert np.isnan(ref.var(st)[0, 1]) and ref.var(st)[0, 0] == 0.25 and ref.std(st, 1)[0, 0] == math.sqrt(0.5)
    one = ref.zonal_stats(np.array([[[7.0]]]), np.array([[1]]))[0]
    with np.errstate(all='ignore'):
        assert not np.isfinite(ref.var(one, 1)[0, 0]) and not np.isfinite(ref.std(one, 1)[0, 0])   # ddof = count
    assert ref.var(one, 0)[0, 0] == 0.0
    # an absent operand is left out, not added as 0.0
    st = ref.zonal_stats(np.array([[[-0.0, np.nan]]]), np.array([[1, 1]]))[0]
    assert np.signbit(st['sum'][0, 0]) and st['count'][0, 0] == 1


def test_the_tree_is_the_one_written_down():
    """against a scalar walk of the definition, NaN positions skipped where they stand"""
    def chunk(v):
        a = list(v) + [None] * (64 - len(v))
        while len(a) > 1:
            a = [x if y is None else (y if x is None else x + y) for x, y in zip(a[0::2], a[1::2])]
        return a[0]

    def chain(parts):
        acc = None
        for p in parts:
            acc = p if acc is None else (acc if p is None else acc + p)
        return acc

    rng = np.random.default_rng(5)
    for m in (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 9000):
        c = rng.gamma(4.0, 0.25, size=m) * 10.0 ** rng.integers(-3, 4, size=m)
        part = rng.random(m) > 0.1
        vals = [float(v) if p else None for v, p in zip(c, part)]
        chunks = [chunk(vals[i:i + 64]) for i in range(0, m, 64)]
        want = chain([chain(chunks[i:i + 64]) for i in range(0, len(chunks), 64)])
        pad = -m % 64
        got, has = ref.tree(np.concatenate([c, np.zeros(pad)]), np.concatenate([part, np.zeros(pad, bool)]))
        assert bool(has) == (want is not None)
        if want is not None:
            assert float(got) == want and m > 0
        x = np.where(part, c, np.nan)[None, None]
        st = ref.zonal_stats(x, np.ones((1, m), np.int32))[0]
        assert st['sum'][0, 0] == (want or 0.0) and st['count'][0, 0] == part.sum()


def test_zone_locality():
    """relabelling or merging OTHER zones leaves a zone's six statistics bit-identical"""
    rng = np.random.default_rng(6)
    lab = cases.sized_zones(rng, (70, 150), (5000, 700, 64, 9, 1, 3000))
    x = cases.speckle(rng, (2, 70, 150), 'float32')
    base = ref.zonal_stats(x, lab)[0]
    other = lab.copy()
    other[lab == 1] = 9                     # relabelled
    other[lab == 3] = 4                     # merged into another
    other[lab == 5] = 0                     # removed
    st, ids = ref.zonal_stats(x, other)
    for z in (2, 6):
        for name in ref.STATS:
            cases.rcases.assert_same(st[name][:, z - 1], base[name][:, z - 1])
    for name in ref.STATS:
        cases.rcases.assert_same(st[name][:, 8], base[name][:, 0])
    assert st['count'][0, 3] == base['count'][0, 2] + base['count'][0, 3]


def test_paint_restated():
    lab = np.array([[1, 0, 2], [2, 5, 1]], np.int32)
    k, n, _ = ref.keys(lab, None, 2)
    table = np.array([[10.0, 20.5]])
    src = np.array([[[1, 2, 3], [4, 5, 6]]], np.float32)
    got = ref.paint(table, k, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got[0], [[10, np.nan, 20.5], [20.5, np.nan, 10]], equal_nan=True)
    assert np.array_equal(ref.paint(table, k, np.float32, fill=-1)[0], [[10, -1, 20.5], [20.5, -1, 10]])
    assert np.array_equal(ref.paint(table, k, np.float32, src)[0], [[10, 2, 20.5], [20.5, 5, 10]])
    # the round trip paint(mean) -> stats gives the mean back
    rng = np.random.default_rng(7)
    lab = cases.sized_zones(rng, (40, 50), (700, 64, 9, 1))
    x = cases.speckle(rng, (1, 40, 50), 'float64', 0.0)
    st = ref.zonal_stats(x, lab)[0]
    k = ref.keys(lab)[0]
    again = ref.zonal_stats(ref.paint(ref.mean(st), k, np.float64), lab)[0]
    assert np.array_equal(again['min'], ref.mean(st)) and np.array_equal(again['max'], ref.mean(st))
    assert np.allclose(ref.mean(again), ref.mean(st), rtol=1e-14, atol=0)


# ---- the header and the entries -------------------------------------------------------------------------------------
ENTRIES = ('nd_amd_zonal_keys', 'nd_amd_zonal_workspace_bytes', 'nd_amd_zonal_stats', 'nd_amd_zonal_paint')


def test_header_declares_the_entries():
    from nd_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert 'Statistics of zones' in hdr and 'a (+) absent = a' in hdr
    assert _lib.KERNEL_NAMES[31] == 'zonal' and re.search(r'#define\s+ND_AMD_KERNEL_ZONAL\s+31\b', hdr)
    src = open(os.path.join(ROOT, 'nd_amd', 'csrc', 'zonal.hip')).read()
    assert not re.search(r'atomicAdd|unsafeAtomicAdd|atomic_fadd|getenv|env_int|env_double', src)


def _keys(L, dtype=4, ny=8, nx=8, n=3, ptr=None, strides=(8, 1)):
    from nd_amd import _lib
    return L.nd_amd_zonal_keys(ptr, dtype, ny, nx, _lib.i64_array(strides), None, n, ptr, None)


def _stats(L, dtype=0, nplanes=1, ny=8, nx=8, n=3, ptr=None, strides=(64, 8, 1), out=None):
    from nd_amd import _lib
    return L.nd_amd_zonal_stats(ptr, dtype, nplanes, ny, nx, _lib.i64_array(strides), ptr, ptr, n, out, None, out,
                                None, None, None, None, 0, None)


def _paint(L, dtype=0, nplanes=1, ny=8, nx=8, n=3, ptr=None, strides=(64, 8, 1)):
    from nd_amd import _lib
    return L.nd_amd_zonal_paint(ptr, ptr, nplanes, ny, nx, n, None, None, ptr, _lib.i64_array(strides), dtype, 0.0,
                                None)


def test_argument_validation_without_gpu():
    """every refusal below comes before the first HIP call"""
    from nd_amd import _lib
    L = _lib.lib()
    dummy = ctypes.c_void_p(4096)
    for call, bad_dtype in ((_keys, 9), (_stats, 4), (_paint, 3)):
        assert call(L, dtype=bad_dtype) == _lib.EINVAL
        assert b'dtype' in L.nd_amd_last_error()
        assert call(L, ny=-1) == _lib.EINVAL
        assert call(L, n=-1) == _lib.EINVAL
        assert call(L, ny=1 << 16, nx=1 << 15) == _lib.EUNSUPPORTED          # 2^31 pixels, null pointers
        assert b'2^31' in L.nd_amd_last_error()
        assert call(L, n=2 ** 31 - 1) == _lib.EUNSUPPORTED
        assert b'zones' in L.nd_amd_last_error()
        assert call(L, ny=0) == _lib.OK and call(L, nx=0) == _lib.OK        # an empty plane: nothing done
        assert call(L) == _lib.EINVAL                                        # null pointers
        assert b'null' in L.nd_amd_last_error()
    assert _keys(L, ptr=dummy, strides=(-8, 1)) == _lib.EINVAL
    assert _stats(L, ptr=dummy, strides=(64, -8, 1)) == _lib.EINVAL
    assert _paint(L, ptr=dummy, strides=(64, 8, -1)) == _lib.EINVAL
    assert b'negative stride' in L.nd_amd_last_error()
    assert _stats(L, nplanes=-1) == _lib.EINVAL and _paint(L, nplanes=-1) == _lib.EINVAL
    assert _stats(L, nplanes=0) == _lib.OK and _paint(L, nplanes=0) == _lib.OK
    assert _stats(L, n=0) == _lib.OK                                         # no zone: nothing done
    assert _stats(L, ptr=dummy) == _lib.OK                                   # no output asked for: nothing done
    assert _stats(L, ptr=dummy, out=dummy) == _lib.EWORKSPACE                # never dereferenced
    assert L.nd_amd_zonal_workspace_bytes(1, 1 << 16, 1 << 15, 3) == 0
    assert L.nd_amd_zonal_workspace_bytes(1, 100, 100, 0) == 0
    small = L.nd_amd_zonal_workspace_bytes(1, 100, 100, 10)
    assert 0 < small < 8192
    # 40 bytes per plane and 2048 pixels, 16 per plane and zone
    big = L.nd_amd_zonal_workspace_bytes(24, 4096, 4096, 374208)
    want = 24 * (4096 * 4096 // 2048 * 40 + 374208 * 16)
    assert want <= big < want + 8 * 256


def test_python_errors_without_gpu():
    import torch
    from nd_amd import kernels as K
    from nd_amd import xr_lite, zonal
    with pytest.raises(ValueError, match='ROCm device'):
        K.zonal_index(torch.zeros((4, 5), dtype=torch.int32))
    for bad in ([3, 3], [5, 2], [1.0, 2.0], [[1, 2]], ['a']):
        with pytest.raises(ValueError, match='ids'):
            K.zonal_ids(bad)
    assert K.zonal_ids([3, 100234, 2 ** 40 + 1]).dtype == np.int64 and len(K.zonal_ids([])) == 0
    ds = xr_lite.Dataset(coords={'y': np.arange(4), 'x': np.arange(5)})
    ds['a'] = (('y', 'x'), np.zeros((4, 5), np.float32))
    zones = np.ones((4, 5), np.int32)
    with pytest.raises(ValueError, match='zones have'):
        zonal.zonal_stats(ds, np.ones((4, 6), np.int32))
    with pytest.raises(ValueError, match='zones have'):
        zonal.zonal_paint(ds, xr_lite.DataArray(np.ones((5, 4), np.int32), ('y', 'x')))
    with pytest.raises(ValueError, match='increasing'):
        zonal.zonal_stats(ds, zones, ids=[2, 1])
    with pytest.raises(ValueError, match='integers'):
        zonal.ZonalStatistics(zones, ids=[1.5, 2.5])
    with pytest.raises(ValueError, match='stats'):
        zonal.zonal_stats(ds, zones, stats=('median',))
    with pytest.raises(ValueError, match='ddof'):
        zonal.zonal_stats(ds, zones, ddof=-1)
    with pytest.raises(ValueError, match='y and x'):
        zonal.zonal_stats(ds, xr_lite.DataArray(zones, ('time', 'x')))
    cplx = xr_lite.Dataset()
    cplx['c'] = (('y', 'x'), np.zeros((4, 5), np.complex64))
    with pytest.raises(TypeError, match='complex'):
        zonal.zonal_stats(cplx, zones)
    with pytest.raises(TypeError, match='complex'):
        zonal.zonal_paint(cplx, zones)
    from nd_amd import _xarray
    assert _xarray._METHODS['zonal_stats'] == ('zonal', 'zonal_stats')
    assert _xarray._METHODS['zonal_paint'] == ('zonal', 'zonal_paint')


# ---- nd_amd.zonal's host logic, with the restatement standing in for the kernels -----------------------------------
@pytest.fixture
def on_the_restatement(monkeypatch):
    import torch
    from nd_amd import kernels as K
    from nd_amd import zonal

    def planes(t, dims):
        a = t.numpy()
        rest = [i for i, d in enumerate(dims) if d not in ('y', 'x')]
        a = np.transpose(a, rest + [dims.index('y'), dims.index('x')])
        return a, a.shape[:-2]

    def index(labels, ids=None, dims=None, n=None):
        dims = ('y', 'x') if dims is None else tuple(dims)
        lab = planes(labels, dims)[0]
        k, n, ids = ref.keys(lab, ids, n)
        perm, offsets = ref.index(k, n)
        return K.ZonalIndex(torch.from_numpy(k), torch.from_numpy(perm), torch.from_numpy(offsets), n, ids)

    def stats(values, index, dims=None, stats=()):
        a, lead = planes(values, tuple(dims))
        st = ref.stats(a.reshape((-1,) + a.shape[-2:]), index.perm.numpy(), index.offsets.numpy(), index.n)
        st['mean'] = ref.mean(st)
        return {s: torch.from_numpy(np.ascontiguousarray(st[s].reshape(lead + (index.n,)))) for s in stats}

    def paint(table, index, like=None, out=None, keep=False, fill=None, dims=None):
        dims = tuple(dims)
        a, lead = planes(like, dims)
        flat = a.reshape((-1,) + a.shape[-2:])
        got = ref.paint(table.numpy().reshape(-1, index.n), index.keys.numpy(), flat.dtype, flat if keep else None,
                        np.nan if fill is None else fill).reshape(a.shape)
        rest = [d for d in dims if d not in ('y', 'x')] + ['y', 'x']
        res = torch.from_numpy(np.ascontiguousarray(np.transpose(got, [rest.index(d) for d in dims])))
        if out is None:
            return res
        out.copy_(res)
        return out

    monkeypatch.setattr(K, 'zonal_index', index)
    monkeypatch.setattr(K, 'zonal_stats', stats)
    monkeypatch.setattr(K, 'zonal_paint', paint)
    monkeypatch.setattr(K, '_zonal_default_n', lambda lab: ref.default_n(lab.numpy()))
    monkeypatch.setattr(zonal._device, 'device_of', lambda *a, **k: torch.device('cpu'))
    monkeypatch.setattr(zonal, '_on', lambda dev: contextlib.nullcontext())
    return zonal


def _dataset(rng, k=3, ny=20, nx=30):
    from nd_amd import xr_lite
    coords = {'time': np.arange(k) * 10, 'y': 5.0 - np.arange(ny), 'x': 2.0 + np.arange(nx)}
    ds = xr_lite.Dataset(coords=coords, attrs={'crs': 'none'})
    ds['vv'] = (('time', 'y', 'x'), cases.speckle(rng, (k, ny, nx), 'float32'))
    ds['vh'] = (('y', 'x', 'time'), cases.speckle(rng, (ny, nx, k), 'float64'))
    ds['dem'] = (('y', 'x'), rng.integers(0, 900, size=(ny, nx)).astype(np.int32))
    ds['dates'] = (('time',), np.arange(k))
    return ds, coords


def test_names_dims_and_coords_of_the_result(on_the_restatement):
    zonal = on_the_restatement
    rng = np.random.default_rng(8)
    ds, coords = _dataset(rng)
    lab = cases.sized_zones(rng, (20, 30), (100, 64, 9, 1))
    ids = [2, 3, 4, 9]
    out = zonal.zonal_stats(ds, lab, ids=ids, ddof=1)
    assert list(out.data_vars) == ['%s__%s' % (v, s) for v in ('vv', 'vh', 'dem')
                                   for s in ('count', 'mean', 'std', 'min', 'max')]
    assert out['vv__mean'].dims == ('zone', 'time') and out['vh__mean'].dims == ('zone', 'time')
    assert out['dem__mean'].dims == ('zone',) and out['vv__mean'].shape == (4, 3)
    assert np.array_equal(out.coords['zone'], ids) and np.array_equal(out.coords['time'], coords['time'])
    assert 'y' not in out.coords and out.attrs['crs'] == 'none'
    assert isinstance(out['vv__count'].values, np.ndarray) and out['vv__count'].values.dtype == np.int64
    want = ref.zonal_stats(ds['vv'].values, lab, ids)[0]
    ref.same(out['vv__mean'].values, ref.mean(want).T.copy())
    ref.same(out['vv__std'].values, ref.std(want, 1).T.copy())
    ref.same(out['vv__count'].values, want['count'].T.copy())
    want = ref.zonal_stats(np.moveaxis(ds['vh'].values, -1, 0), lab, ids)[0]
    ref.same(out['vh__std'].values, ref.std(want, 1).T.copy())
    want = ref.zonal_stats(ds['dem'].values[None], lab, ids)[0]
    ref.same(out['dem__mean'].values, ref.mean(want)[0])
    assert np.isnan(out['dem__mean'].values[3]) and out['dem__count'].values[3] == 0     # id 9: an absent zone
    assert not np.isfinite(out['dem__std'].values[2])                                    # ddof = 1 with count = 1
    same = zonal.zonal_statistics(ds, lab, ids=ids, ddof=1)
    assert same.equals(out) and zonal.ZonalStatistics(lab, ids=ids, ddof=1).apply(ds).equals(out)
    one = zonal.zonal_stats(ds['vv'], lab, stats=('sum',))
    assert list(one.data_vars) == ['vv__sum'] and list(one.coords['zone']) == [1, 2, 3, 4]


def test_zones_over_time(on_the_restatement):
    from nd_amd import xr_lite
    zonal = on_the_restatement
    rng = np.random.default_rng(9)
    ds, coords = _dataset(rng)
    labs = np.stack([cases.sized_zones(rng, (20, 30), sizes) for sizes in ((50, 5), (7, 8, 9, 300), (600,))])
    zones = xr_lite.DataArray(labs, ('time', 'y', 'x'))
    out = zonal.zonal_stats(ds[['vv', 'vh']], zones, stats=('count', 'sum'))
    assert list(out.coords['zone']) == [1, 2, 3, 4] and out['vv__sum'].dims == ('zone', 'time')
    for t in range(3):
        want = ref.zonal_stats(ds['vv'].values[t:t + 1], labs[t], [1, 2, 3, 4])[0]
        ref.same(out['vv__sum'].values[:, t], want['sum'][0])
        want = ref.zonal_stats(ds['vh'].values[None, :, :, t], labs[t], [1, 2, 3, 4])[0]
        ref.same(out['vh__count'].values[:, t], want['count'][0])
    assert list(out['vv__count'].values[:, 2]) == [out['vv__count'].values[0, 2], 0, 0, 0]    # absent zones: count 0
    with pytest.raises(ValueError, match='does not share'):
        zonal.zonal_stats(ds[['dem']], zones)
    painted = zonal.zonal_paint(ds[['vv', 'dates']], zones, 'max', fill=-1.0)
    assert painted['dates'].values is ds['dates'].values and painted['vv'].dims == ('time', 'y', 'x')
    for t in range(3):
        st = ref.zonal_stats(ds['vv'].values[t:t + 1], labs[t], [1, 2, 3, 4])[0]
        ref.same(painted['vv'].values[t], ref.paint(st['max'], ref.keys(labs[t], None, 4)[0], np.float32, fill=-1.0)[0])


def test_paint_keeps_the_variable_s_form_and_round_trips(on_the_restatement):
    zonal = on_the_restatement
    rng = np.random.default_rng(10)
    ds, coords = _dataset(rng)
    lab = cases.sized_zones(rng, (20, 30), (100, 64, 9, 1))
    out = zonal.zonal_paint(ds, lab, 'mean', keep=True)
    assert list(out.data_vars) == list(ds.data_vars) and out.attrs == ds.attrs
    assert out['vh'].dims == ('y', 'x', 'time') and out['vh'].values.dtype == np.float64
    assert out['vv'].values.dtype == np.float32 and out['dem'].values.dtype == np.float64
    assert np.array_equal(out['vv'].values[:, lab == 0], ds['vv'].values[:, lab == 0], equal_nan=True)
    filled = zonal.zonal_paint(ds['vv'], lab, 'mean')
    assert np.isnan(filled.values[:, lab == 0]).all() and filled.name == 'vv'
    # paint(mean) -> stats gives the mean back: every pixel of a zone holds one value
    first = zonal.zonal_stats(ds[['vh']], lab, stats=('mean',))
    again = zonal.zonal_stats(zonal.zonal_paint(ds[['vh']], lab, 'mean'), lab, stats=('min', 'max', 'mean'))
    ref.same(again['vh__min'].values, first['vh__mean'].values)
    ref.same(again['vh__max'].values, first['vh__mean'].values)
    assert np.allclose(again['vh__mean'].values, first['vh__mean'].values, rtol=1e-14, atol=0)
