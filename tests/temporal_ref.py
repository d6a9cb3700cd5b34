"""The definition of nd_amd's statistics along time (include/nd_amd.h, "Statistics along time"), restated in numpy:
vectorised over the pixels, a loop over the dates, every operation in the type and the order the header names.  The
device is held to this bit for bit (tests/test_temporal_gpu.py); tests/test_temporal_cpu.py holds this to numpy 2.2.6's
nanpercentile / nanmedian / nanmin / nanargmin and to exact arithmetic.

stats(x, axis, skipna, ddof, q) -> {name: (ny, nx) array}: count, nan_count, argmin, argmax int32; sum, mean, m2, var,
std, cv float64; min, max, median and the percentiles ('p%g' % p) of the type computed in (float32 and float64 as they
are, every other type as float64)."""
import numpy as np

STATS = ('count', 'nan_count', 'sum', 'mean', 'min', 'max', 'argmin', 'argmax', 'm2', 'var', 'std', 'cv', 'median')
MOMENTS = ('sum', 'mean', 'm2', 'var', 'std', 'cv')
INTEGERS = ('count', 'nan_count', 'argmin', 'argmax')


def name(p):
    return 'p%g' % p


def computed(x):
    """the series first, in the type it is computed in"""
    x = np.asarray(x)
    return x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)


def _rank(A, r):
    return np.take_along_axis(A, r[None].astype(np.int64), 0)[0]


def percentile(A, n, bad, p):
    """A: the series sorted ascending along axis 0, NaN last; n: the valid values; bad: where the result is NaN"""
    T = A.dtype.type
    m = np.maximum(n, 1)
    q = T(p) / T(100)
    last = (m - 1).astype(T)
    vi = last * q
    top = vi >= last
    lo = np.where(top, m - 1, np.minimum(np.floor(vi).astype(np.int64), m - 1))
    hi = np.where(top, m - 1, np.minimum(lo + 1, m - 1))
    g = (vi.astype(np.float64) - lo.astype(np.float64)).astype(T)
    a, b = _rank(A, lo), _rank(A, hi)
    d = b - a
    r = np.where(g >= T(0.5), b - d * (T(1) - g), a + d * g)
    return np.where(bad, T(np.nan), r).astype(T)


def median(A, n, bad):
    T = A.dtype.type
    m = np.maximum(n, 1)
    odd = _rank(A, (m - 1) // 2)
    even = (_rank(A, np.maximum(m // 2 - 1, 0)) + _rank(A, m // 2)) / T(2)
    return np.where(bad, T(np.nan), np.where(m % 2 == 1, odd, even)).astype(T)


def stats(x, axis=0, skipna=True, ddof=0, q=()):
    x = np.moveaxis(computed(x), axis, 0)
    T = x.dtype.type
    k, shape = x.shape[0], x.shape[1:]
    nan = np.isnan(x)
    valid = ~nan if skipna else np.ones_like(nan)
    out = {}
    with np.errstate(all='ignore'):
        n = valid.sum(0).astype(np.int32)
        nans = nan.sum(0).astype(np.int32)
        s = np.zeros(shape, np.float64)
        for t in range(k):
            s = np.where(valid[t], s + x[t].astype(np.float64), s)
        mean = s / n.astype(np.float64)
        m2 = np.zeros(shape, np.float64)
        for t in range(k):
            d = x[t].astype(np.float64) - mean
            m2 = np.where(valid[t], m2 + d * d, m2)
        dof = n - np.int32(ddof)
        var = np.where(dof > 0, m2 / np.where(dof > 0, dof, 1).astype(np.float64), np.nan)
        std = np.sqrt(var)
        out.update(count=n, nan_count=nans, sum=s, mean=mean, m2=m2, var=var, std=std, cv=std / mean)

        mn, mx = np.full(shape, np.nan, T), np.full(shape, np.nan, T)
        amin, amax = np.full(shape, -1, np.int32), np.full(shape, -1, np.int32)
        first_nan = np.full(shape, -1, np.int32)
        for t in range(k):
            ok = ~nan[t]
            take = ok & ((amin < 0) | (x[t] < mn))
            mn, amin = np.where(take, x[t], mn), np.where(take, np.int32(t), amin)
            take = ok & ((amax < 0) | (x[t] > mx))
            mx, amax = np.where(take, x[t], mx), np.where(take, np.int32(t), amax)
            first_nan = np.where(nan[t] & (first_nan < 0), np.int32(t), first_nan)
        if not skipna:
            hit = nans > 0
            mn, mx = np.where(hit, T(np.nan), mn), np.where(hit, T(np.nan), mx)
            amin, amax = np.where(hit, first_nan, amin), np.where(hit, first_nan, amax)
        out.update(min=mn.astype(T), max=mx.astype(T), argmin=amin.astype(np.int32), argmax=amax.astype(np.int32))

        A = np.sort(x, axis=0)                              # NaN last
        nv = (k - nans).astype(np.int64)
        bad = (nv == 0) | (nans > 0 if not skipna else False)
        out['median'] = median(A, nv, bad)
        for p in q:
            out[name(p)] = percentile(A, nv, bad, p)
    return out


# ---- comparisons --------------------------------------------------------------------------------------------------
def same_bits(got, want, what=''):
    """integers equal; floats: NaN where `want` has NaN, the same bits elsewhere"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind != 'f':
        assert np.array_equal(got, want), '%s: %d of %d differ' % (what, (got != want).sum(), got.size)
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), '%s: NaN at other places: %d against %d' % (what, gn.sum(), wn.sum())
    view = 'i%d' % got.dtype.itemsize
    gi = np.where(gn, 0, np.ascontiguousarray(got).view(view))
    wi = np.where(wn, 0, np.ascontiguousarray(want).view(view))
    diff = gi != wi
    if diff.any():
        at = tuple(np.argwhere(diff)[0])
        raise AssertionError('%s: %d of %d values differ in bits, first at %s: %r against %r'
                             % (what, diff.sum(), diff.size, at, got[at], want[at]))


def same_values(got, want, what=''):
    """== with NaN where `want` has NaN: the order statistics, whose zeros have no pinned sign"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), '%s: NaN at other places: %d against %d' % (what, gn.sum(), wn.sum())
    diff = ~wn & (got != want)
    if diff.any():
        at = tuple(np.argwhere(diff)[0])
        raise AssertionError('%s: %d of %d values differ, first at %s: %r against %r'
                             % (what, diff.sum(), diff.size, at, got[at], want[at]))


def same(got, want, what=''):
    """a dict of results against the restatement's: float64 and integer outputs by their bits, the T-typed order
    statistics, min and max by =="""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key in got:
        if key in MOMENTS or key in INTEGERS:
            same_bits(got[key], want[key], '%s %s' % (what, key))
        else:
            same_values(got[key], want[key], '%s %s' % (what, key))
