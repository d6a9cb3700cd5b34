"""The numpy restatement of "Statistics of zones" (include/nd_amd.h): keys, the caller's stable argsort and offsets, the
fixed tree of every floating-point sum, the six statistics and paint.  The device result equals it bit for bit.

The tree over a zone's positions 0 .. m - 1 (its pixels in raster order): chunks of CHUNK = 64 positions summed by the
aligned pairwise tree (position l with l ^ 1, the pairs with ^ 2, ... ^ 32; an absent or NaN operand does not take
part: a (+) absent = a); the chunk sums of a segment of 64 chunks added sequentially in order; the segment sums added
sequentially in order.  Zones are batched by their number of chunks, which changes no operation."""
import numpy as np

CHUNK = 64
SEG_CHUNKS = 64
SEG = CHUNK * SEG_CHUNKS
STATS = ('count', 'nan_count', 'sum', 'min', 'max', 'm2')


def _label_ints(labels):
    """-> (int64 values, bool: the label is an integer at all)"""
    lab = np.asarray(labels)
    if lab.dtype == np.bool_:
        lab = lab.astype(np.uint8)
    if lab.dtype.kind == 'f':
        with np.errstate(invalid='ignore'):
            ok = (lab >= -9223372036854775808.0) & (lab < 9223372036854775808.0) & (lab == np.trunc(lab))
            return np.where(ok, lab, 0).astype(np.int64), ok
    return lab.astype(np.int64), np.ones(lab.shape, bool)


def default_n(labels):
    """the largest label that is a positive whole number, 0 if there is none"""
    v, ok = _label_ints(labels)
    v = v[ok]
    return max(int(v.max()), 0) if v.size else 0


def keys(labels, ids=None, n=None):
    """-> (int32 keys of the plane's shape: the zone's rank, or n; n; int64 ids)"""
    v, ok = _label_ints(labels)
    if ids is None:
        n = default_n(labels) if n is None else int(n)
        ids = np.arange(1, n + 1, dtype=np.int64)
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    if n == 0:
        return np.zeros(v.shape, np.int32), 0, ids
    r = np.searchsorted(ids, v)
    hit = ok & (r < n) & (ids[np.minimum(r, n - 1)] == v)
    return np.where(hit, r, n).astype(np.int32), n, ids


def index(k, n):
    """what the caller builds between the two entries: perm, the stable argsort of the keys (int32), and offsets[z], the
    number of keys < z (int64, n + 1 entries)"""
    flat = np.asarray(k).reshape(-1)
    perm = np.argsort(flat, kind='stable').astype(np.int32)
    offsets = np.searchsorted(flat[perm], np.arange(n + 1)).astype(np.int64)
    return perm, offsets


def tree(c, part):
    """the sum over the last axis (positions, a multiple of CHUNK long) of the float64 c where `part`, in the fixed tree
    -> (sum, bool: anything took part)"""
    lead = c.shape[:-1]
    v = c.reshape(lead + (-1, CHUNK))
    ok = part.reshape(v.shape)
    with np.errstate(all='ignore'):
        while v.shape[-1] > 1:
            a, b, oa, ob = v[..., 0::2], v[..., 1::2], ok[..., 0::2], ok[..., 1::2]
            v = np.where(oa & ob, a + b, np.where(oa, a, b))
            ok = oa | ob
        v, ok = v[..., 0], ok[..., 0]                   # (..., chunks)
        nchunk = v.shape[-1]
        pad = -nchunk % SEG_CHUNKS
        if pad:
            v = np.concatenate([v, np.zeros(lead + (pad,))], -1)
            ok = np.concatenate([ok, np.zeros(lead + (pad,), bool)], -1)
        v = v.reshape(lead + (-1, SEG_CHUNKS))
        ok = ok.reshape(v.shape)

        def chain(v, ok):                               # sequentially along the last axis
            acc, has = v[..., 0], ok[..., 0]
            for i in range(1, v.shape[-1]):
                acc = np.where(has & ok[..., i], acc + v[..., i], np.where(ok[..., i], v[..., i], acc))
                has = has | ok[..., i]
            return acc, has
        v, ok = chain(v, ok)                            # (..., segments)
        return chain(v, ok)


def stats(planes, perm, offsets, n):
    """planes (P, ny, nx) of float32 / float64 (integers are computed as float64) -> a dict of (P, n) arrays"""
    planes = np.asarray(planes)
    if planes.dtype.kind != 'f':
        planes = planes.astype(np.float64)
    P = planes.shape[0]
    flat = planes.reshape(P, -1)
    out = {'count': np.zeros((P, n), np.int64), 'nan_count': np.zeros((P, n), np.int64), 'sum': np.zeros((P, n)),
           'min': np.full((P, n), np.nan), 'max': np.full((P, n), np.nan), 'm2': np.zeros((P, n))}
    if n == 0 or flat.shape[1] == 0:
        return out
    m = np.diff(offsets)
    nch = -(-m // CHUNK)
    for k in np.unique(nch[nch > 0]):
        zs = np.nonzero(nch == k)[0]
        pos = np.arange(int(k) * CHUNK)[None, :]
        present = pos < m[zs][:, None]
        src = perm[np.minimum(offsets[zs][:, None] + pos, len(perm) - 1)]
        x = flat[:, src]                                # (P, zones, positions)
        isnan = x != x
        part = present[None] & ~isnan
        c = x.astype(np.float64)
        cnt = part.sum(-1)
        s, has = tree(c, part)
        s = np.where(has, s, 0.0)
        with np.errstate(all='ignore'):
            mean = s / cnt.astype(np.float64)
            d = c - mean[..., None]
            q = d * d
        m2, has2 = tree(q, part)
        out['count'][:, zs] = cnt
        out['nan_count'][:, zs] = (present[None] & isnan).sum(-1)
        out['sum'][:, zs] = s
        out['m2'][:, zs] = np.where(has2, m2, 0.0)
        out['min'][:, zs] = np.where(cnt > 0, np.where(part, c, np.inf).min(-1), np.nan)
        out['max'][:, zs] = np.where(cnt > 0, np.where(part, c, -np.inf).max(-1), np.nan)
    return out


def mean(st):
    with np.errstate(all='ignore'):
        return st['sum'] / st['count'].astype(np.float64)


def var(st, ddof=0):
    with np.errstate(all='ignore'):
        return st['m2'] / (st['count'] - ddof).astype(np.float64)


def std(st, ddof=0):
    with np.errstate(all='ignore'):
        return np.sqrt(var(st, ddof))


def zonal_stats(planes, labels, ids=None):
    """keys, index and stats in one call -> (dict of (P, n) arrays, ids)"""
    k, n, ids = keys(labels, ids)
    perm, offsets = index(k, n)
    return stats(planes, perm, offsets, n), ids


def paint(table, k, dtype, src=None, fill=np.nan):
    """table (P, n) float64, keys (ny, nx) -> (P, ny, nx) of dtype: a zone's pixels get its entry, the others src's value
    or fill"""
    table = np.asarray(table, np.float64)
    P, n = table.shape
    dtype = np.dtype(dtype)
    zoned = k < n
    out = np.empty((P,) + k.shape, dtype)
    with np.errstate(all='ignore'):
        for p in range(P):
            rest = src[p] if src is not None else dtype.type(fill)
            out[p] = np.where(zoned, table[p][np.minimum(k, max(n - 1, 0))].astype(dtype) if n else rest, rest)
    return out


def same(got, want):
    """the device's float64 (or count) table against the restatement's: NaN where it has NaN, the same bits elsewhere"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind != 'f':
        assert np.array_equal(got, want), '%d of %d counts differ' % ((got != want).sum(), got.size)
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), 'NaN at other places: %d against %d' % (gn.sum(), wn.sum())
    gi = np.where(gn, 0, np.ascontiguousarray(got).view('i%d' % got.dtype.itemsize))
    wi = np.where(wn, 0, np.ascontiguousarray(want).view('i%d' % want.dtype.itemsize))
    diff = gi != wi
    assert not diff.any(), '%d of %d values differ in bits, first at %s: %r against %r' % (
        diff.sum(), diff.size, tuple(np.argwhere(diff)[0]), got[tuple(np.argwhere(diff)[0])],
        want[tuple(np.argwhere(diff)[0])])


def same_minmax(got, want):
    """min / max compare ==, the sign of a zero is not pinned; NaN where the restatement has NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert (got[ok] == want[ok]).all()


def same_stats(got, want):
    assert set(got) >= set(want) or set(want) >= set(got)
    for name in got:
        if name not in want:
            continue
        (same_minmax if name in ('min', 'max') else same)(np.asarray(got[name]), np.asarray(want[name]))
