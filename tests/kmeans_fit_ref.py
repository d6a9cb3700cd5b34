"""A numpy restatement of k-means training as include/nd_amd.h defines it (nd_amd_feature_moments,
nd_amd_kmeans_step, nd_amd_gather_rows) and of the Lloyd driver of nd_amd.classify.fit_kmeans, which is
scikit-learn 1.7.2's _kmeans_single_lloyd in float64 with one difference: an empty cluster keeps its centre.
Also the seeded cases the golden file (tests/golden/make_kmeans_fit_golden.py) and the tests share: speckle-like
gamma stacks with class structure."""
import numpy as np

from tests import classify_cases as cases, classify_ref as ref

DTYPES = cases.DTYPES
# name -> (variables, dates, feature_dims, n_clusters, scale); every stack is (dates, 24, 32) per variable
CASES = {'f2k3': (2, 5, (), 3, False), 'f4k5': (4, 5, (), 5, False), 'f12k8': (3, 4, ('time',), 8, False),
         'f3k2': (3, 5, (), 2, False), 'f8k6_scale': (4, 2, ('time',), 6, True), 'f4k16_scale': (4, 5, (), 16, True)}


# ---- stacks ---------------------------------------------------------------------------------------------
def class_map(ny, nx, n_classes, seed=0):
    """(ny, nx) labels 1 .. n_classes in blocks of 8 x 8 (classify_cases.class_map where the shape is its own)"""
    if (ny, nx) == (cases.NY, cases.NX):
        return cases.class_map(n_classes, seed)
    rng = np.random.default_rng(100 + seed)
    coarse = rng.integers(1, n_classes + 1, size=(-(-ny // 8), -(-nx // 8)))
    coarse.reshape(-1)[:n_classes] = np.arange(1, n_classes + 1)
    return np.kron(coarse, np.ones((8, 8), np.int64))[:ny, :nx]


def stack(nvars, shape, n_classes, dtype, seed=0, nan=True, constant=None):
    """-> {name: (nt, ny, nx) array}: gamma speckle (4 looks) around class-dependent means that overlap, another
    mean per variable; NaN: single pixels, one pixel on every date, and the 64 consecutive pixels 128 .. 191 of
    the first date of the first variable (one whole wave of rows).  constant: a variable that is 2.5 everywhere."""
    nt, ny, nx = shape
    rng = np.random.default_rng(seed)
    truth = class_map(ny, nx, n_classes, seed)
    out = {}
    for v in range(nvars):
        level = 1.0 + 0.5 * ((truth + 2 * v) % n_classes) + 0.3 * v
        out['v%02d' % v] = (level[None] * rng.gamma(4.0, 0.25, size=shape)).astype(dtype)
    if constant is not None:
        out['v%02d' % constant][...] = 2.5
    if nan:
        first, last = out['v00'], out['v%02d' % (nvars - 1)]
        first.reshape(-1)[128:192] = np.nan
        first[:, ny // 2, 3] = np.nan
        last[nt - 1, ny - 2, nx - 4:nx - 1] = np.nan
        last[1 % nt, 5, 7] = np.nan
    return out


def variables(data, layout='tyx'):
    if layout == 'tyx':
        return [(('time', 'y', 'x'), a) for a in data.values()]
    return [(('y', 'x', 'time'), np.ascontiguousarray(np.transpose(a, (1, 2, 0)))) for a in data.values()]


def case(name, dtype):
    """-> (data, X (rows, features) with its NaN rows, feature_dims, k, scale, init (k, features) float64 | None).
    The initial centres are k distinct rows without NaN; of a scaled case they are drawn by scaled_init once
    the scaler is known."""
    nvars, nt, fdims, k, scale = CASES[name]
    seed = sorted(CASES).index(name)
    data = stack(nvars, (nt, cases.NY, cases.NX), max(2, min(k, 6)), dtype, seed=seed)
    X, _ = ref.build_X(variables(data), cases.data_dims(fdims), fdims)
    return data, X, fdims, k, scale, (None if scale else draw_init(X, k, seed))


def draw_init(Xs, k, seed):
    """k distinct rows without NaN of the (scaled) matrix, as float64"""
    keep = np.flatnonzero(~np.isnan(Xs).any(axis=1))
    pick = np.random.default_rng(500 + seed).choice(keep, size=k, replace=False)
    return Xs[pick].astype(np.float64)


def scaled_init(name, X, mean, scale_):
    return draw_init(ref.scale(X, mean, scale_), CASES[name][3], sorted(CASES).index(name))


# ---- the definitions ------------------------------------------------------------------------------------
def values(X, mean=None, scale_=None):
    """-> (float64 values of the rows as the kernels see them, valid (rows,)): the scaler applied in X's type"""
    valid = ~np.isnan(X).any(axis=1)
    Xs = X if mean is None else ref.scale(X, mean, scale_)
    return Xs.astype(np.float64), valid


def moments(X, mean=None, scale_=None):
    """-> (count, mean, population variance in two passes) over the valid rows"""
    V, valid = values(X, mean, scale_)
    V = V[valid]
    n = V.shape[0]
    with np.errstate(invalid='ignore', divide='ignore'):
        m = V.sum(axis=0) / n
        var = ((V - m) ** 2).sum(axis=0) / n
    return n, m, var


def scaler_scale(var):
    s = np.sqrt(var)
    s[s == 0.0] = 1.0
    return s


def step(X, centers, prev, mean=None, scale_=None, chunk=16384):
    """one Lloyd iteration -> (labels int32 with -1 for invalid rows, sums (k, F), counts (k,), inertia,
    changed, magnitude): magnitude (k, F) is the sum of |x| behind every entry of sums, what the forward bound of
    a float64 sum in any order is relative to"""
    V, valid = values(X, mean, scale_)
    centers = np.asarray(centers, np.float64)
    k, F = centers.shape
    labels = np.full(X.shape[0], -1, np.int32)
    best = np.zeros(X.shape[0])
    for lo in range(0, X.shape[0], chunk):
        d = ref.kmeans_d2(np.nan_to_num(V[lo:lo + chunk]), centers)
        j = np.argmin(d, axis=1)                     # the first minimum
        labels[lo:lo + chunk] = j
        best[lo:lo + chunk] = d[np.arange(d.shape[0]), j]
    labels[~valid] = -1
    sums, mag, counts = np.zeros((k, F)), np.zeros((k, F)), np.zeros(k, np.int64)
    for j in range(k):
        sel = labels == j
        counts[j] = sel.sum()
        sums[j] = V[sel].sum(axis=0)
        mag[j] = np.abs(V[sel]).sum(axis=0)
    inertia = float(best[valid].sum())
    changed = int((valid & (labels != np.asarray(prev).reshape(-1))).sum())
    return labels, sums, counts, inertia, changed, mag


def lloyd(X, init, max_iter=300, tol=1e-4, mean=None, scale_=None):
    """-> dict(centers, labels, n_iter, inertia, counts, empty): new centre = sums / counts (an empty cluster keeps
    its centre); strict stop when no label changed, else stop when sum((new - old)^2) <= tol * mean(var); after a
    stop that was not strict one more assignment for the final centres"""
    centers = np.array(init, np.float64)
    threshold = tol * float(np.mean(moments(X, mean, scale_)[2]))
    labels = np.full(X.shape[0], -1, np.int32)
    strict = False
    for n_iter in range(1, max_iter + 1):
        labels, sums, counts, inertia, changed, _ = step(X, centers, labels, mean, scale_)
        new = centers.copy()
        full = counts > 0
        new[full] = sums[full] / counts[full, None]
        shift = float(((new - centers) ** 2).sum())
        centers = new
        if changed == 0:
            strict = True
            break
        if shift <= threshold:
            break
    if not strict:
        labels, _, counts, inertia, _, _ = step(X, centers, labels, mean, scale_)
    return dict(centers=centers, labels=labels, n_iter=n_iter, inertia=inertia, counts=counts,
                empty=np.flatnonzero(counts == 0))
