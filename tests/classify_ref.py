"""A numpy restatement of pixel classification as include/nd_amd.h defines it (and as nd/classify.py with
scikit-learn computes it): the (rows, features) matrix, label broadcast and masks, the forest walk, the
scaler's rounding, float64 k-means and the literal class_mean loop.  Plain dicts of dims -> arrays stand
in for datasets: {'dims': {name: size, ...} in data-dimension order, 'vars': [(dims, array), ...]}."""
import numpy as np


# ---- build_X: rows over data_dims, feature = position along feature_dims * n_variables + variable -------
def build_X(variables, data_dims, feature_dims=()):
    """variables: list of (dims, array).  Only variables spanning all data_dims take part."""
    used = [(d, a) for d, a in variables if set(data_dims) <= set(d)]
    fdims = [f for f in feature_dims if any(f in d for d, _ in used)]
    fshape = []
    for f in fdims:
        fshape.append(next(a.shape[d.index(f)] for d, a in used if f in d))
    shape = None
    cols = []
    for pos in np.ndindex(*fshape):
        for d, a in used:
            idx = tuple(pos[fdims.index(x)] if x in fdims else slice(None) for x in d)
            rest = [x for x in d if x not in fdims]
            plane = np.transpose(a[idx], [rest.index(x) for x in data_dims])
            shape = plane.shape
            cols.append(plane.reshape(-1))
    dt = np.result_type(*[c.dtype for c in cols])
    if dt.kind != 'f':
        dt = np.float64
    return np.stack(cols, axis=1).astype(dt), shape


def broadcast_array(arr, shape):
    """nd/classify.py:74-81"""
    matching = list(shape)
    new_shape = [1] * len(shape)
    for dim in arr.shape:
        i = matching.index(dim)
        new_shape[i] = dim
        matching[i] = None
    return np.broadcast_to(arr.reshape(new_shape), shape)


def broadcast_named(labels, label_dims, data_dims, shape):
    """labels over a subset of the data dimensions -> over all of them, in their order"""
    a = np.transpose(labels, [label_dims.index(d) for d in data_dims if d in label_dims])
    idx = tuple(slice(None) if d in label_dims else None for d in data_dims)
    return np.broadcast_to(a[idx], shape)


def make_Xy(X, labels_flat=None):
    """the masks of make_Xy: label not NaN and > 0, no NaN feature; row order kept"""
    if labels_flat is None:
        keep = ~np.isnan(X).any(axis=1)
        return X[keep], None, keep
    lab = np.asarray(labels_flat)
    with np.errstate(invalid='ignore'):
        ymask = ~np.isnan(lab.astype(np.float64)) & (lab > 0)
    keep = ymask & ~np.isnan(X).any(axis=1)
    return X[keep], lab[keep], keep


# ---- scaler: X -= mean_; X /= scale_ in place on X of its own type with float64 operands ---------------
def scale(X, mean, scale_):
    X = X.copy()
    X[...] = (X.astype(np.float64) - mean).astype(X.dtype)
    X[...] = (X.astype(np.float64) / scale_).astype(X.dtype)
    return X


# ---- forest ---------------------------------------------------------------------------------------
def forest_proba(X, feature, threshold, left, right, value, tree_offsets):
    """walk every tree with float32(x) <= float64 threshold, add the leaf rows in tree order, one float64
    add per class per tree, divide by the tree count"""
    X32 = X.astype(np.float32)
    n = X32.shape[0]
    out = np.zeros((n, value.shape[1]), np.float64)
    rows = np.arange(n)
    for t in range(len(tree_offsets) - 1):
        base = int(tree_offsets[t])
        node = np.full(n, base, np.int64)
        while True:
            inner = left[node] >= 0
            if not inner.any():
                break
            i = node[inner]
            go_left = X32[rows[inner], feature[i]].astype(np.float64) <= threshold[i]
            node[inner] = base + np.where(go_left, left[i], right[i])
        out += value[node]
    out /= (len(tree_offsets) - 1)
    return out


def forest_predict(proba, classes):
    return np.asarray(classes, np.float64)[np.argmax(proba, axis=1)]


def packed_proba(X, nodes, roots, value):
    """an interpreter of the packed 16-byte nodes {bits of t32, feature (-1 leaf), left | value row, right}"""
    X32 = X.astype(np.float32)
    t32 = np.ascontiguousarray(nodes[:, 0]).view(np.float32)
    n = X32.shape[0]
    out = np.zeros((n, value.shape[1]), np.float64)
    rows = np.arange(n)
    for r in roots:
        node = np.full(n, int(r), np.int64)
        while True:
            inner = nodes[node, 1] >= 0
            if not inner.any():
                break
            i = node[inner]
            go_left = X32[rows[inner], nodes[i, 1]] <= t32[i]
            node[inner] = np.where(go_left, nodes[i, 2], nodes[i, 3])
        out += value[nodes[node, 2]]
    out /= len(roots)
    return out


def masked(result, keep):
    """scatter the kept rows' results back, NaN elsewhere (nd/classify.py:239-240)"""
    out = np.full(keep.shape + result.shape[1:], np.nan)
    out[keep] = result
    return out


# ---- k-means ----------------------------------------------------------------------------------------
def kmeans_d2(X, centers):
    """(rows, k) squared distances, float64, summed in feature order"""
    d = np.zeros((X.shape[0], centers.shape[0]), np.float64)
    for f in range(X.shape[1]):
        e = X[:, f].astype(np.float64)[:, None] - centers[None, :, f].astype(np.float64)
        d += e * e
    return d


def kmeans_labels(X, centers):
    return np.argmin(kmeans_d2(X, centers), axis=1).astype(np.float64)


def kmeans_gap(X, centers):
    """relative gap (d2 - d1) / d2 between nearest and second-nearest squared distance (1 for k = 1)"""
    d = np.sort(kmeans_d2(X, centers), axis=1)
    if d.shape[1] < 2:
        return np.ones(d.shape[0])
    with np.errstate(invalid='ignore', divide='ignore'):
        g = (d[:, 1] - d[:, 0]) / d[:, 1]
    return np.where(d[:, 1] > 0, g, 0.0)


# ---- class_mean: the literal loop ---------------------------------------------------------------------
def class_mean(a, labels):
    """labels already broadcast to a.shape.  means.where(labels != l).fillna(means.where(labels == l).mean())"""
    n = len(np.unique(labels))
    means = np.array(a, dtype=a.dtype if a.dtype.kind == 'f' else np.float64)
    for l in range(n):
        sel = labels == l
        inside = means[sel]
        inside = inside[~np.isnan(inside)]
        m = inside.astype(np.float64).mean() if inside.size else np.nan
        wherenot = np.where(sel, np.nan, means)
        means = np.where(np.isnan(wherenot), m, wherenot).astype(means.dtype)
    return means
