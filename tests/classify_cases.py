"""Seeded cases for the classification tests: small speckle stacks, labels and model recipes, shared by the
golden generator (tests/golden/make_classify_golden.py) and the tests."""
import numpy as np

NY, NX, NT = 24, 32, 4
VARS = ('C11', 'C22', 'ratio')
DTYPES = (np.float32, np.float64)
F32, F64 = (np.float32,), (np.float32, np.float64)
# name -> (number of classes, feature_dims, scale, dates, data types).  The recorded probabilities are most of
# the golden file, so the many-class models see one date and only three models are recorded for float64.
FORESTS = {'rf2': (2, (), False, NT, F32), 'rf3': (3, (), False, NT, F64), 'rf7': (7, (), False, 1, F32),
           'rf11': (11, (), False, 1, F32), 'rf3_time': (3, ('time',), False, NT, F64),
           'rf3_scale': (3, (), True, NT, F64), 'et3': (3, (), False, NT, F32), 'tree3': (3, (), False, NT, F32)}
KMEANS = {'km3': (3, (), False, NT, F64), 'km5_time': (5, ('time',), False, NT, F64),
          'km3_scale': (3, (), True, NT, F64), 'mbk3': (3, (), False, NT, F64)}


def class_map(n_classes, seed=0):
    """(NY, NX) labels 1 .. n_classes in blocks"""
    rng = np.random.default_rng(100 + seed)
    coarse = rng.integers(1, n_classes + 1, size=(NY // 8, NX // 8))
    coarse.reshape(-1)[:n_classes] = np.arange(1, n_classes + 1)
    return np.kron(coarse, np.ones((8, 8), np.int64))


def stack(n_classes, dtype, seed=0, nan=True, nt=NT):
    """-> ({var: (nt, NY, NX) array}, truth (NY, NX)): gamma speckle around class-dependent means that
    overlap, a few NaN pixels in one variable"""
    rng = np.random.default_rng(seed)
    truth = class_map(n_classes, seed)
    level = 1.0 + 0.6 * truth.astype(np.float64)
    c11 = level[None] * rng.gamma(4.0, 0.25, size=(nt, NY, NX))
    c22 = (2.0 + np.sin(level))[None] * rng.gamma(4.0, 0.25, size=(nt, NY, NX))
    ratio = c11 / c22
    out = {'C11': c11.astype(dtype), 'C22': c22.astype(dtype), 'ratio': ratio.astype(dtype)}
    if nan:
        out['C22'][1 % nt, 5, 7] = np.nan
        out['C22'][:, 20, 3] = np.nan
        out['C11'][nt - 1, 22, 28:31] = np.nan
    return out, truth


def training_labels(truth, fraction=0.3, seed=0):
    """truth on a random `fraction` of the pixels, 0 elsewhere, one NaN"""
    rng = np.random.default_rng(200 + seed)
    lab = np.where(rng.random(truth.shape) < fraction, truth, 0).astype(np.float64)
    lab[0, 0] = np.nan
    return lab


def variables(data, layout='tyx'):
    """the stack as the (dims, array) list classify_ref.build_X takes"""
    if layout == 'tyx':
        return [(('time', 'y', 'x'), data[v]) for v in VARS]
    return [(('y', 'x', 'time'), np.ascontiguousarray(np.transpose(data[v], (1, 2, 0)))) for v in VARS]


def data_dims(feature_dims):
    return tuple(d for d in ('time', 'y', 'x') if d not in feature_dims)


def integer_stack(seed=0):
    """integer-valued features, so that many lie exactly on a tree's thresholds after a fit on half-integers"""
    rng = np.random.default_rng(300 + seed)
    X = rng.integers(0, 12, size=(4000, 3)).astype(np.float64)
    y = (X[:, 0] + 2 * X[:, 1] > 14).astype(np.int64) + (X[:, 2] > 6)
    return X, y


def array_forest(X, n_classes, n_trees=7, depth=5, seed=0):
    """A forest as scikit-learn's arrays, built without scikit-learn: complete trees in heap order (the children
    of node i are 2 i + 1 and 2 i + 2) whose inner nodes take the features in turn, so that a forest of a few
    trees reads every feature, and test them against values the float32 matrix holds: features lie exactly on
    thresholds.  Leaf rows are random distributions over the classes.
    -> (feature, threshold, left, right, value, tree_offsets, classes)"""
    rng = np.random.default_rng(400 + seed)
    X32 = X[~np.isnan(X).any(axis=1)].astype(np.float32)
    inner, n = 2 ** depth - 1, 2 ** (depth + 1) - 1
    feature, threshold, left, right = [], [], [], []
    for t in range(n_trees):
        for i in range(n):
            f = (t + i) % X.shape[1]
            feature.append(f if i < inner else -2)
            threshold.append(float(X32[rng.integers(0, X32.shape[0]), f]) if i < inner else -2.0)
            left.append(2 * i + 1 if i < inner else -1)
            right.append(2 * i + 2 if i < inner else -1)
    value = rng.random((len(feature), n_classes))
    value /= value.sum(axis=1, keepdims=True)
    return (np.array(feature), np.array(threshold), np.array(left), np.array(right), value,
            np.arange(n_trees + 1) * n, np.arange(1, n_classes + 1))
