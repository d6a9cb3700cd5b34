"""A numpy restatement of k-nearest-neighbour and linear classification as include/nd_amd.h defines them
(nd_amd_classify_knn, nd_amd_classify_linear), and the seeded recipes that the golden generator
(tests/golden/make_classify_knn_linear_golden.py) and the tests share.  Data, labels and the (rows, features)
matrix come from tests/classify_cases.py and tests/classify_ref.py."""
import numpy as np

from tests import classify_cases as cases, classify_ref as ref

# name -> (n_neighbors, number of classes, feature_dims, scale, algorithm)
KNN = {'knn1': (1, 3, (), False, 'auto'), 'knn3': (3, 3, (), False, 'auto'), 'knn5_c2': (5, 2, (), False, 'brute'),
       'knn8_time': (8, 3, ('time',), False, 'auto'), 'knn9_c11': (9, 11, (), False, 'auto'),
       'knn32': (32, 3, (), False, 'brute'), 'knn3_scale': (3, 3, (), True, 'auto'),
       'knn5_c11_time': (5, 11, ('time',), False, 'brute')}
# name -> (estimator, number of classes, scale); one date, so that the recorded decision values stay small
LINEAR = {'lr2': ('LogisticRegression', 2, False), 'lr3': ('LogisticRegression', 3, False),
          'lr11': ('LogisticRegression', 11, False), 'lr3_scale': ('LogisticRegression', 3, True),
          'svc3': ('LinearSVC', 3, False), 'ridge3': ('RidgeClassifier', 3, False),
          'sgd3': ('SGDClassifier', 3, False)}
KNN_FRACTION = 0.15          # of the pixels carry a training label
PROBA_CLASSES = 3            # probabilities are recorded for models of up to this many classes
KNN_GAP = 1e-6               # rows whose k-th and (k+1)-th distances are relatively closer are not compared
KNN_GAP_ROWS = 1e-3          # and may be at most this fraction of a case
LINEAR_TIE_ROWS = 1e-2       # rows whose two largest decision values lie within twice the bound


def make_linear(name):
    from sklearn import linear_model, svm
    kind = LINEAR[name][0]
    if kind == 'LogisticRegression':
        return linear_model.LogisticRegression(max_iter=300)
    if kind == 'LinearSVC':
        return svm.LinearSVC(random_state=0)
    if kind == 'RidgeClassifier':
        return linear_model.RidgeClassifier()
    return linear_model.SGDClassifier(random_state=0)


def knn_case(name, dtype):
    """-> data, X (rows, features), its row shape, (Xt, yt) the training rows"""
    k, ncls, fdims, _, _ = KNN[name]
    data, truth = cases.stack(ncls, dtype, seed=ncls)
    X, shape = ref.build_X(cases.variables(data), cases.data_dims(fdims), fdims)
    lab = ref.broadcast_array(cases.training_labels(truth, KNN_FRACTION, seed=ncls), shape).reshape(-1)
    Xt, yt, _ = ref.make_Xy(X, lab)
    return data, X, shape, (Xt, yt)


def linear_case(name, dtype):
    _, ncls, _ = LINEAR[name]
    data, truth = cases.stack(ncls, dtype, seed=ncls, nt=1)
    X, shape = ref.build_X(cases.variables(data), ('time', 'y', 'x'))
    lab = ref.broadcast_array(cases.training_labels(truth, seed=ncls), shape).reshape(-1)
    Xt, yt, _ = ref.make_Xy(X, lab)
    return data, X, shape, (Xt, yt)


# ---- k nearest neighbours ---------------------------------------------------------------------------
def knn_d2(X, train):
    """(rows, n_train) squared distances, float64, summed in feature order"""
    d = np.zeros((X.shape[0], train.shape[0]), np.float64)
    for f in range(X.shape[1]):
        e = X[:, f].astype(np.float64)[:, None] - train[None, :, f].astype(np.float64)
        d += e * e
    return d


def knn_neighbours(X, train, k):
    """-> (indices (rows, k) of the k samples smallest by (distance, index), in that order;
    relative gap between the k-th and the (k+1)-th distance, 1 where k == n_train)"""
    d = knn_d2(X, train)
    order = np.argsort(d, axis=1, kind='stable')
    if k == train.shape[0]:
        return order[:, :k], np.ones(X.shape[0])
    dk = np.take_along_axis(d, order[:, k - 1:k + 1], 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = np.where(dk[:, 1] > 0, (dk[:, 1] - dk[:, 0]) / dk[:, 1], 0.0)
    return order[:, :k], gap


def knn_proba(X, train, target, k, n_classes):
    """-> (count_c / k in float64, gap)"""
    nb, gap = knn_neighbours(X, train, k)
    counts = np.zeros((X.shape[0], n_classes), np.float64)
    for j in range(k):
        np.add.at(counts, (np.arange(X.shape[0]), np.asarray(target)[nb[:, j]]), 1.0)
    return counts / np.float64(k), gap


def first_max(values, classes):
    return np.asarray(classes, np.float64)[np.argmax(values, axis=1)]


# ---- linear -----------------------------------------------------------------------------------------
def linear_decision(X, coef, intercept):
    """(rows, n_rows) s_c = b_c + sum_f x_f w_cf in float64, summed in feature order, and S = |b_c| +
    sum_f |x_f w_cf|"""
    coef = np.asarray(coef, np.float64)
    b = np.broadcast_to(np.asarray(intercept, np.float64).reshape(-1), (coef.shape[0],))
    s = np.repeat(b[None], X.shape[0], 0).copy()
    S = np.abs(s)
    for f in range(X.shape[1]):
        term = X[:, f].astype(np.float64)[:, None] * coef[None, :, f]
        s += term
        S += np.abs(term)
    return s, S


def linear_bound(S, n_features, dtype):
    """2 (F + 2) u S: twice the forward bound of a sum of F + 1 terms whose products are rounded"""
    u = np.finfo(dtype).eps / 2
    return 2.0 * (n_features + 2) * u * S


def linear_predict(s, classes):
    classes = np.asarray(classes, np.float64)
    if s.shape[1] == 1:
        return classes[(s[:, 0] > 0).astype(np.int64)]
    return classes[np.argmax(s, axis=1)]


def expit(s):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where(s < 0, np.exp(s) / (1.0 + np.exp(s)), 1.0 / (1.0 + np.exp(-s)))


def linear_proba(s, link):
    if link == 'softmax':
        if s.shape[1] == 1:
            s = np.concatenate([-s, s], axis=1)
        e = np.exp(s - s.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    p = expit(s)
    if s.shape[1] == 1:
        return np.concatenate([1.0 - p, p], axis=1)
    return p / p.sum(axis=1, keepdims=True)


def linear_margin(s):
    """what separates the predicted class from the next: |s| for a binary model, else the difference of the
    two largest decision values"""
    if s.shape[1] == 1:
        return np.abs(s[:, 0])
    top = np.sort(s, axis=1)
    return top[:, -1] - top[:, -2]
