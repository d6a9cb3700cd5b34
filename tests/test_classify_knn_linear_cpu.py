"""k-nearest-neighbour and linear classification without a GPU: the numpy restatement
(tests/classify_knn_linear_ref.py) against scikit-learn 1.7.2's recorded output
(tests/golden/classify_knn_linear_sklearn.npz) and against live scikit-learn, what from_sklearn refuses, the
keys of the Classifier's model cache, and the C ABI declarations."""
import os
import re

import numpy as np
import pytest

from nd_amd import classify, xr_lite
from tests import classify_cases as cases, classify_knn_linear_ref as kl, classify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'classify_knn_linear_sklearn.npz')
NEW_SYMBOLS = ('nd_amd_classify_knn', 'nd_amd_classify_linear')
KNN_CASES = [(n, dt) for n in kl.KNN for dt in cases.DTYPES]
LINEAR_CASES = [(n, dt) for n in kl.LINEAR for dt in cases.DTYPES]


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def kept(name, dtype, case, g):
    """the rows without NaN of a recipe, scaled as recorded"""
    X = case(name, dtype)[1]
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    Xp = X[~np.isnan(X).any(axis=1)]
    if key + 'mean' in g.files:
        Xp = ref.scale(Xp, g[key + 'mean'], g[key + 'scale'])
    return key, Xp


def sklearn_decision(Xp, coef, intercept):
    """LinearClassifierMixin.decision_function: X @ coef_.T + intercept_ in the arrays' common type"""
    s = Xp @ coef.T + intercept
    return s.reshape(Xp.shape[0], -1)


def check_linear(Xp, coef, intercept, classes, link, decision, predict, proba=None):
    """scikit-learn's output against the restatement, inside the bounds the GPU test uses"""
    s, S = kl.linear_decision(Xp, coef, intercept)
    bound = kl.linear_bound(S, Xp.shape[1], np.result_type(Xp.dtype, coef.dtype))
    decision = np.asarray(decision, np.float64).reshape(s.shape)
    assert np.all(np.abs(s - decision) <= bound), np.max(np.abs(s - decision) / bound)
    sure = kl.linear_margin(s) > 2 * bound.max(axis=1)
    assert (~sure).mean() <= kl.LINEAR_TIE_ROWS
    np.testing.assert_array_equal(kl.linear_predict(s, classes)[sure], np.asarray(predict, np.float64)[sure])
    if proba is not None:
        u = np.finfo(np.result_type(Xp.dtype, coef.dtype)).eps / 2
        tol = 2 * bound.max(axis=1, keepdims=True) + 8 * u
        got = kl.linear_proba(s, link)
        assert np.all(np.abs(got - proba) <= tol), np.max(np.abs(got - proba) / tol)


def test_golden_is_sklearn_1_7_2(golden):
    assert str(golden['sklearn_version']) == '1.7.2'
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'classify_sklearn.npz'))
    assert str(golden['float64/lr3/link']) == 'softmax' and str(golden['float64/lr2/link']) == 'ovr'
    assert str(golden['float32/svc3/link']) == 'none'


@pytest.mark.parametrize('name,dtype', KNN_CASES)
def test_knn_restatement_matches_golden(golden, name, dtype):
    k, ncls = kl.KNN[name][:2]
    key, Xp = kept(name, dtype, kl.knn_case, golden)
    train, target, classes = golden[key + 'train'], golden[key + 'target'], golden[key + 'classes']
    assert train.dtype == dtype and len(classes) == ncls and k <= train.shape[0]
    proba, gap = kl.knn_proba(Xp, train, target, k, ncls)
    ok = gap >= kl.KNN_GAP
    assert (~ok).mean() <= kl.KNN_GAP_ROWS
    np.testing.assert_array_equal(kl.first_max(proba, classes)[ok], golden[key + 'predict'][ok])
    if key + 'proba' in golden.files:
        assert proba[ok].tobytes() == golden[key + 'proba'][ok].tobytes()
    model = classify.KNNModel(train, target, classes, k)
    assert model.n_features == Xp.shape[1] and model.n_classes == ncls and model.train.dtype == np.float64


@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_knn_restatement_matches_live_sklearn(dtype):
    pytest.importorskip('sklearn')
    from sklearn.neighbors import KNeighborsClassifier
    data, truth = cases.stack(3, dtype, seed=11, nan=False)
    for fdims in ((), ('time',)):
        X, shape = ref.build_X(cases.variables(data), cases.data_dims(fdims), fdims)
        lab = ref.broadcast_array(cases.training_labels(truth, seed=11), shape).reshape(-1)
        Xt, yt, _ = ref.make_Xy(X, lab)
        for k, algorithm in ((1, 'auto'), (3, 'kd_tree'), (5, 'brute')):
            clf = KNeighborsClassifier(k, algorithm=algorithm).fit(Xt, yt)
            model = classify.KNNModel.from_sklearn(clf)
            assert model.train.dtype == np.float64 and model.n_neighbors == k
            proba, gap = kl.knn_proba(X, model.train, model.target, k, model.n_classes)
            ok = gap >= kl.KNN_GAP
            assert (~ok).mean() <= kl.KNN_GAP_ROWS
            assert proba[ok].tobytes() == clf.predict_proba(X)[ok].tobytes()
            np.testing.assert_array_equal(kl.first_max(proba, model.classes)[ok], clf.predict(X)[ok])


def test_knn_restatement_breaks_ties_by_index():
    train = np.array([[0., 0.], [2., 0.], [0., 0.], [2., 0.], [5., 5.]])
    target = np.array([1, 0, 0, 1, 2])
    X = np.array([[1., 0.], [0., 0.]])
    nb, gap = kl.knn_neighbours(X, train, 3)
    np.testing.assert_array_equal(nb, [[0, 1, 2], [0, 2, 1]])
    np.testing.assert_array_equal(gap, [0.0, 0.0])
    proba, _ = kl.knn_proba(X, train, target, 3, 3)
    np.testing.assert_array_equal(proba, np.array([[2, 1, 0], [2, 1, 0]]) / 3.0)
    np.testing.assert_array_equal(kl.first_max(np.array([[.5, .5, 0]]), [4, 5, 6]), [4.0])


@pytest.mark.parametrize('name,dtype', LINEAR_CASES)
def test_linear_restatement_matches_golden(golden, name, dtype):
    key, Xp = kept(name, dtype, kl.linear_case, golden)
    coef, intercept, classes = golden[key + 'coef'], golden[key + 'intercept'], golden[key + 'classes']
    link = str(golden[key + 'link'])
    decision = golden[key + 'decision'] if key + 'decision' in golden.files else sklearn_decision(Xp, coef, intercept)
    check_linear(Xp, coef, intercept, classes, link, decision, golden[key + 'predict'],
                 golden[key + 'proba'] if key + 'proba' in golden.files else None)
    if key + 'decision' in golden.files:          # the recorded values are scikit-learn's expression
        assert sklearn_decision(Xp, coef, intercept).tobytes() == decision.reshape(Xp.shape[0], -1).tobytes()
    model = classify.LinearModel(coef, intercept, classes, link)
    assert model.coef.shape == (1 if len(classes) == 2 else len(classes), Xp.shape[1])


@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_linear_restatement_matches_live_sklearn(dtype):
    pytest.importorskip('sklearn')
    from sklearn import linear_model
    for name in kl.LINEAR:
        _, X, _, (Xt, yt) = kl.linear_case(name, dtype)
        Xp = X[~np.isnan(X).any(axis=1)]
        clf = kl.make_linear(name).fit(Xt, yt)
        model = classify.LinearModel.from_sklearn(clf)
        has_proba = kl.LINEAR[name][0] == 'LogisticRegression'
        assert (model.link != 'none') == has_proba
        check_linear(Xp, clf.coef_, clf.intercept_, clf.classes_, model.link, clf.decision_function(Xp),
                     clf.predict(Xp), clf.predict_proba(Xp) if has_proba else None)
    # the link is the one LogisticRegression.predict_proba applies
    _, X, _, (Xt, yt) = kl.linear_case('lr3', dtype)
    Xp = X[~np.isnan(X).any(axis=1)]
    for clf, link in ((linear_model.LogisticRegression(solver='liblinear'), 'ovr'),
                      (linear_model.LogisticRegression(), 'softmax'),
                      (linear_model.LogisticRegressionCV(cv=2, Cs=2, max_iter=300), 'softmax')):
        clf.fit(Xt, yt)
        model = classify.LinearModel.from_sklearn(clf)
        assert model.link == link, type(clf).__name__
        check_linear(Xp, clf.coef_, clf.intercept_, clf.classes_, link, clf.decision_function(Xp), clf.predict(Xp),
                     clf.predict_proba(Xp))
    for clf in (linear_model.Perceptron(random_state=0), linear_model.PassiveAggressiveClassifier(random_state=0)):
        assert classify.LinearModel.from_sklearn(clf.fit(Xt, yt)).link == 'none'


def test_linear_restatement_links_and_ties():
    s = np.array([[1.0, 1.0, -2.0], [0.0, 3.0, 3.0]])
    np.testing.assert_array_equal(kl.linear_predict(s, [7, 8, 9]), [7.0, 8.0])
    np.testing.assert_array_equal(kl.linear_predict(np.array([[0.0], [1e-300], [-1.0]]), [7, 8]), [7.0, 8.0, 7.0])
    p = kl.linear_proba(s, 'softmax')
    np.testing.assert_allclose(p.sum(1), 1.0, rtol=1e-15)
    assert p[0, 0] == p[0, 1] and kl.linear_proba(np.array([[800.0, -800.0]]), 'softmax')[0, 0] == 1.0
    b = kl.linear_proba(np.array([[-800.0], [0.0], [800.0]]), 'ovr')
    np.testing.assert_array_equal(b, [[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])
    np.testing.assert_allclose(kl.linear_proba(np.array([[0.3]]), 'softmax'), kl.linear_proba(np.array([[0.6]]), 'ovr'),
                               rtol=1e-15)


def test_from_sklearn_refuses_what_is_not_served():
    pytest.importorskip('sklearn')
    from scipy import sparse
    from sklearn import linear_model, naive_bayes, neighbors, svm
    X, y = cases.integer_stack()
    X, y = X[:200], y[:200]
    knn = neighbors.KNeighborsClassifier
    unsupported = [knn(3, weights='distance'), knn(3, weights=lambda d: 1.0 / (d + 1)), knn(3, metric='manhattan'),
                   knn(3, p=1), knn(3, metric='minkowski', p=3), knn(3, metric='cosine'), knn(33)]
    for clf in unsupported:
        with pytest.raises(NotImplementedError, match='KNeighborsClassifier'):
            classify.KNNModel.from_sklearn(clf.fit(X, y))
    with pytest.raises(NotImplementedError, match='sparse'):
        classify.KNNModel.from_sklearn(knn(3).fit(sparse.csr_matrix(X), y))
    with pytest.raises(NotImplementedError, match='multi-output'):
        classify.KNNModel.from_sklearn(knn(3).fit(X, np.stack([y, y], 1)))
    with pytest.raises(NotImplementedError, match='numeric'):
        classify.KNNModel.from_sklearn(knn(3).fit(X, np.array(['u', 'v', 'w'])[y]))
    with pytest.raises(NotImplementedError, match='Got GaussianNB'):
        classify.KNNModel.from_sklearn(naive_bayes.GaussianNB().fit(X, y))
    for ok in (knn(32), knn(3, weights=None), knn(1, metric='euclidean'), knn(2, metric='minkowski', p=2)):
        assert classify.KNNModel.from_sklearn(ok.fit(X, y)).n_train == 200
    # the plain-array model
    with pytest.raises(NotImplementedError, match='n_neighbors=33'):
        classify.KNNModel(X, y, [0, 1, 2], 33)
    for bad in ((X, y, [0, 1, 2], 0), (X[:2], y[:2], [0, 1, 2], 3), (X, y[:-1], [0, 1, 2], 3), (X[:, 0], y, [0, 1, 2], 3),
                (X, y, [0, 1], 3), (X, -y, [0, 1, 2], 3), (np.where(X > 10, np.nan, X), y, [0, 1, 2], 3)):
        with pytest.raises(ValueError, match='KNNModel'):
            classify.KNNModel(*bad)
    with pytest.raises(NotImplementedError, match='numeric'):
        classify.KNNModel(X, y, ['a', 'b', 'c'], 3)
    # linear
    with pytest.raises(NotImplementedError, match='sparse'):
        classify.LinearModel.from_sklearn(linear_model.LogisticRegression().fit(X, y).sparsify())
    with pytest.raises(NotImplementedError, match='numeric'):
        classify.LinearModel.from_sklearn(svm.LinearSVC().fit(X, np.array(['u', 'v', 'w'])[y]))
    with pytest.raises(NotImplementedError, match='multi-output'):
        classify.LinearModel.from_sklearn(linear_model.RidgeClassifier().fit(X, np.stack([y > 0, y > 1], 1)))
    with pytest.raises(NotImplementedError, match='Got GaussianNB'):
        classify.LinearModel.from_sklearn(naive_bayes.GaussianNB().fit(X, y))
    for bad in ((np.ones(3), 0.0, [0, 1]), (np.ones((3, 2)), np.zeros(3), [0, 1]), (np.ones((1, 2)), 0.0, [0, 1, 2])):
        with pytest.raises(ValueError, match='LinearModel'):
            classify.LinearModel(*bad)
    with pytest.raises(ValueError, match='link'):
        classify.LinearModel(np.ones((1, 2)), 0.0, [0, 1], 'probit')
    # func: the predict-only estimators serve nothing else, and no linear model serves decision_function
    ds = xr_lite.Dataset({v: (('y', 'x'), np.ones((4, 5), np.float32)) for v in 'abc'})
    predict_only = (svm.LinearSVC(), linear_model.RidgeClassifier(), linear_model.SGDClassifier(loss='log_loss'),
                    linear_model.Perceptron(), linear_model.PassiveAggressiveClassifier())
    for clf in predict_only:
        for func in ('predict_proba', 'decision_function'):
            if hasattr(clf, func):
                with pytest.raises(NotImplementedError, match='func'):
                    classify.Classifier(clf.fit(X, y)).predict(ds, func=func)
    for func in ('decision_function', 'predict_log_proba'):
        with pytest.raises(NotImplementedError, match='func'):
            classify.Classifier(linear_model.LogisticRegression().fit(X, y)).predict(ds, func=func)
    with pytest.raises(NotImplementedError, match='func'):
        classify.Classifier(knn(3).fit(X, y)).predict(ds, func='kneighbors')
    with pytest.raises(NotImplementedError, match='func'):
        classify.predict_linear(ds, classify.LinearModel(np.ones((1, 3)), 0.0, [0, 1]), func='predict_proba')
    # what the extended message must still say
    for word in ('RandomForestClassifier', 'KMeans', 'func', 'numeric', 'KNeighborsClassifier', 'LogisticRegression'):
        assert word in classify._SUPPORTED


def test_model_cache_follows_partial_fit_and_refit():
    pytest.importorskip('sklearn')
    from sklearn import linear_model, neighbors
    X, y = cases.integer_stack()
    sgd = linear_model.SGDClassifier(random_state=0)
    sgd.partial_fit(X[:500], y[:500], classes=[0, 1, 2])
    c = classify.Classifier(sgd)
    first = c._cached_model('predict')
    assert isinstance(first, classify.LinearModel) and c._cached_model('predict') is first
    held = sgd.coef_
    sgd.partial_fit(X[500:1000] + 1, y[500:1000])
    assert sgd.coef_ is held                                   # scikit-learn updated the array in place
    second = c._cached_model('predict')
    assert second is not first and not np.array_equal(first.coef, second.coef)
    np.testing.assert_array_equal(second.coef, sgd.coef_)
    np.testing.assert_array_equal(second.intercept, sgd.intercept_)
    lr = linear_model.LogisticRegression().fit(X[:500], y[:500])
    c = classify.Classifier(lr)
    first = c._cached_model('predict')
    assert c._cached_model('predict_proba') is first           # one model serves both
    lr.fit(X[500:1000], y[500:1000])
    assert c._cached_model('predict') is not first
    knn = neighbors.KNeighborsClassifier(3).fit(X[:300], y[:300])
    c = classify.Classifier(knn)
    first = c._cached_model('predict')
    assert isinstance(first, classify.KNNModel) and c._cached_model('predict_proba') is first
    knn.fit(X[300:700], y[300:700])
    second = c._cached_model('predict')
    assert second is not first and second.n_train == 400
    np.testing.assert_array_equal(second.train, X[300:700])
    knn.set_params(n_neighbors=5)                              # read at predict time, without a fit
    third = c._cached_model('predict')
    assert third is not second and third.n_neighbors == 5
    assert c._cached_model('predict') is third


def test_header_and_binding_declare_the_new_symbols():
    from nd_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    for s in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, header), s
        assert s in _lib.SYMBOLS
    for i, (py, c) in enumerate((('classify_knn', 'CLASSIFY_KNN'), ('classify_linear', 'CLASSIFY_LINEAR')), 21):
        assert _lib.KERNEL_NAMES[i] == py
        assert re.search(r'#define\s+ND_AMD_KERNEL_%s\s+%d\b' % (c, i), header)
    for name, value in (('CLASSIFY_KNN_MAX_K', _lib.CLASSIFY_KNN_MAX_K), ('CLASSIFY_KNN_TILE', _lib.CLASSIFY_KNN_TILE),
                        ('CLASSIFY_KNN_MAX_FEATURES', _lib.CLASSIFY_KNN_MAX_FEATURES)):
        assert re.search(r'#define\s+ND_AMD_%s\s+%d\b' % (name, value), header)
    assert (_lib.CLASSIFY_KNN_MAX_K, _lib.CLASSIFY_KNN_MAX_FEATURES) == (classify.KNN_MAX_K, classify.KNN_MAX_FEATURES)
    for name, value in _lib.LINKS.items():
        assert re.search(r'#define\s+ND_AMD_LINK_%s\s+%d\b' % (name.upper(), value), header)
    # the scratch check reads every kernel of classify.hip whose name contains this, the new ones included
    assert build.NO_SCRATCH['classify.hip'] in 'classify_knn_kernel'
    assert build.NO_SCRATCH['classify.hip'] in 'classify_linear_kernel'
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s)


def test_bad_arguments_are_refused_without_a_gpu():
    """every refusal happens before the first HIP call (the pointers are never read)"""
    import ctypes
    from nd_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    msg = lambda: L.nd_amd_last_error().decode()
    feat = (vp * 2)(256, 256)
    sz, st = _lib.i64_array([1, 1, 4, 4]), _lib.i64_array([0, 0, 4, 1])
    ws = L.nd_amd_classify_workspace_bytes(2)

    def knn(nfeat=2, dtype=0, ntrain=5, k=3, ncls=2, mean=None, labels=256, wsb=ws, table=feat):
        return L.nd_amd_classify_knn(table, nfeat, dtype, sz, st, vp(256), vp(256), ntrain, k, vp(256), ncls, mean,
                                     None, vp(labels), None, vp(256), wsb, None)

    def linear(nfeat=2, dtype=0, ncoef=3, link=1, output=0, mean=None, out=256, wsb=ws):
        return L.nd_amd_classify_linear(feat, nfeat, dtype, sz, st, vp(256), vp(256), ncoef, vp(256), link, output,
                                        mean, None, vp(out), vp(256), wsb, None)

    for call in (knn, linear):
        assert call(dtype=7) == _lib.EINVAL and 'dtype' in msg()
        assert call(nfeat=0) == _lib.EINVAL and 'features' in msg()
        assert call(wsb=8) == _lib.EWORKSPACE and 'workspace' in msg()
        assert call(mean=vp(256)) == _lib.EINVAL and 'scaler' in msg()
    assert knn(k=0) == _lib.EINVAL and 'k = 0' in msg()
    assert knn(k=6) == _lib.EINVAL and 'k = 6' in msg()
    assert knn(ncls=0) == _lib.EINVAL
    assert knn(labels=0) == _lib.EINVAL and 'no output' in msg()
    assert knn(ntrain=40, k=33) == _lib.EUNSUPPORTED and 'k <= 32' in msg()
    many = (vp * 129)(*[256] * 129)
    assert knn(nfeat=129, table=many, wsb=L.nd_amd_classify_workspace_bytes(129)) == _lib.EUNSUPPORTED
    assert linear(ncoef=0) == _lib.EINVAL and 'model' in msg()
    assert linear(link=3) == _lib.EINVAL and 'link' in msg()
    assert linear(output=3) == _lib.EINVAL
    assert linear(link=0, output=2) == _lib.EINVAL and 'link' in msg()
    assert linear(out=0) == _lib.EINVAL and 'no output' in msg()
