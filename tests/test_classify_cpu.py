"""Classification without a GPU: the numpy restatement (tests/classify_ref.py) against scikit-learn 1.7.2's
recorded output (tests/golden/classify_sklearn.npz) and against live scikit-learn, the packed node format,
the scaler's rounding, row / feature order, label broadcast, the class_mean closed form, the C ABI
declarations and argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest

from nd_amd import classify, xr_lite
from tests import classify_cases as cases, classify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'classify_sklearn.npz')
NEW_SYMBOLS = ('nd_amd_classify_workspace_bytes', 'nd_amd_classify_forest', 'nd_amd_classify_kmeans',
               'nd_amd_classify_select', 'nd_amd_classify_gather', 'nd_amd_class_stats', 'nd_amd_class_fill')
FOREST_CASES = [(n, dt) for n, c in cases.FORESTS.items() for dt in c[4]]
KMEANS_CASES = [(n, dt) for n, c in cases.KMEANS.items() for dt in c[4]]


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def golden_forest(g, name, dtype):
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    model = classify.ForestModel(*[g[key + k] for k in ('feature', 'threshold', 'left', 'right', 'value',
                                                        'tree_offsets', 'classes')])
    sc = (g[key + 'mean'], g[key + 'scale']) if key + 'mean' in g.files else None
    return model, sc, g[key + 'proba'], g[key + 'predict']


def case_X(name, dtype, table):
    n, fdims, _, nt, _ = table[name]
    data, truth = cases.stack(n, dtype, seed=n, nt=nt)
    X, shape = ref.build_X(cases.variables(data), cases.data_dims(fdims), fdims)
    return X, shape, data, truth


def test_golden_is_sklearn_1_7_2(golden):
    assert str(golden['sklearn_version']) == '1.7.2'
    sizes = {n: golden_forest(golden, n, np.float32)[0].n_classes for n in cases.FORESTS}
    assert sizes['rf2'] == 2 and sizes['rf7'] == 7 and sizes['rf11'] > 8


@pytest.mark.parametrize('name,dtype', FOREST_CASES)
def test_forest_restatement_matches_golden(golden, name, dtype):
    model, sc, proba, predict = golden_forest(golden, name, dtype)
    X = case_X(name, dtype, cases.FORESTS)[0]
    assert X.dtype == dtype
    keep = ~np.isnan(X).any(axis=1)
    assert 0 < (~keep).sum() < keep.size
    Xp = X[keep] if sc is None else ref.scale(X[keep], *sc)
    got = ref.forest_proba(Xp, model.feature, model.threshold, model.left, model.right, model.value,
                           model.tree_offsets)
    assert got.tobytes() == proba.tobytes()
    np.testing.assert_array_equal(ref.forest_predict(got, model.classes), predict)
    nodes, roots = model.packed()
    assert ref.packed_proba(Xp, nodes, roots, model.value).tobytes() == proba.tobytes()


@pytest.mark.parametrize('name,dtype', KMEANS_CASES)
def test_kmeans_restatement_matches_golden(golden, name, dtype):
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    X = case_X(name, dtype, cases.KMEANS)[0]
    X = X[~np.isnan(X).any(axis=1)]
    if key + 'mean' in golden.files:
        X = ref.scale(X, golden[key + 'mean'], golden[key + 'scale'])
    centers = golden[key + 'centers']
    gap = ref.kmeans_gap(X, centers)
    ok = gap >= 1e-3
    assert (~ok).mean() <= 0.01
    np.testing.assert_array_equal(ref.kmeans_labels(X, centers)[ok], golden[key + 'labels'][ok])


def _live_forests():
    from sklearn import ensemble, tree
    return [ensemble.RandomForestClassifier(20, random_state=0),
            ensemble.RandomForestClassifier(15, max_depth=12, random_state=1),
            ensemble.ExtraTreesClassifier(10, random_state=2),
            ensemble.RandomForestClassifier(8, max_leaf_nodes=40, random_state=3),
            tree.DecisionTreeClassifier(random_state=4), tree.ExtraTreeClassifier(random_state=5)]


@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_restatement_and_packing_match_live_sklearn(dtype):
    pytest.importorskip('sklearn')
    data, truth = cases.stack(3, dtype, seed=11, nan=False)
    X, shape = ref.build_X(cases.variables(data), ('time', 'y', 'x'))
    y = ref.broadcast_array(truth, shape).reshape(-1)
    for clf in _live_forests():
        clf.fit(X[::3], y[::3])
        model = classify.ForestModel.from_sklearn(clf)
        want = clf.predict_proba(X)
        got = ref.forest_proba(X, model.feature, model.threshold, model.left, model.right, model.value,
                               model.tree_offsets)
        assert got.tobytes() == want.tobytes(), type(clf).__name__
        np.testing.assert_array_equal(ref.forest_predict(got, model.classes), clf.predict(X))
        nodes, roots = model.packed()
        assert ref.packed_proba(X, nodes, roots, model.value).tobytes() == want.tobytes()
        assert model.depth() == max(e.tree_.max_depth for e in getattr(clf, 'estimators_', [clf]))
    # a max_leaf_nodes forest is grown best-first: left children do not follow their parent
    best_first = classify.ForestModel.from_sklearn(_live_forests()[3].fit(X[::3], y[::3]))
    inner = best_first.left >= 0
    local = np.arange(best_first.feature.size) - np.repeat(best_first.tree_offsets[:-1],
                                                           np.diff(best_first.tree_offsets))
    assert np.any(best_first.left[inner] != local[inner] + 1)


def test_features_exactly_on_thresholds():
    """Integer-valued features and a tree whose thresholds are moved onto them: float32 x <= float64 t
    and x <= t32 must agree where x == t, just below and just above."""
    pytest.importorskip('sklearn')
    from sklearn import ensemble
    X, y = cases.integer_stack()
    clf = ensemble.RandomForestClassifier(6, random_state=0).fit(X, y)
    model = classify.ForestModel.from_sklearn(clf)
    inner = model.left >= 0
    thr = model.threshold.copy()
    thr[inner] = np.floor(thr[inner])                    # x.5 -> x: features now lie on thresholds
    odd = np.flatnonzero(inner)[::3]
    thr[odd] = np.nextafter(thr[odd], np.inf)            # and thresholds no float32 represents
    even = np.flatnonzero(inner)[1::3]
    thr[even] = np.nextafter(thr[even], -np.inf)
    moved = classify.ForestModel(model.feature, thr, model.left, model.right, model.value, model.tree_offsets,
                                 model.classes)
    for dt in cases.DTYPES:
        Xd = X.astype(dt)
        on = (Xd[:, None, :] == thr[inner][None, :20, None]).any()
        assert on
        want = ref.forest_proba(Xd, moved.feature, moved.threshold, moved.left, moved.right, moved.value,
                                moved.tree_offsets)
        nodes, roots = moved.packed()
        assert ref.packed_proba(Xd, nodes, roots, moved.value).tobytes() == want.tobytes()
    t32 = np.ascontiguousarray(moved.packed()[0][:, 0]).view(np.float32)[inner]
    assert np.all(t32.astype(np.float64) <= thr[inner])
    assert np.all(np.nextafter(t32, np.float32(np.inf)).astype(np.float64) > thr[inner])


@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_scaler_rounding_matches_sklearn(dtype):
    pytest.importorskip('sklearn')
    from sklearn import preprocessing
    X = case_X('rf3', dtype, cases.FORESTS)[0]
    X = X[~np.isnan(X).any(axis=1)]
    sc = preprocessing.StandardScaler().fit(X[::7])
    want = sc.transform(X)
    got = ref.scale(X, sc.mean_, sc.scale_)
    assert got.dtype == want.dtype == dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_kmeans_restatement_matches_live_sklearn(dtype):
    pytest.importorskip('sklearn')
    from sklearn import cluster
    X = case_X('km3', dtype, cases.KMEANS)[0]
    X = X[~np.isnan(X).any(axis=1)]
    for clf in (cluster.KMeans(5, n_init=2, random_state=0), cluster.MiniBatchKMeans(3, n_init=2, random_state=0)):
        clf.fit(X)
        model = classify.KMeansModel.from_sklearn(clf)
        ok = ref.kmeans_gap(X, model.centers) >= 1e-3
        assert (~ok).mean() <= 0.01
        np.testing.assert_array_equal(ref.kmeans_labels(X, model.centers)[ok], clf.predict(X)[ok])


def test_build_X_row_and_feature_order():
    """test_build_X of the reference, restated: the same X for every order of a variable's dimensions"""
    data, _ = cases.stack(3, np.float32, seed=1)
    nt = cases.NT
    for fdims in ((), ('time',)):
        dd = cases.data_dims(fdims)
        X, shape = ref.build_X(cases.variables(data, 'tyx'), dd, fdims)
        X2, shape2 = ref.build_X(cases.variables(data, 'yxt'), dd, fdims)
        assert shape == shape2 and X.tobytes() == X2.tobytes()
        nv = len(cases.VARS)
        assert X.shape == (np.prod(shape), nv * (nt if fdims else 1))
    X, _ = ref.build_X(cases.variables(data), ('time', 'y', 'x'))
    assert X[5 * cases.NX + 7 + cases.NY * cases.NX, 1] != X[5 * cases.NX + 7 + cases.NY * cases.NX, 1]   # the NaN
    np.testing.assert_array_equal(X[:, 0], data['C11'].reshape(-1))
    Xt, _ = ref.build_X(cases.variables(data), ('y', 'x'), ('time',))
    np.testing.assert_array_equal(Xt[:, 2 * 3 + 1], data['C22'][2].reshape(-1))
    # the layout object orders dimensions as the restatement does
    ds = xr_lite.Dataset({v: (('y', 'x', 'time'), np.transpose(data[v], (1, 2, 0))) for v in cases.VARS},
                         coords={'time': np.arange(nt), 'y': np.arange(cases.NY), 'x': np.arange(cases.NX)})
    assert classify._data_dims(ds, ()) == ('time', 'y', 'x')
    assert classify._data_dims(ds, ['time']) == ('y', 'x')
    bare = xr_lite.Dataset({v: (('y', 'x', 'time'), np.transpose(data[v], (1, 2, 0))) for v in cases.VARS})
    assert classify._data_dims(bare, ()) == ('y', 'x', 'time')


def test_broadcast_and_masks():
    """test_broadcast of the reference, restated"""
    shape = (4, 6, 5)
    lab = np.arange(30.).reshape(6, 5)
    b = ref.broadcast_array(lab, shape)
    assert b.shape == shape and all(np.array_equal(b[i], lab) for i in range(4))
    n = ref.broadcast_named(lab.T, ['x', 'y'], ['time', 'y', 'x'], shape)
    np.testing.assert_array_equal(n, b)
    with pytest.raises(ValueError):
        ref.broadcast_array(np.zeros((7, 5)), shape)
    X = np.arange(12.).reshape(6, 2)
    X[4, 1] = np.nan
    y = np.array([1, 0, np.nan, 2, 3, -1])
    Xs, ys, keep = ref.make_Xy(X, y)
    np.testing.assert_array_equal(keep, [True, False, False, True, False, False])
    np.testing.assert_array_equal(ys, [1, 2])
    np.testing.assert_array_equal(Xs, X[[0, 3]])
    assert ref.make_Xy(X)[2].sum() == 5


def _stats(a, labels, n):
    a = a.reshape(-1).astype(np.float64)
    l = labels.reshape(-1)
    s = [np.nansum(a[l == c]) for c in range(n)]
    k = [int(np.isnan(a[l == c]).sum()) for c in range(n)]
    c = [int((l == c_).sum()) - k_ for c_, k_ in zip(range(n), k)]
    return s, c, k


@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('nans', ['none', 'some', 'class0_all', 'class1_all'])
def test_class_mean_closed_form_is_the_loop(first, nans):
    rng = np.random.default_rng(3)
    labels = rng.integers(first, first + 4, size=(20, 30))
    a = rng.gamma(4.0, 0.25, size=(20, 30)) + labels
    if nans == 'some':
        a[rng.random(a.shape) < 0.1] = np.nan
    elif nans != 'none':
        a[labels == int(nans[5])] = np.nan
        a[3, 4:9] = np.nan
    want = ref.class_mean(a, labels)
    n = len(np.unique(labels))
    fill = classify.class_mean_fill(*_stats(a, labels, n), np.float64)
    cls = np.where((labels >= 0) & (labels < n), labels, n)
    got = np.where(cls < n, fill[cls], np.where(np.isnan(a), fill[n], a))
    np.testing.assert_allclose(got, want, rtol=1e-12, equal_nan=True)
    if first == 1:
        top = labels == n                                  # the last class is no class: untouched
        np.testing.assert_array_equal(got[top & ~np.isnan(a)], a[top & ~np.isnan(a)])


def test_class_mean_refuses_labels_of_another_extent():
    """before any device work: labels shorter than the variable would be read out of bounds"""
    a = np.ones((20, 20, 3), np.float32)
    ds = xr_lite.Dataset({'C11': (('y', 'x', 'time'), a)})
    with pytest.raises(ValueError, match='size 10 along'):
        classify.class_mean(ds, xr_lite.DataArray(np.zeros((10, 10)), ('y', 'x')))
    with pytest.raises(ValueError, match='size 10 along y'):
        classify.class_mean(ds['C11'], xr_lite.DataArray(np.zeros((10, 20)), ('y', 'x')))
    with pytest.raises(ValueError, match='lacks the label dimensions'):
        classify.class_mean(ds, xr_lite.DataArray(np.zeros((20, 4)), ('y', 'band')))
    with pytest.raises(ValueError, match="labels' size 10"):
        classify.class_mean(ds, np.zeros((10, 20)))
    # a dimension of size 1 is squeezed, as make_Xy squeezes it: the refusal is about the sizes, not 'band'
    with pytest.raises(ValueError, match='size 10 along'):
        classify.class_mean(ds, xr_lite.DataArray(np.zeros((1, 10, 10)), ('band', 'y', 'x')))
    # the tensor-level entry refuses strides that reach past the labels, also before any device work
    torch = pytest.importorskip('torch')
    from nd_amd import kernels
    with pytest.raises(ValueError, match='reach element'):
        kernels._label_args(torch.zeros(100, dtype=torch.float64), [10, 1, 0], [20, 20, 3], torch.device('cpu'),
                            'class_stats')
    kernels._label_args(torch.zeros(400, dtype=torch.float64), [20, 1, 0], [20, 20, 3], torch.device('cpu'), 'x')


def test_classifier_model_follows_fits_done_in_place():
    """The Classifier keeps its packed model while the estimator's fitted state is unchanged, and only then:
    warm_start extends estimators_ in place and partial_fit updates cluster_centers_ in place."""
    pytest.importorskip('sklearn')
    from sklearn import cluster, ensemble
    X, y = cases.integer_stack()
    X32 = X.astype(np.float32)

    def proba(model):
        return ref.forest_proba(X32, model.feature, model.threshold, model.left, model.right, model.value,
                                model.tree_offsets)

    for make in (ensemble.RandomForestClassifier, ensemble.ExtraTreesClassifier):
        clf = make(3, warm_start=True, random_state=0).fit(X32, y)
        c = classify.Classifier(clf)
        first = c._cached_model('predict')
        assert c._cached_model('predict_proba') is first and first.n_trees == 3
        held = clf.estimators_
        clf.set_params(n_estimators=8).fit(X32, (y + (X[:, 2] > 3)) % 3)
        assert clf.estimators_ is held                          # scikit-learn extended the list in place
        second = c._cached_model('predict_proba')
        assert second is not first and second.n_trees == 8
        assert proba(second).tobytes() == clf.predict_proba(X32).tobytes() != proba(first).tobytes()
        assert c._cached_model('predict') is second
    km = cluster.MiniBatchKMeans(3, n_init=1, random_state=0).fit(X32[:500])
    c = classify.Classifier(km)
    first = c._cached_model('predict')
    assert c._cached_model('predict') is first
    held = km.cluster_centers_
    km.partial_fit(X32[500:] + 3)
    second = c._cached_model('predict')
    assert second is not first and not np.array_equal(first.centers, second.centers)
    np.testing.assert_array_equal(second.centers, km.cluster_centers_.astype(np.float64))
    assert km.cluster_centers_ is held or True                  # in place in 1.7.2; the key does not rely on it
    # Classifier.fit drops the model whatever the estimator does
    c = classify.Classifier(ensemble.RandomForestClassifier(2, random_state=0).fit(X32, y))
    c._cached_model('predict')
    assert c._model is not None
    c.make_Xy = lambda ds, labels=None: (X32, y)
    c.fit(None)
    assert c._model is None


def test_model_validation_and_unsupported():
    with pytest.raises(ValueError):
        classify.ForestModel([0, -2, -2], [0.5, -2, -2], [1, -1, -1], [5, -1, -1], np.ones((3, 2)), [0, 3], [0, 1])
    with pytest.raises(ValueError):
        classify.ForestModel([0, -2, -2], [0.5, -2, -2], [1, -1, -1], [2, -1, -1], np.ones((3, 2)), [0, 2], [0, 1])
    with pytest.raises(NotImplementedError, match='RandomForestClassifier'):
        classify.ForestModel([0, -2, -2], [0.5, -2, -2], [1, -1, -1], [2, -1, -1], np.ones((3, 2)), [0, 3], ['a', 'b'])
    with pytest.raises(ValueError):
        classify.KMeansModel(np.zeros(3))
    pytest.importorskip('sklearn')
    from sklearn import cluster, ensemble, naive_bayes
    from sklearn.exceptions import NotFittedError
    X, y = cases.integer_stack()
    ds = xr_lite.Dataset({'a': (('y', 'x'), np.ones((4, 5), np.float32))})
    with pytest.raises(NotImplementedError, match='KMeans'):
        classify.Classifier(naive_bayes.GaussianNB().fit(X, y)).predict(ds)
    with pytest.raises(NotImplementedError, match='func'):
        classify.Classifier(ensemble.RandomForestClassifier(2).fit(X, y)).predict(ds, func='predict_log_proba')
    with pytest.raises(NotImplementedError, match='func'):
        classify.Classifier(cluster.KMeans(2, n_init=1).fit(X)).predict(ds, func='transform')
    with pytest.raises(NotImplementedError, match='numeric'):
        classify.Classifier(ensemble.RandomForestClassifier(2).fit(X, np.array(['u', 'v', 'w'])[y])).predict(ds)
    with pytest.raises(NotImplementedError, match='multi-output'):
        classify.Classifier(ensemble.RandomForestClassifier(2).fit(X, np.stack([y, y], 1))).predict(ds)
    with pytest.raises(AttributeError, match='no method'):
        classify.Classifier(cluster.KMeans(2)).predict(ds, func='predict_proba')
    with pytest.raises(NotFittedError):
        classify.Classifier(ensemble.RandomForestClassifier(2)).predict(ds)
    with pytest.raises(ValueError, match='not a valid scoring'):
        classify.Classifier(ensemble.RandomForestClassifier(2)).score(ds, np.ones((4, 5)), method='nope')
    cds = xr_lite.Dataset({'a': (('y', 'x'), np.ones((4, 5), np.complex64))})
    with pytest.raises(TypeError, match='disassemble_complex'):
        classify._Layout(cds, ())


def test_header_and_binding_declare_the_new_symbols():
    from nd_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    for s in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, header), s
        assert s in _lib.SYMBOLS
    for i, (py, c) in enumerate((('classify_forest', 'CLASSIFY_FOREST'), ('classify_kmeans', 'CLASSIFY_KMEANS'),
                                 ('classify_gather', 'CLASSIFY_GATHER'), ('class_mean', 'CLASS_MEAN')), 17):
        assert _lib.KERNEL_NAMES[i] == py
        assert re.search(r'#define\s+ND_AMD_KERNEL_%s\s+%d\b' % (c, i), header)
    assert re.search(r'#define\s+ND_AMD_CLASSIFY_BLOCK_ROWS\s+%d\b' % _lib.CLASSIFY_BLOCK_ROWS, header)
    assert re.search(r'#define\s+ND_AMD_CLASSIFY_MAX_FEATURES\s+%d\b' % _lib.CLASSIFY_MAX_FEATURES, header)
    assert 'classify.hip' in build.NO_SCRATCH
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s)


def test_bad_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call, so it needs no device (the pointers are never read)."""
    from nd_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    msg = lambda: L.nd_amd_last_error().decode()
    feat = (vp * 2)(256, 256)
    sz, st = _lib.i64_array([1, 1, 4, 4]), _lib.i64_array([0, 0, 4, 1])
    neg = _lib.i64_array([0, 0, -4, 1])
    ws = L.nd_amd_classify_workspace_bytes(2)
    assert ws >= 16 and ws % 256 == 0
    assert L.nd_amd_classify_workspace_bytes(0) == 0 and L.nd_amd_classify_workspace_bytes(1025) == 0

    def forest(nfeat=2, dtype=0, sizes=sz, strides=st, ntrees=1, ncls=2, mean=None, labels=256, wsb=ws):
        return L.nd_amd_classify_forest(feat, nfeat, dtype, sizes, strides, vp(256), 3, vp(256), vp(256), ntrees,
                                        vp(256), ncls, mean, None, vp(labels), None, vp(256), wsb, None)

    def kmeans(nfeat=2, dtype=0, sizes=sz, strides=st, k=2, wsb=ws):
        return L.nd_amd_classify_kmeans(feat, nfeat, dtype, sizes, strides, vp(256), k, None, None, vp(256), vp(256),
                                        wsb, None)

    def select(nfeat=2, dtype=0, sizes=sz, strides=st, wsb=ws, count=256):
        return L.nd_amd_classify_select(feat, nfeat, dtype, sizes, strides, None, None, vp(256), vp(256), vp(count),
                                        vp(256), wsb, None)

    def gather(nfeat=2, dtype=0, sizes=sz, strides=st, wsb=ws, X=256):
        return L.nd_amd_classify_gather(feat, nfeat, dtype, sizes, strides, None, None, vp(256), vp(256), vp(X),
                                        None, vp(256), wsb, None)

    for call in (forest, kmeans, select, gather):
        assert call(dtype=7) == _lib.EINVAL and 'dtype' in msg()
        assert call(nfeat=0) == _lib.EINVAL and 'features' in msg()
        assert call(sizes=neg) == _lib.EINVAL and 'shape' in msg()
        assert call(strides=neg) == _lib.EINVAL and 'stride' in msg()
        assert call(wsb=8) == _lib.EWORKSPACE and 'workspace' in msg()
    assert forest(ntrees=0) == _lib.EINVAL and 'forest' in msg()
    assert forest(ncls=0) == _lib.EINVAL and 'forest' in msg()
    assert forest(mean=vp(256)) == _lib.EINVAL and 'scaler' in msg()
    assert forest(labels=0) == _lib.EINVAL and 'no output' in msg()
    assert kmeans(k=0) == _lib.EINVAL and 'k >= 1' in msg()
    assert select(count=0) == _lib.EINVAL and 'count' in msg()
    assert gather(X=0) == _lib.EINVAL and 'X' in msg()

    def stats(dtype=0, sizes=sz, strides=st, n=3, ls=st, out=256):
        return L.nd_amd_class_stats(vp(256), dtype, sizes, strides, vp(256), ls, n, vp(out), vp(256), vp(256), None)

    def fill(dtype=0, sizes=sz, strides=st, n=3, ls=st, out=256):
        return L.nd_amd_class_fill(vp(256), vp(out), dtype, sizes, strides, vp(256), ls, n, vp(256), None)

    for call in (stats, fill):
        assert call(dtype=7) == _lib.EINVAL and 'dtype' in msg()
        assert call(sizes=neg) == _lib.EINVAL and 'shape' in msg()
        assert call(ls=neg) == _lib.EINVAL and 'stride' in msg()
        assert call(ls=None) == _lib.EINVAL and 'label_strides' in msg()
        assert call(n=0) == _lib.EINVAL and 'classes' in msg()
        assert call(out=0) == _lib.EINVAL and 'NULL' in msg()
