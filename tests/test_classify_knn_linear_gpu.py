"""k-nearest-neighbour and linear classification on the device against scikit-learn 1.7.2's recorded output
(tests/golden/classify_knn_linear_sklearn.npz), the numpy restatement (tests/classify_knn_linear_ref.py) and, for
the Classifier interface, the reference's own tests restated.

k-NN: predict_proba and predict equal scikit-learn's on every row whose k-th and (k+1)-th restated distances
differ by at least 1e-6 relative (at most 0.1 % of a case may be left out; tests/test_classify_knn_linear_cpu.py
holds scikit-learn against the restatement to the same condition), and the restatement's on every row.
Linear: decision values within 2 (F + 2) u S of scikit-learn's, probabilities within twice that plus 8 u,
labels equal outside near-ties (at most 1 % of a case)."""
import functools
import os

import numpy as np
import pytest

from nd_amd import classify, xr_lite
from tests import classify_cases as cases, classify_knn_linear_ref as kl, classify_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'classify_knn_linear_sklearn.npz')
DIMS = {'tyx': ('time', 'y', 'x'), 'yxt': ('y', 'x', 'time')}
TILE = 8                                     # ND_AMD_CLASSIFY_KNN_TILE (pinned by the CPU test of the header)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


class Scaler:
    def __init__(self, mean, scale):
        self.mean_, self.scale_ = mean, scale


def dataset(data, layout='tyx', device=None):
    import torch
    first = next(iter(data.values()))
    ds = xr_lite.Dataset(coords={'time': np.arange(first.shape[0]), 'y': np.arange(first.shape[1]),
                                 'x': np.arange(first.shape[2])})
    for name, a in data.items():
        a = a if layout == 'tyx' else np.ascontiguousarray(np.transpose(a, (1, 2, 0)))
        ds[name] = (DIMS[layout], torch.from_numpy(a).to(device) if device is not None else a)
    return ds


def host(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def table(X, device=None):
    """a (rows, features) matrix as a one-variable dataset: features along 'f', rows along 'x'"""
    import torch
    a = np.ascontiguousarray(X.T)
    return xr_lite.Dataset({'a': (('f', 'x'), torch.from_numpy(a).to(device) if device is not None else a)})


# ---- k nearest neighbours: the golden ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def knn_expectation(name, dtype):
    """computed once per recipe and data type, shared by the layouts; read only"""
    g = np.load(GOLDEN)
    k, ncls, fdims, _, _ = kl.KNN[name]
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    data, X, shape, _ = kl.knn_case(name, dtype)
    keep = ~np.isnan(X).any(axis=1)
    sc = Scaler(g[key + 'mean'], g[key + 'scale']) if key + 'mean' in g.files else None
    Xp = X[keep] if sc is None else ref.scale(X[keep], sc.mean_, sc.scale_)
    model = classify.KNNModel(g[key + 'train'], g[key + 'target'], g[key + 'classes'], k)
    proba, gap = kl.knn_proba(Xp, model.train, model.target, k, ncls)
    return dict(data=data, shape=shape, keep=keep, scaler=sc, model=model, proba=proba, gap=gap,
                labels=kl.first_max(proba, model.classes), sk_predict=g[key + 'predict'].astype(np.float64),
                sk_proba=g[key + 'proba'] if key + 'proba' in g.files else None)


@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
@pytest.mark.parametrize('name', list(kl.KNN))
def test_knn_is_sklearn_outside_near_ties(device, name, dtype, layout):
    e = knn_expectation(name, dtype)
    fdims, keep, shape = kl.KNN[name][2], e['keep'], e['shape']
    ok = e['gap'] >= kl.KNN_GAP
    print(name, np.dtype(dtype).name, 'rows left out:', int((~ok).sum()), 'of', ok.size)
    assert (~ok).mean() <= kl.KNN_GAP_ROWS
    for dev in (None, device):
        ds = dataset(e['data'], layout, dev)
        p = classify.predict_knn(ds, e['model'], fdims, 'predict_proba', e['scaler'])
        l = classify.predict_knn(ds, e['model'], fdims, 'predict', e['scaler'])
        assert p.dims == cases.data_dims(fdims) + ('label',) and l.dims == cases.data_dims(fdims)
        assert (dev is None) == isinstance(p.values, np.ndarray)
        pv, lv = host(p.values).reshape(keep.size, -1), host(l.values).reshape(-1)
        assert pv.dtype == np.float64 and lv.dtype == np.float64 and pv.shape[1] == e['model'].n_classes
        assert np.isnan(pv[~keep]).all() and np.isnan(lv[~keep]).all() and 0 < (~keep).sum()
        np.testing.assert_array_equal(lv[keep][ok], e['sk_predict'][ok])
        if e['sk_proba'] is not None:
            assert pv[keep][ok].tobytes() == e['sk_proba'][ok].tobytes()
        # and the definition on every row, near-ties included
        assert pv[keep].tobytes() == e['proba'].tobytes()
        np.testing.assert_array_equal(lv[keep], e['labels'])


# ---- k nearest neighbours: edges, against the restatement ---------------------------------------------
def knn_check(device, X, train, target, classes, k, scaler=None):
    model = classify.KNNModel(train, target, classes, k)
    keep = ~np.isnan(X).any(axis=1)
    Xp = X[keep] if scaler is None else ref.scale(X[keep], scaler.mean_, scaler.scale_)
    want, _ = kl.knn_proba(Xp, model.train, model.target, k, model.n_classes)
    ds = table(X, device)
    p = host(classify.predict_knn(ds, model, ('f',), 'predict_proba', scaler).values)
    l = host(classify.predict_knn(ds, model, ('f',), 'predict', scaler).values)
    assert p.shape == (X.shape[0], model.n_classes) and l.shape == (X.shape[0],)
    assert np.isnan(p[~keep]).all() and np.isnan(l[~keep]).all()
    assert p[keep].tobytes() == want.tobytes()
    np.testing.assert_array_equal(l[keep], kl.first_max(want, model.classes))
    return p, l


def speckle(rng, rows, nfeat, dtype):
    return (rng.gamma(4.0, 0.5, size=(rows, nfeat)) * 2).astype(dtype)


@pytest.mark.parametrize('rows', [1, 63, 65, 4093])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_knn_row_counts_off_the_wave_and_block(device, rows, dtype):
    rng = np.random.default_rng(rows)
    X = speckle(rng, rows, 3, dtype)
    if rows > 1:
        X[rows // 2, 1] = np.nan
    train = speckle(rng, 50, 3, dtype)
    knn_check(device, X, train, rng.integers(0, 3, 50), [1, 2, 3], 3)


# (k = 2, 4, 8, 16 are the last of a neighbour-list size, 3, 5, 9 and 17 the first of the next)
@pytest.mark.parametrize('ntrain,k', [(1, 1), (5, 5), (TILE, TILE), (TILE + 1, 3), (2 * TILE + 1, 16), (100, 32),
                                      (40, 2), (40, 4), (40, 9), (40, 17)])
@pytest.mark.parametrize('nfeat', [3, 9])
def test_knn_training_sizes_around_the_tile(device, ntrain, k, nfeat):
    rng = np.random.default_rng(ntrain * 100 + k)
    X = speckle(rng, 130, nfeat, np.float32)
    train = speckle(rng, ntrain, nfeat, np.float32)
    target = rng.integers(0, 4, ntrain)
    p, _ = knn_check(device, X, train, target, [5, 6, 7, 9], k)
    if k == ntrain:                                        # every sample is a neighbour of every row
        np.testing.assert_array_equal(p, np.broadcast_to(np.bincount(target, minlength=4) / float(k), p.shape))


@pytest.mark.parametrize('dtype', cases.DTYPES)
@pytest.mark.parametrize('nfeat', [3, 8, 9, 128])
def test_knn_feature_counts_at_the_register_and_lds_forms(device, nfeat, dtype):
    """8 features are the last register form, 9 the first in LDS; 128 float64 features leave 64 rows to a block,
    so 300 rows are several blocks of every form"""
    rng = np.random.default_rng(nfeat)
    X = speckle(rng, 300, nfeat, dtype)
    X[7, nfeat - 1] = np.nan
    train = speckle(rng, 40, nfeat, dtype)
    sc = Scaler(np.full(nfeat, 1.5), np.full(nfeat, 0.75))
    knn_check(device, X, train, rng.integers(0, 3, 40), [0, 1, 2], 5)
    knn_check(device, X, ref.scale(train, sc.mean_, sc.scale_), rng.integers(0, 3, 40), [0, 1, 2], 5, sc)


def test_knn_refuses_more_than_128_features(device):
    rng = np.random.default_rng(0)
    model = classify.KNNModel(speckle(rng, 10, 129, np.float32), np.zeros(10, np.int64), [0], 1)
    with pytest.raises(NotImplementedError, match='129 features'):
        classify.predict_knn(table(speckle(rng, 5, 129, np.float32), device), model, ('f',))


@pytest.mark.parametrize('k', [1, 3, 4, 32])
def test_knn_ties_go_to_the_lower_training_index(device, k):
    """integer-valued features: many training samples coincide with each other (under different classes) and
    with queries, so most rows have exact ties at the k-th distance"""
    rng = np.random.default_rng(k)
    train = rng.integers(0, 4, size=(64, 2)).astype(np.float64)
    target = rng.integers(0, 3, 64)
    X = rng.integers(0, 4, size=(200, 2)).astype(np.float64)
    d = kl.knn_d2(X, train)
    assert (d == 0).any(axis=1).mean() > 0.9                               # queries that equal a sample
    if k < 32:
        assert (kl.knn_neighbours(X, train, k)[1] == 0).mean() > 0.5       # exact ties at the k-th place
    knn_check(device, X, train, target, [10, 20, 30], k)
    if k == 1:
        two = np.zeros((2, 2))
        _, l = knn_check(device, two, two, [1, 0], [10, 20], 1)
        np.testing.assert_array_equal(l, [20.0, 20.0])                       # sample 0, of class index 1


# ---- linear: the golden --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_expectation(name, dtype):
    g = np.load(GOLDEN)
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    data, X, shape, _ = kl.linear_case(name, dtype)
    keep = ~np.isnan(X).any(axis=1)
    sc = Scaler(g[key + 'mean'], g[key + 'scale']) if key + 'mean' in g.files else None
    Xp = X[keep] if sc is None else ref.scale(X[keep], sc.mean_, sc.scale_)
    coef, intercept = g[key + 'coef'], g[key + 'intercept']
    model = classify.LinearModel(coef, intercept, g[key + 'classes'], str(g[key + 'link']))
    # scikit-learn's decision values: recorded, or its expression X @ coef_.T + intercept_ (many classes)
    sk = g[key + 'decision'] if key + 'decision' in g.files else Xp @ coef.T + intercept
    s, S = kl.linear_decision(Xp, coef, intercept)
    u_type = np.result_type(Xp.dtype, coef.dtype)
    return dict(data=data, shape=shape, keep=keep, scaler=sc, model=model, s=s,
                bound=kl.linear_bound(S, Xp.shape[1], u_type), u=np.finfo(u_type).eps / 2,
                sk_decision=np.asarray(sk, np.float64).reshape(s.shape), sk_predict=g[key + 'predict'].astype(np.float64),
                sk_proba=g[key + 'proba'] if key + 'proba' in g.files else None)


@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
@pytest.mark.parametrize('name', list(kl.LINEAR))
def test_linear_is_sklearn_within_the_forward_bound(device, name, dtype, layout):
    e = linear_expectation(name, dtype)
    keep, model, bound = e['keep'], e['model'], e['bound']
    sure = kl.linear_margin(e['s']) > 2 * bound.max(axis=1)
    print(name, np.dtype(dtype).name, 'near-ties left out:', int((~sure).sum()), 'of', sure.size)
    assert (~sure).mean() <= kl.LINEAR_TIE_ROWS
    for dev in (None, device):
        ds = dataset(e['data'], layout, dev)
        s = classify.predict_linear(ds, model, (), 'decision_function', e['scaler'])
        l = classify.predict_linear(ds, model, (), 'predict', e['scaler'])
        assert s.dims == ('time', 'y', 'x', 'label') and l.dims == ('time', 'y', 'x')
        assert (dev is None) == isinstance(s.values, np.ndarray)
        sv, lv = host(s.values).reshape(keep.size, -1), host(l.values).reshape(-1)
        assert sv.shape[1] == model.coef.shape[0] and sv.dtype == np.float64
        assert np.isnan(sv[~keep]).all() and np.isnan(lv[~keep]).all() and 0 < (~keep).sum()
        err = np.abs(sv[keep] - e['sk_decision'])
        print(' decision: largest error / bound', np.max(err / bound))
        assert np.all(err <= bound)
        np.testing.assert_array_equal(lv[keep][sure], e['sk_predict'][sure])
        if model.link != 'none':
            p = classify.predict_linear(ds, model, (), 'predict_proba', e['scaler'])
            pv = host(p.values).reshape(keep.size, -1)
            assert pv.shape[1] == model.n_classes and np.isnan(pv[~keep]).all()
            np.testing.assert_allclose(pv[keep].sum(1), 1.0, rtol=1e-14)
            if e['sk_proba'] is not None:
                tol = 2 * bound.max(axis=1, keepdims=True) + 8 * e['u']
                perr = np.abs(pv[keep] - e['sk_proba'])
                print(' proba: largest error / tolerance', np.max(perr / tol))
                assert np.all(perr <= tol)


# ---- linear: edges, against the restatement -----------------------------------------------------------
def linear_check(device, X, coef, intercept, classes, link='softmax', scaler=None):
    """The decision values are the restatement's operations in the restatement's order, each a correctly
    rounded float64 operation (the build does not contract a product into the sum): bit for bit.  The
    probabilities pass through exp, good to an ulp on either side, and a sum of n of them: 4 (n + 4) u."""
    model = classify.LinearModel(coef, intercept, classes, link)
    keep = ~np.isnan(X).any(axis=1)
    Xp = X[keep] if scaler is None else ref.scale(X[keep], scaler.mean_, scaler.scale_)
    s, _ = kl.linear_decision(Xp, model.coef, model.intercept)
    ds = table(X, device)
    got = {f: host(classify.predict_linear(ds, model, ('f',), f, scaler).values)
           for f in ('decision_function', 'predict') + (('predict_proba',) if link != 'none' else ())}
    d, l = got['decision_function'], got['predict']
    assert d.shape == (X.shape[0], model.coef.shape[0]) and l.shape == (X.shape[0],)
    assert np.isnan(d[~keep]).all() and np.isnan(l[~keep]).all()
    assert d[keep].tobytes() == s.tobytes()
    np.testing.assert_array_equal(l[keep], kl.linear_predict(s, model.classes))
    if link != 'none':
        p = got['predict_proba']
        n = model.n_classes
        assert p.shape == (X.shape[0], n) and np.isnan(p[~keep]).all()
        np.testing.assert_allclose(p[keep], kl.linear_proba(s, link), rtol=0, atol=4 * (n + 4) * 2.0 ** -53)
    return got


@pytest.mark.parametrize('rows', [1, 63, 65, 4093])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_linear_row_counts_off_the_wave_and_block(device, rows, dtype):
    rng = np.random.default_rng(rows)
    X = speckle(rng, rows, 3, dtype)
    if rows > 1:
        X[rows // 2, 2] = np.nan
    linear_check(device, X, rng.normal(size=(3, 3)), rng.normal(size=3), [1, 2, 3])


@pytest.mark.parametrize('link', ['softmax', 'ovr', 'none'])
@pytest.mark.parametrize('ncoef', [1, 2, 3, 4, 5, 8, 9, 11])
def test_linear_class_counts_around_the_passes(device, ncoef, link):
    """1 is the binary form; 2 and 4 are the last of an accumulator count, 3 and 5 the first of the next; 8 fills
    one pass, 9 and 11 need a second with the running maximum"""
    rng = np.random.default_rng(ncoef)
    X = speckle(rng, 130, 5, np.float64) - 4.0
    X[3, 0] = np.nan
    classes = np.arange(2 if ncoef == 1 else ncoef) * 2 + 1
    coef, intercept = rng.normal(size=(ncoef, 5)), rng.normal(size=ncoef)
    sc = Scaler(np.full(5, 0.25), np.full(5, 1.5))
    for scaler in (None, sc):
        got = linear_check(device, X, coef, intercept, classes, link, scaler)
    assert len(np.unique(got['predict'][~np.isnan(got['predict'])])) > 1
    # the class that wins last in a second pass, and first in the first
    if ncoef > 1:
        for winner in (0, ncoef - 1):
            b = intercept.copy()
            b[winner] += 1e3
            got = linear_check(device, X, coef, b, classes, link)
            assert set(got['predict'][~np.isnan(got['predict'])]) == {float(classes[winner])}


def test_linear_zero_rows_and_ties_give_the_first_class(device):
    rng = np.random.default_rng(5)
    X = speckle(rng, 100, 4, np.float32) - np.float32(4.0)
    w = rng.normal(size=4)
    # a zero row with a zero intercept: s = 0 exactly, which is not > 0
    got = linear_check(device, X, np.zeros((1, 4)), 0.0, [3, 4], 'ovr')
    np.testing.assert_array_equal(got['predict'], 3.0)
    np.testing.assert_array_equal(got['predict_proba'], 0.5)
    # rows 1 and 2 are the same and beat the zero row 0 wherever x.w > 0: the tie goes to row 1
    coef = np.stack([np.zeros(4), w, w, -w])
    got = linear_check(device, X, coef, np.zeros(4), [10, 11, 12, 13])
    s = X.astype(np.float64) @ w
    assert (s > 0).any() and (s < 0).any()
    np.testing.assert_array_equal(got['predict'], np.where(s > 0, 11.0, np.where(s < 0, 13.0, 10.0)))
    # every row equal: class 0; also across the passes of a model with many rows
    for n in (3, 11):
        got = linear_check(device, X, np.repeat(w[None], n, 0), np.full(n, 0.5), np.arange(n) + 1)
        np.testing.assert_array_equal(got['predict'], 1.0)
        np.testing.assert_allclose(got['predict_proba'], 1.0 / n, rtol=1e-15)


# ---- the Classifier interface: the reference's tests restated -------------------------------------------
def mock_classes(dims=('y', 'x', 'time'), shape=(30, 40, 3), nclasses=3, seed=0, device=None, dtype=np.float64):
    """well separated classes in vertical stripes: every variable of a pixel lies near its class index"""
    import torch
    rng = np.random.default_rng(seed)
    ny, nx = shape[dims.index('y')], shape[dims.index('x')]
    labels = np.repeat((np.arange(nx) * nclasses // nx + 1)[None], ny, 0)
    idx = tuple(slice(None) if d in ('y', 'x') else None for d in dims)
    lab_full = np.transpose(labels, (0, 1) if dims.index('y') < dims.index('x') else (1, 0))[idx]
    ds = xr_lite.Dataset(coords={d: np.arange(n) for d, n in zip(dims, shape)})
    for v in ('C11', 'C22'):
        a = (lab_full + rng.normal(0, 0.05, size=shape)).astype(dtype)
        ds[v] = (dims, torch.from_numpy(a).to(device) if device is not None else a)
    return ds, xr_lite.DataArray(labels, ('y', 'x'))


@pytest.mark.parametrize('on_device', [False, True])
@pytest.mark.parametrize('kind', ['Dataset', 'DataArray'])
def test_classifier_knn_fit_predict_score(device, kind, on_device):
    """nd/tests/test_classifier.py::test_classifier with KNeighborsClassifier(3): fitted on 10 % of the pixels,
    every pixel is predicted right"""
    pytest.importorskip('sklearn')
    from sklearn.neighbors import KNeighborsClassifier
    ds, labels = mock_classes(device=device if on_device else None)
    if kind == 'DataArray':
        ds = ds['C11']
    rng = np.random.default_rng(1)
    train = np.where(rng.random(labels.shape) < 0.1, labels.values, 0)
    c = classify.Classifier(KNeighborsClassifier(3))
    pred = c.fit(ds, xr_lite.DataArray(train, ('y', 'x'))).predict(ds)
    assert pred.dims == ('y', 'x', 'time')
    pv = host(pred.values)
    full = np.broadcast_to(labels.values[..., None], pv.shape)
    np.testing.assert_array_equal(pv, full)                                                   # 100 % accuracy
    c2 = classify.Classifier(KNeighborsClassifier(3))
    np.testing.assert_array_equal(host(c2.fit_predict(ds, train).values), pv)
    assert c.score(ds, labels) == 1.0
    p = host(c.predict(ds, func='predict_proba').values)
    assert p.shape == pv.shape + (3,) and set(np.unique(p)) <= {0.0, 1 / 3, 2 / 3, 1.0}
    np.testing.assert_array_equal(p.argmax(-1) + 1, pv)
    # time as a feature dimension, scaled
    c3 = classify.Classifier(KNeighborsClassifier(3), feature_dims=['time'], scale=True)
    p3 = c3.fit_predict(ds, train)
    assert p3.dims == ('y', 'x')
    np.testing.assert_array_equal(host(p3.values), labels.values)


@pytest.mark.parametrize('on_device', [False, True])
def test_classifier_logistic_predict_proba(device, on_device):
    """nd/tests/test_classifier.py::test_predict_proba with LogisticRegression()"""
    pytest.importorskip('sklearn')
    from sklearn.linear_model import LogisticRegression
    ds, labels = mock_classes(device=device if on_device else None)
    c = classify.Classifier(LogisticRegression())
    c.fit(ds, labels)
    proba = c.predict(ds, func='predict_proba')
    assert proba.dims == ('y', 'x', 'time', 'label')
    pv = host(proba.values)
    assert pv.shape == (30, 40, 3, 3) and (pv >= 0).all() and (pv <= 1).all()
    np.testing.assert_array_equal(host(c.predict(ds).values), pv.argmax(-1) + 1)
    np.testing.assert_array_equal(host(c.fit_predict(ds, labels).values), pv.argmax(-1) + 1)
    assert c.score(ds, labels) == (host(c.predict(ds).values) == labels.values[..., None]).mean() > 0.95
    # against scikit-learn on the reference's matrix
    variables = [(('y', 'x', 'time'), host(ds[v].values)) for v in ('C11', 'C22')]
    X, _ = ref.build_X(variables, ('y', 'x', 'time'))
    np.testing.assert_allclose(pv.reshape(-1, 3), c.clf.predict_proba(X), rtol=0, atol=1e-12)


def test_classifier_reuses_the_packed_model(device):
    pytest.importorskip('sklearn')
    from sklearn.linear_model import SGDClassifier
    from sklearn.neighbors import KNeighborsClassifier
    ds, labels = mock_classes(device=device)
    c = classify.Classifier(KNeighborsClassifier(3)).fit(ds, labels)
    a = c.predict(ds)
    first = c._model[2]
    c.predict(ds, func='predict_proba')
    assert isinstance(first, classify.KNNModel) and c._model[2] is first and len(first._device) == 1
    c.fit(ds, labels)
    np.testing.assert_array_equal(host(c.predict(ds).values), host(a.values))
    assert c._model[2] is not first                              # a new fit is a new model
    sgd = SGDClassifier(random_state=0)
    c = classify.Classifier(sgd).fit(ds, labels)
    c.predict(ds)
    first = c._model[2]
    c.predict(ds)
    assert isinstance(first, classify.LinearModel) and c._model[2] is first and len(first._device) == 1
    Xt, yt = c.make_Xy(ds, labels)
    sgd.partial_fit(Xt[::2] * 1.5, yt[::2])
    got = host(c.predict(ds).values).reshape(-1)
    assert c._model[2] is not first
    variables = [(('y', 'x', 'time'), host(ds[v].values)) for v in ('C11', 'C22')]
    X, _ = ref.build_X(variables, ('y', 'x', 'time'))
    s, S = kl.linear_decision(X, sgd.coef_, sgd.intercept_)
    sure = kl.linear_margin(s) > 2 * kl.linear_bound(S, 2, np.float64).max(axis=1)
    assert sure.mean() >= 0.99
    np.testing.assert_array_equal(got[sure], kl.linear_predict(s, sgd.classes_)[sure])
