"""Classification on the device against scikit-learn 1.7.2's recorded output (tests/golden/classify_sklearn.npz),
the numpy restatement (tests/classify_ref.py) and, for the Classifier interface, the reference's own tests
restated.  Forest probabilities must be bit-equal and labels equal; k-means labels equal outside near-ties;
class_mean within 1e-5 relative (the package's bound for float32 reductions)."""
import os

import numpy as np
import pytest

from nd_amd import classify, xr_lite
from tests import classify_cases as cases, classify_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'classify_sklearn.npz')
FOREST_CASES = [(n, dt) for n, c in cases.FORESTS.items() for dt in c[4]]
KMEANS_CASES = [(n, dt) for n, c in cases.KMEANS.items() for dt in c[4]]
DIMS = {'tyx': ('time', 'y', 'x'), 'yxt': ('y', 'x', 'time')}


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


class Scaler:
    def __init__(self, mean, scale):
        self.mean_, self.scale_ = mean, scale


def dataset(data, layout='tyx', device=None, coords=True):
    """the stack as an xr_lite Dataset in one of the two layouts, on the host or on the device"""
    import torch
    first = next(iter(data.values()))
    c = {'time': np.arange(first.shape[0]), 'y': np.arange(first.shape[1]), 'x': np.arange(first.shape[2])}
    ds = xr_lite.Dataset(coords=c if coords else None)
    for name, a in data.items():
        a = a if layout == 'tyx' else np.ascontiguousarray(np.transpose(a, (1, 2, 0)))
        ds[name] = (DIMS[layout], torch.from_numpy(a).to(device) if device is not None else a)
    return ds


def host(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def golden_forest(g, name, dtype):
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    model = classify.ForestModel(*[g[key + k] for k in ('feature', 'threshold', 'left', 'right', 'value',
                                                        'tree_offsets', 'classes')])
    sc = Scaler(g[key + 'mean'], g[key + 'scale']) if key + 'mean' in g.files else None
    return model, sc, g[key + 'proba'], g[key + 'predict']


@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
@pytest.mark.parametrize('name', list(cases.FORESTS))
def test_forest_is_sklearn_bit_for_bit(golden, device, name, dtype, layout):
    """Every golden model on float32 and on float64 data.  Where scikit-learn's output for that data type is
    recorded it is the expectation; for the models recorded for float32 only, the float64 expectation is the
    restatement's walk of the same model over the float64 stack, which tests/test_classify_cpu.py pins bit for
    bit to scikit-learn for both data types."""
    ncls, fdims, _, nt, recorded = cases.FORESTS[name]
    model, sc, proba, predict = golden_forest(golden, name, dtype if dtype in recorded else np.float32)
    data, _ = cases.stack(ncls, dtype, seed=ncls, nt=nt)
    X, shape = ref.build_X(cases.variables(data), cases.data_dims(fdims), fdims)
    assert X.dtype == dtype
    keep = ~np.isnan(X).any(axis=1)
    if dtype not in recorded:
        Xp = X[keep] if sc is None else ref.scale(X[keep], sc.mean_, sc.scale_)
        proba = ref.forest_proba(Xp, model.feature, model.threshold, model.left, model.right, model.value,
                                 model.tree_offsets)
        predict = ref.forest_predict(proba, model.classes)
    want_p = ref.masked(proba, keep).reshape(shape + (ncls,))
    want_l = ref.masked(predict.astype(np.float64), keep).reshape(shape)
    for dev in (None, device):
        ds = dataset(data, layout, dev)
        p = classify.predict_forest(ds, model, fdims, 'predict_proba', sc)
        l = classify.predict_forest(ds, model, fdims, 'predict', sc)
        assert p.dims == cases.data_dims(fdims) + ('label',) and l.dims == cases.data_dims(fdims)
        assert (dev is None) == isinstance(p.values, np.ndarray)
        pv, lv = host(p.values), host(l.values)
        assert pv.dtype == np.float64 and lv.dtype == np.float64
        assert np.isnan(pv[~keep.reshape(shape)]).all() and np.isnan(lv[~keep.reshape(shape)]).all()
        assert pv.tobytes() == want_p.tobytes(), np.nanmax(np.abs(pv - want_p))
        np.testing.assert_array_equal(lv, want_l)


def test_forest_single_dataarray_and_integers(golden, device):
    import torch
    model, _, _, _ = golden_forest(golden, 'tree3', np.float32)
    rng = np.random.default_rng(0)
    a = rng.integers(0, 5, size=(3, 9, 11)).astype(np.int16)
    one = classify.ForestModel(np.where(model.feature >= 0, 0, model.feature), model.threshold, model.left,
                               model.right, model.value, model.tree_offsets, model.classes, n_features=1)
    X = a.reshape(-1, 1).astype(np.float64)
    want = ref.forest_proba(X, one.feature, one.threshold, one.left, one.right, one.value, one.tree_offsets)
    da = xr_lite.DataArray(torch.from_numpy(a).to(device), ('time', 'y', 'x'))
    got = classify.predict_forest(da, one, func='predict_proba')
    assert host(got.values).tobytes() == want.reshape(3, 9, 11, -1).tobytes()


@pytest.mark.parametrize('rows', [1, 63, 65, 4093])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_forest_row_counts_off_the_wave_and_block(golden, device, rows, dtype):
    import torch
    model, _, _, _ = golden_forest(golden, 'rf3', np.float32)
    rng = np.random.default_rng(rows)
    data = {v: (rng.gamma(4.0, 0.5, size=(1, 1, rows)) * 2).astype(dtype) for v in cases.VARS}
    if rows > 1:
        data['C22'][0, 0, rows // 2] = np.nan
    X, shape = ref.build_X(cases.variables(data), ('time', 'y', 'x'))
    keep = ~np.isnan(X).any(axis=1)
    want = ref.masked(ref.forest_proba(X[keep], model.feature, model.threshold, model.left, model.right,
                                       model.value, model.tree_offsets), keep)
    got = classify.predict_forest(dataset(data, 'tyx', device), model, func='predict_proba')
    assert host(got.values).reshape(rows, -1).tobytes() == want.tobytes()


def test_feature_on_threshold_and_scaler_one_ulp(device):
    """features lying exactly on thresholds, and thresholds one ulp off, go the way scikit-learn goes"""
    import torch
    rng = np.random.default_rng(4)
    for dtype in cases.DTYPES:
        x = rng.integers(0, 6, size=(1, 40, 50)).astype(dtype)
        thr = np.array([3.0, np.nextafter(2.0, 3.0), np.nextafter(np.float32(5.0), np.float32(0)), -2, -2, -2, -2],
                       np.float64)
        model = classify.ForestModel([0, 0, 0, -2, -2, -2, -2], thr, [1, 3, 5, -1, -1, -1, -1],
                                     [2, 4, 6, -1, -1, -1, -1], np.eye(7)[:, 3:], [0, 7], [10, 20, 30, 40])
        X = x.reshape(-1, 1)
        want = ref.forest_proba(X, model.feature, model.threshold, model.left, model.right, model.value,
                                model.tree_offsets)
        assert len(np.unique(np.argmax(want, 1))) == 4
        da = xr_lite.DataArray(torch.from_numpy(x).to(device), ('time', 'y', 'x'))
        got = classify.predict_forest(da, model, func='predict_proba')
        assert host(got.values).reshape(-1, 4).tobytes() == want.tobytes()
        # scaled: x - mean lands on / next to the threshold after rounding in the data type
        sc = Scaler(np.array([1.0 / 3.0]), np.array([0.7]))
        Xs = ref.scale(X, sc.mean_, sc.scale_)
        t = np.sort(np.unique(Xs.astype(np.float32)).astype(np.float64))
        model2 = classify.ForestModel([0, 0, 0, -2, -2, -2, -2], [t[2], t[1], np.nextafter(t[4], -np.inf), -2, -2, -2, -2],
                                      [1, 3, 5, -1, -1, -1, -1], [2, 4, 6, -1, -1, -1, -1], np.eye(7)[:, 3:],
                                      [0, 7], [10, 20, 30, 40])
        want = ref.forest_proba(Xs, model2.feature, model2.threshold, model2.left, model2.right, model2.value,
                                model2.tree_offsets)
        got = classify.predict_forest(da, model2, func='predict_proba', scaler=sc)
        assert host(got.values).reshape(-1, 4).tobytes() == want.tobytes()


@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('name,dtype', KMEANS_CASES)
def test_kmeans_labels(golden, device, name, dtype, layout):
    k, fdims, _, nt, _ = cases.KMEANS[name]
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    centers = golden[key + 'centers']
    sc = Scaler(golden[key + 'mean'], golden[key + 'scale']) if key + 'mean' in golden.files else None
    data, _ = cases.stack(k, dtype, seed=k, nt=nt)
    X, shape = ref.build_X(cases.variables(data), cases.data_dims(fdims), fdims)
    keep = ~np.isnan(X).any(axis=1)
    Xp = X[keep] if sc is None else ref.scale(X[keep], sc.mean_, sc.scale_)
    gap = ref.kmeans_gap(Xp, centers)
    want = ref.kmeans_labels(Xp, centers)
    model = classify.KMeansModel(centers)
    for dev in (None, device):
        got = classify.predict_kmeans(dataset(data, layout, dev), model, fdims, sc)
        lv = host(got.values).reshape(-1)
        assert np.isnan(lv[~keep]).all()
        ok = gap >= 1e-12
        print(name, 'left out of the float64 comparison:', (~ok).mean(), 'of the recorded one:', (gap < 1e-3).mean())
        assert (~ok).mean() <= 1e-4
        np.testing.assert_array_equal(lv[keep][ok], want[ok])
        ok = gap >= 1e-3
        assert (~ok).mean() <= 1e-2
        np.testing.assert_array_equal(lv[keep][ok], golden[key + 'labels'][ok])


def test_kmeans_duplicate_centres_give_the_lower_index(device):
    data, _ = cases.stack(3, np.float32, seed=3, nan=False)
    c = np.array([[9., 9., 9.], [1., 2., .5], [1., 2., .5], [3., 2., 1.5], [3., 2., 1.5]])
    got = host(classify.predict_kmeans(dataset(data, 'tyx', device), classify.KMeansModel(c)).values)
    seen = set(np.unique(got))
    assert not seen & {2.0, 4.0} and {1.0, 3.0} & seen
    X, _ = ref.build_X(cases.variables(data), ('time', 'y', 'x'))
    np.testing.assert_array_equal(got.reshape(-1), ref.kmeans_labels(X, c))


@pytest.mark.parametrize('scale', [False, True])
@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_kmeans_six_features(device, dtype, layout, scale):
    """two dates as features: 6 features, the 5-to-8-feature register form; against the float64 restatement"""
    data, _ = cases.stack(3, dtype, seed=9, nt=2)
    X, shape = ref.build_X(cases.variables(data), ('y', 'x'), ('time',))
    assert X.shape[1] == 6
    keep = ~np.isnan(X).any(axis=1)
    sc = Scaler(np.nanmean(X, 0).astype(np.float64), np.nanstd(X, 0).astype(np.float64)) if scale else None
    Xp = X[keep] if sc is None else ref.scale(X[keep], sc.mean_, sc.scale_)
    centers = Xp[[5, 200, 400, 600]].astype(np.float64) * 1.0625
    ok = ref.kmeans_gap(Xp, centers) >= 1e-12
    assert (~ok).mean() <= 1e-4
    got = classify.predict_kmeans(dataset(data, layout, device), classify.KMeansModel(centers), ('time',), sc)
    lv = host(got.values).reshape(-1)
    assert got.dims == ('y', 'x') and np.isnan(lv[~keep]).all()
    np.testing.assert_array_equal(lv[keep][ok], ref.kmeans_labels(Xp, centers)[ok])


def many_feature_case(dtype, nt, scale):
    """nt dates of the three variables as 3 nt features -> (data, keep, shape, scaler, the kept rows as a model
    sees them)"""
    data, _ = cases.stack(3, dtype, seed=9, nt=nt)
    X, shape = ref.build_X(cases.variables(data), ('y', 'x'), ('time',))
    assert X.shape[1] == 3 * nt and X.dtype == dtype
    keep = ~np.isnan(X).any(axis=1)
    assert 0 < keep.sum() < keep.size
    sc = Scaler(np.nanmean(X, 0).astype(np.float64), np.nanstd(X, 0).astype(np.float64)) if scale else None
    return data, keep, shape, sc, (X[keep] if sc is None else ref.scale(X[keep], sc.mean_, sc.scale_))


def check_array_forest(device, data, layout, keep, shape, sc, Xp):
    """a forest of arrays that reads every feature, thresholds on the (scaled) data's own values: probabilities
    bit for bit, labels equal, NaN on the masked rows"""
    model = classify.ForestModel(*cases.array_forest(Xp, 4, seed=Xp.shape[1]))
    assert set(model.feature[model.feature >= 0]) == set(range(Xp.shape[1]))
    proba = ref.forest_proba(Xp, model.feature, model.threshold, model.left, model.right, model.value,
                             model.tree_offsets)
    assert len(np.unique(np.argmax(proba, 1))) == 4
    want_p = ref.masked(proba, keep)
    want_l = ref.masked(ref.forest_predict(proba, model.classes), keep)
    ds = dataset(data, layout, device)
    p = classify.predict_forest(ds, model, ('time',), 'predict_proba', sc)
    l = classify.predict_forest(ds, model, ('time',), 'predict', sc)
    assert p.dims == ('y', 'x', 'label') and l.dims == ('y', 'x')
    pv, lv = host(p.values).reshape(keep.size, -1), host(l.values).reshape(-1)
    assert np.isnan(pv[~keep]).all() and np.isnan(lv[~keep]).all()
    assert pv[keep].tobytes() == want_p[keep].tobytes()
    np.testing.assert_array_equal(lv, want_l)


@pytest.mark.parametrize('scale', [False, True])
@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_forest_six_features(device, dtype, layout, scale):
    """two dates as features: 6 features, the 5-to-8-feature register form of the forest walk"""
    data, keep, shape, sc, Xp = many_feature_case(dtype, 2, scale)
    check_array_forest(device, data, layout, keep, shape, sc, Xp)


@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_twelve_features_with_a_scaler(device, dtype, layout):
    """four dates as features with a scaler: the scaler on the form that reads its features from memory, for the
    forest (bit for bit) and for k-means (labels equal outside the 1e-12 near-ties, at most 1 row in 10^4)"""
    data, keep, shape, sc, Xp = many_feature_case(dtype, 4, True)
    check_array_forest(device, data, layout, keep, shape, sc, Xp)
    centers = Xp[[5, 200, 400, 600, 700]].astype(np.float64) * 1.0625
    ok = ref.kmeans_gap(Xp, centers) >= 1e-12
    assert (~ok).mean() <= 1e-4
    got = classify.predict_kmeans(dataset(data, layout, device), classify.KMeansModel(centers), ('time',), sc)
    lv = host(got.values).reshape(-1)
    assert got.dims == ('y', 'x') and np.isnan(lv[~keep]).all()
    np.testing.assert_array_equal(lv[keep][ok], ref.kmeans_labels(Xp, centers)[ok])
    assert len(np.unique(lv[keep])) == 5


@pytest.mark.parametrize('dtype', cases.DTYPES)
@pytest.mark.parametrize('nfeat,ncls', [(4, 5), (5, 8), (8, 9), (9, 2), (3, 3)])
def test_feature_and_class_counts_at_the_bounds_of_the_forms(device, nfeat, ncls, dtype):
    """4 features are the last of the first register form, 5 the first and 8 the last of the second, 9 the first
    read from memory; 2, 4 and 8 classes are the last of a class-count form and 3, 5 and 9 the first of the next
    (4 classes: check_array_forest).  One variable per feature: the forest bit for bit against the restatement,
    k-means labels equal outside the 1e-12 near-ties."""
    from tests import kmeans_fit_ref as kf
    data = kf.stack(nfeat, (1, 12, 25), 3, dtype, seed=nfeat, nan=False)
    data['v00'][0, 5, 7] = np.nan
    X, shape = ref.build_X(kf.variables(data), ('time', 'y', 'x'))
    assert X.shape == (300, nfeat) and X.dtype == dtype
    keep = ~np.isnan(X).any(axis=1)
    Xp = X[keep]
    model = classify.ForestModel(*cases.array_forest(Xp, ncls, seed=nfeat))
    assert set(model.feature[model.feature >= 0]) == set(range(nfeat))
    proba = ref.forest_proba(Xp, model.feature, model.threshold, model.left, model.right, model.value,
                             model.tree_offsets)
    ds = dataset(data, 'tyx', device)
    pv = host(classify.predict_forest(ds, model, (), 'predict_proba').values).reshape(keep.size, -1)
    lv = host(classify.predict_forest(ds, model, (), 'predict').values).reshape(-1)
    assert pv.shape[1] == ncls and np.isnan(pv[~keep]).all() and np.isnan(lv[~keep]).all()
    assert pv[keep].tobytes() == proba.tobytes()
    np.testing.assert_array_equal(lv[keep], ref.forest_predict(proba, model.classes))
    centers = Xp[[5, 100, 200, 290]].astype(np.float64) * 1.0625
    ok = ref.kmeans_gap(Xp, centers) >= 1e-12
    assert (~ok).mean() <= 1e-4
    got = host(classify.predict_kmeans(ds, classify.KMeansModel(centers)).values).reshape(-1)
    assert np.isnan(got[~keep]).all()
    np.testing.assert_array_equal(got[keep][ok], ref.kmeans_labels(Xp, centers)[ok])


def test_classifier_reuses_the_packed_model(device):
    pytest.importorskip('sklearn')
    from sklearn.ensemble import RandomForestClassifier
    ds, labels = mock_classes(device=device)
    c = classify.Classifier(RandomForestClassifier(5, random_state=0)).fit(ds, labels)
    a = c.predict(ds)
    first = c._model[2]
    c.predict(ds, func='predict_proba')
    assert c._model[2] is first and len(first._device) == 1      # no re-packing, one upload
    c.fit(ds, labels)
    c.predict(ds, func='predict_proba')
    assert c._model[2] is not first                              # a new fit is a new model
    np.testing.assert_array_equal(host(a.values), host(c.predict(ds).values))
    # fits that change the estimator in place: warm_start with more trees, partial_fit
    variables = [(('y', 'x', 'time'), host(ds[v].values)) for v in ('C11', 'C22')]
    X, _ = ref.build_X(variables, ('y', 'x', 'time'))
    clf = RandomForestClassifier(3, warm_start=True, random_state=0)
    c = classify.Classifier(clf).fit(ds, labels)
    p3 = host(c.predict(ds, func='predict_proba').values)
    assert p3.reshape(X.shape[0], -1).tobytes() == clf.predict_proba(X).tobytes()
    Xt, yt = c.make_Xy(ds, labels)
    clf.set_params(n_estimators=8).fit(Xt, yt)
    p8 = host(c.predict(ds, func='predict_proba').values)
    assert p8.reshape(X.shape[0], -1).tobytes() == clf.predict_proba(X).tobytes()
    from sklearn.cluster import MiniBatchKMeans
    km = MiniBatchKMeans(3, n_init=1, random_state=0)
    c = classify.Classifier(km).fit(ds)
    c.predict(ds)
    km.partial_fit(Xt[::2] * 1.5)
    got = host(c.predict(ds).values).reshape(-1)
    centers = km.cluster_centers_.astype(np.float64)
    ok = ref.kmeans_gap(X, centers) >= 1e-12
    assert (~ok).mean() <= 1e-4
    np.testing.assert_array_equal(got[ok], ref.kmeans_labels(X, centers)[ok])


# ---- the Classifier interface: the reference's tests restated --------------------------------------------
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
@pytest.mark.parametrize('dims', [('y', 'x', 'time'), ('time', 'y', 'x')])
def test_classifier_fit_predict_score(device, dims, on_device):
    pytest.importorskip('sklearn')
    from sklearn.ensemble import RandomForestClassifier
    shape = (30, 40, 3) if dims[0] == 'y' else (3, 30, 40)
    ds, labels = mock_classes(dims, shape, device=device if on_device else None)
    rng = np.random.default_rng(1)
    train = np.where(rng.random(labels.shape) < 0.1, labels.values, 0)            # 10 % training pixels
    c = classify.Classifier(RandomForestClassifier(n_estimators=20, random_state=0))
    pred = c.fit(ds, xr_lite.DataArray(train, ('y', 'x'))).predict(ds)
    data_dims = dims                       # rows follow the order of the dimension coordinates
    assert pred.dims == data_dims
    pv = host(pred.values)
    full = np.broadcast_to(labels.values[tuple(slice(None) if d in ('y', 'x') else None for d in dims)], pv.shape)
    np.testing.assert_array_equal(pv, full)                                                   # 100 % accuracy
    c2 = classify.Classifier(RandomForestClassifier(n_estimators=20, random_state=0))
    np.testing.assert_array_equal(host(c2.fit_predict(ds, train).values), pv)                 # numpy labels
    assert c.score(ds, labels) == (pv == full).mean() == 1.0
    # against scikit-learn itself on the reference's matrix
    variables = [(dims, host(ds[v].values)) for v in ('C11', 'C22')]
    X, _ = ref.build_X(variables, data_dims)
    assert host(c.predict(ds, func='predict_proba').values).reshape(X.shape[0], -1).tobytes() == \
        c.clf.predict_proba(X).tobytes()
    # time as a feature dimension, scaled
    c3 = classify.Classifier(RandomForestClassifier(n_estimators=10, random_state=0), feature_dims=['time'], scale=True)
    p3 = c3.fit_predict(ds, train)
    assert p3.dims == ('y', 'x')
    np.testing.assert_array_equal(host(p3.values), labels.values)
    X3, _ = ref.build_X(variables, ('y', 'x'), ('time',))
    assert host(c3.predict(ds, func='predict_proba').values).reshape(X3.shape[0], -1).tobytes() == \
        c3.clf.predict_proba(c3._scaler.transform(X3)).tobytes()


def test_classifier_kmeans_and_errors(device):
    pytest.importorskip('sklearn')
    from sklearn.cluster import KMeans
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.exceptions import NotFittedError
    from sklearn.naive_bayes import GaussianNB
    ds, labels = mock_classes(device=device)
    c = classify.Classifier(KMeans(3, n_init=2, random_state=0))
    pv = host(c.fit_predict(ds).values)
    assert pv.shape == (30, 40, 3) and len(np.unique(pv)) == 3
    for k in range(3):
        assert len(np.unique(pv[labels.values == k + 1])) == 1
    with pytest.raises(NotFittedError):
        classify.Classifier(RandomForestClassifier()).predict(ds)
    with pytest.raises(ValueError, match='not a valid scoring'):
        c.score(ds, labels, method='invalid')
    X, y = c.make_Xy(ds, labels)
    with pytest.raises(NotImplementedError):
        classify.Classifier(GaussianNB().fit(X, y)).predict(ds)
    with pytest.raises(NotImplementedError):
        classify.Classifier(RandomForestClassifier(3).fit(X, y)).predict(ds, func='predict_log_proba')
    with pytest.raises(NotImplementedError):
        classify.Classifier(RandomForestClassifier(3).fit(X, np.array(['a', 'b', 'c', 'd'])[y])).predict(ds)
    with pytest.raises(AttributeError):
        c.predict(ds, func='predict_proba')


@pytest.mark.parametrize('fdims', [(), ('time',)])
@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_make_Xy_row_for_row(device, dtype, layout, fdims):
    data, truth = cases.stack(3, dtype, seed=5)
    lab = cases.training_labels(truth, seed=5)
    X, shape = ref.build_X(cases.variables(data), cases.data_dims(fdims), fdims)
    wX, wy, keep = ref.make_Xy(X, ref.broadcast_array(lab, shape).reshape(-1))
    assert 0 < keep.sum() < keep.size
    for dev in (None, device):
        ds = dataset(data, layout, dev)
        c = classify.Classifier(None, feature_dims=list(fdims))
        for labels in (lab, xr_lite.DataArray(lab.T.copy(), ('x', 'y')), lab[None]):
            gX, gy = c.make_Xy(ds, labels)
            assert isinstance(gX, np.ndarray) and gX.dtype == dtype and gX.tobytes() == wX.tobytes()
            np.testing.assert_array_equal(gy, wy)
        gX, gy = c.make_Xy(ds)
        assert gy is None and gX.tobytes() == X[~np.isnan(X).any(axis=1)].tobytes()
    if not fdims:
        # a dataset without coordinates: rows follow the first variable's dimension order
        bare = dataset(data, 'yxt', device, coords=False)
        Xb, shapeb = ref.build_X(cases.variables(data, 'yxt'), ('y', 'x', 'time'))
        wXb, _, _ = ref.make_Xy(Xb, ref.broadcast_array(lab, shapeb).reshape(-1))
        assert classify.Classifier(None).make_Xy(bare, lab)[0].tobytes() == wXb.tobytes()


def test_make_Xy_many_blocks(device):
    """more rows than one scan chunk per thread: 300 blocks of 1024 rows, sparse labels"""
    import torch
    rng = np.random.default_rng(8)
    a = rng.random((3, 320, 320)).astype(np.float32)
    a[rng.random(a.shape) < 0.01] = np.nan
    lab = np.where(rng.random((320, 320)) < 0.05, 2.0, 0.0)
    ds = xr_lite.Dataset({'a': (('time', 'y', 'x'), torch.from_numpy(a).to(device)),
                          'b': (('time', 'y', 'x'), torch.from_numpy(a * 2).to(device))})
    X, _ = ref.build_X([(('time', 'y', 'x'), a), (('time', 'y', 'x'), a * 2)], ('time', 'y', 'x'))
    wX, wy, _ = ref.make_Xy(X, np.broadcast_to(lab, a.shape).reshape(-1))
    gX, gy = classify.Classifier(None).make_Xy(ds, lab)
    assert gX.tobytes() == wX.tobytes() and np.array_equal(gy, wy)


# ---- class_mean -------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('nans', [False, True])
@pytest.mark.parametrize('nclasses', [4, 20, 1500])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_class_mean_is_the_loop(device, dtype, nclasses, nans, first):
    import torch
    rng = np.random.default_rng(nclasses)
    ny, nx, nt = 60, 70, 3
    labels = rng.integers(first, first + nclasses, size=(ny, nx))
    labels.reshape(-1)[:nclasses] = np.arange(first, first + nclasses)
    a = (rng.gamma(4.0, 0.25, size=(ny, nx, nt)) + labels[..., None] % 7).astype(dtype)
    if nans:
        a[rng.random(a.shape) < 0.05] = np.nan
    want = ref.class_mean(a, np.broadcast_to(labels[..., None], a.shape))
    lab = xr_lite.DataArray(labels, ('y', 'x'))
    for dev in (None, device):
        ds = xr_lite.Dataset({'C11': (('y', 'x', 'time'), torch.from_numpy(a).to(dev) if dev else a),
                              'flat': (('y', 'x'), torch.from_numpy(a[..., 0].copy()).to(dev) if dev else a[..., 0])})
        got = classify.class_mean(ds, lab)
        g = host(got['C11'].values)
        assert g.dtype == dtype and got['C11'].dims == ('y', 'x', 'time')
        np.testing.assert_allclose(g, want, rtol=1e-5, equal_nan=True)
        np.testing.assert_allclose(host(got['flat'].values), ref.class_mean(a[..., 0], labels), rtol=1e-5,
                                   equal_nan=True)
        if not nans:
            for l in range(first, nclasses):
                assert len(np.unique(g[labels == l])) == 1                  # test_class_mean of the reference
        if first == 1:
            top = (labels == nclasses)[..., None] & ~np.isnan(a)            # no class: untouched
            np.testing.assert_array_equal(g[top], a[top])
    # a label dimension of size 1 is squeezed, as make_Xy squeezes it
    banded = xr_lite.DataArray(labels[None], ('band', 'y', 'x'))
    np.testing.assert_allclose(host(classify.class_mean(ds, banded)['C11'].values), want, rtol=1e-5, equal_nan=True)
    # a transposed variable and a single DataArray
    da = xr_lite.DataArray(torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 0, 1)))).to(device),
                           ('time', 'y', 'x'))
    np.testing.assert_allclose(host(classify.class_mean(da, lab).values), np.transpose(want, (2, 0, 1)), rtol=1e-5,
                               equal_nan=True)
