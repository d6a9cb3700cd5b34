"""K-means training on the device against the numpy restatement (tests/kmeans_fit_ref.py) and scikit-learn 1.7.2's
recorded fits (tests/golden/kmeans_fit_sklearn.npz).  Labels, counts and iteration counts must be equal; float64
sums are held to rows * 2^-52 relative to the sum of the magnitudes, the forward bound of a float64 sum in any
order; fitted centres and inertia to 1e-12, the bound the restatement itself keeps against scikit-learn."""
import functools
import os

import numpy as np
import pytest

from nd_amd import classify, xr_lite
from tests import classify_cases as cases, classify_ref as ref, kmeans_fit_ref as kf
from tests.test_classify_gpu import Scaler, dataset, host, mock_classes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kmeans_fit_sklearn.npz')
SMALL, LARGE = (3, 37, 53), (2, 300, 301)
# features -> (variables, feature_dims) on a stack of three dates
FEATURES = {1: (1, ()), 3: (3, ()), 9: (3, ('time',)), 33: (11, ('time',))}
U = 2.0 ** -52
RTOL = 1e-12


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def reference(nvars, shape, fdims, dtype, constant=None):
    """-> (data, X): a stack and the reference's matrix of it, computed once and left unchanged"""
    data = kf.stack(nvars, shape, 4, dtype, seed=nvars, constant=constant)
    X, _ = ref.build_X(kf.variables(data), cases.data_dims(fdims), fdims)
    X.setflags(write=False)
    return data, X


def table(data, fdims, layout, device):
    return classify._Layout(dataset(data, layout, device), fdims)


def scaler_of(X):
    _, mean, var = kf.moments(X)
    return mean, kf.scaler_scale(var)


def run_step(lay, centers, prev, mean=None, scale=None):
    import torch
    from nd_amd import kernels
    labels = torch.from_numpy(np.asarray(prev, np.int32)).to(lay.device).reshape(lay.shape).contiguous()
    out = kernels.kmeans_step(lay.features, lay.shape, lay.strides, torch.from_numpy(centers).to(lay.device), labels,
                              mean, scale)
    sums, counts, inertia, changed = (host(t) for t in out)
    return host(labels).reshape(-1), sums, counts, float(inertia), int(changed)


def check_step(lay, X, centers, prev, mean=None, scale=None):
    """one step against the restatement -> the device's (labels, sums)"""
    want_labels, want_sums, want_counts, want_inertia, want_changed, mag = kf.step(X, centers, prev, mean, scale)
    labels, sums, counts, inertia, changed = run_step(lay, centers, prev, mean, scale)
    np.testing.assert_array_equal(labels, want_labels)
    np.testing.assert_array_equal(counts, want_counts)
    assert changed == want_changed
    bound = X.shape[0] * U
    excess = np.abs(sums - want_sums) - bound * mag
    assert np.all(excess <= 0), (np.abs(sums - want_sums) / np.maximum(mag, 1e-300)).max() / bound
    assert abs(inertia - want_inertia) <= bound * want_inertia, abs(inertia / want_inertia - 1) / bound
    return labels, sums, inertia


@pytest.mark.parametrize('k', [1, 2, 5, 16])
@pytest.mark.parametrize('nfeat', list(FEATURES))
def test_kmeans_step_is_the_restatement(device, nfeat, k):
    """both data types, both layouts, with and without the scaler; NaN pixels, one whole wave of them; the first
    iteration (every valid row changes), a repeated one (none does) and one from other labels"""
    nvars, fdims = FEATURES[nfeat]
    for dtype in cases.DTYPES:
        data, X = reference(nvars, SMALL, fdims, dtype)
        assert X.shape[1] == nfeat and X.shape[0] % 64 != 0 and X.shape[0] > 256
        assert np.isnan(X[128:192]).any(axis=1).all()                       # a whole wave of rows drops out
        for layout in ('tyx', 'yxt'):
            lay = table(data, fdims, layout, device)
            for scaled in (False, True):
                mean, scale = scaler_of(X) if scaled else (None, None)
                Xs = ref.scale(X, mean, scale) if scaled else X
                centers = kf.draw_init(Xs, k, seed=k + nfeat)
                if k == 5:
                    centers[3] = centers[1]                                    # a duplicate: the lower index wins
                first = np.full(X.shape[0], -1)
                labels, sums, inertia = check_step(lay, X, centers, first, mean, scale)
                assert (labels >= 0).sum() == (~np.isnan(X).any(axis=1)).sum()
                again = run_step(lay, centers, labels, mean, scale)
                assert again[4] == 0                                           # no label changed
                assert again[1].tobytes() == sums.tobytes() and again[3] == inertia      # bit for bit
                if k > 1:
                    check_step(lay, X, centers, (labels + 1) % k, mean, scale)


@pytest.mark.parametrize('nfeat', [4, 5, 8])
def test_kmeans_step_feature_counts_at_the_bounds_of_the_register_forms(device, nfeat):
    """4 features are the last of the first register form, 5 the first and 8 the last of the second (9, the first
    read through LDS, is in FEATURES): one variable per feature, both data types, with the scaler"""
    for dtype in cases.DTYPES:
        data, X = reference(nfeat, SMALL, (), dtype)
        assert X.shape[1] == nfeat
        lay = table(data, (), 'tyx', device)
        mean, scale = scaler_of(X)
        centers = kf.draw_init(ref.scale(X, mean, scale), 3, seed=nfeat)
        labels, _, _ = check_step(lay, X, centers, np.full(X.shape[0], -1), mean, scale)
        check_step(lay, X, centers, (labels + 1) % 3, mean, scale)


def test_kmeans_step_at_the_accumulator_limit_and_past_the_grid(device):
    """k * (features + 1) = 4080 of 4096 accumulators; and a stack of more batches than the grid has blocks, where
    a block walks several batches"""
    import torch
    from nd_amd import kernels
    data, X = reference(11, SMALL, ('time',), np.float32)
    lay = table(data, ('time',), 'yxt', device)
    centers = kf.draw_init(X, 120, seed=7)
    check_step(lay, X, centers, np.full(X.shape[0], -1))
    with pytest.raises(NotImplementedError, match='4096'):
        kernels.kmeans_step(lay.features, lay.shape, lay.strides, torch.zeros((121, 33), dtype=torch.float64,
                                                                              device=device),
                            torch.zeros(lay.shape, dtype=torch.int32, device=device))
    for shape, nvars, fdims, k in ((LARGE, 3, (), 5), ((2, 600, 601), 1, (), 2)):
        data, X = reference(nvars, shape, fdims, np.float32)
        lay = table(data, fdims, 'tyx', device)
        labels, sums, _ = check_step(lay, X, kf.draw_init(X, k, seed=3), np.full(X.shape[0], -1))
        assert run_step(lay, kf.draw_init(X, k, seed=3), labels)[1].tobytes() == sums.tobytes()
    assert X.shape[0] > 8192 * 64                                               # more batches than blocks


def check_moments(lay, X, mean=None, scale=None):
    from nd_amd import kernels
    count, fmean, fvar = (host(t) for t in kernels.feature_moments(lay.features, lay.shape, lay.strides, mean, scale))
    n, want_mean, want_var = kf.moments(X, mean, scale)
    assert int(count) == n
    V, valid = kf.values(X, mean, scale)
    mag = np.abs(V[valid]).sum(axis=0) / n
    bound = X.shape[0] * U
    assert np.all(np.abs(fmean - want_mean) <= bound * mag)
    # a mean off by dm moves sum (x - m)^2 by at most 2 dm sum |x - m| + n dm^2 <= about 2 n dm sigma
    slack = bound * (want_var + 2 * mag * np.sqrt(want_var)) + (bound * mag) ** 2
    assert np.all(np.abs(fvar - want_var) <= slack), np.abs(fvar - want_var) / np.maximum(slack, 1e-300)
    return int(count), fmean, fvar


@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_feature_moments(device, dtype, layout):
    from nd_amd import kernels
    for nfeat, (nvars, fdims) in FEATURES.items():
        data, X = reference(nvars, SMALL, fdims, dtype)
        lay = table(data, fdims, layout, device)
        _, fmean, fvar = check_moments(lay, X)
        mean, scale = scaler_of(X)
        _, smean, svar = check_moments(lay, X, mean, scale)
        assert np.all(np.abs(smean) < 1e-5) and np.all(np.abs(svar - 1) < 1e-5)     # the scaled values
        twice = kernels.feature_moments(lay.features, lay.shape, lay.strides)
        assert host(twice[1]).tobytes() == fmean.tobytes() and host(twice[2]).tobytes() == fvar.tobytes()
    # a constant feature: variance exactly 0, which the scaler turns into a scale of 1
    data, X = reference(3, SMALL, (), dtype, constant=1)
    lay = table(data, (), layout, device)
    _, fmean, fvar = check_moments(lay, X)
    assert fmean[1] == 2.5 and fvar[1] == 0.0
    sc = classify._device_scaler(lay)
    assert sc.scale_[1] == 1.0 and sc.var_[1] == 0.0 and sc.n_features_in_ == 3
    np.testing.assert_array_equal(sc.scale_[[0, 2]], np.sqrt(fvar[[0, 2]]))


def test_feature_moments_many_batches_and_no_valid_row(device):
    import torch
    from nd_amd import kernels
    data, X = reference(1, (2, 600, 601), (), np.float32)
    check_moments(table(data, (), 'tyx', device), X)
    nan = torch.full((4, 5), float('nan'), device=device)
    count, fmean, fvar = kernels.feature_moments([nan, nan], (4, 5), (5, 1))
    assert int(count) == 0 and np.isnan(host(fmean)).all() and np.isnan(host(fvar)).all()


@pytest.mark.parametrize('layout', ['tyx', 'yxt'])
@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_gather_rows(device, dtype, layout):
    import torch
    from nd_amd import kernels
    rng = np.random.default_rng(5)
    for nfeat, (nvars, fdims) in FEATURES.items():
        data, X = reference(nvars, SMALL, fdims, dtype)
        lay = table(data, fdims, layout, device)
        rows = X.shape[0]
        index = np.concatenate([rng.integers(0, rows, 300), [0, rows - 1, 130, 130, 191, 7, 7, 7]])
        assert np.isnan(X[index]).any() and len(np.unique(index)) < len(index)
        idx = torch.from_numpy(index).to(device)
        got, valid = kernels.gather_rows(lay.features, lay.shape, lay.strides, idx)
        assert got.dtype == lay.features[0].dtype
        np.testing.assert_array_equal(host(got), X[index])
        np.testing.assert_array_equal(host(valid).astype(bool), ~np.isnan(X[index]).any(axis=1))
        mean, scale = scaler_of(X)
        got, valid = kernels.gather_rows(lay.features, lay.shape, lay.strides, idx, mean, scale)
        np.testing.assert_array_equal(host(got), ref.scale(X, mean, scale)[index])
        # an index outside the rows is not followed
        out = torch.tensor([3, -1, rows, 2 ** 40, 4], device=device)
        got, valid = kernels.gather_rows(lay.features, lay.shape, lay.strides, out)
        np.testing.assert_array_equal(host(valid), [1, 0, 0, 0, 1])
        assert np.isnan(host(got)[1:4]).all()
        np.testing.assert_array_equal(host(got)[[0, 4]], X[[3, 4]])
    empty = kernels.gather_rows(lay.features, lay.shape, lay.strides, torch.zeros(0, dtype=torch.int64, device=device))
    assert empty[0].shape == (0, X.shape[1]) and empty[1].shape == (0,)


def golden_case(golden, name, dtype, device, layout='tyx'):
    data, X, fdims, k, scale, _ = kf.case(name, dtype)
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    sc = Scaler(golden[key + 'mean'], golden[key + 'scale']) if scale else None
    return dataset(data, layout, device), X, fdims, key, sc


def check_model(model, ds, X, fdims, sc, centers, labels, n_iter, inertia, counts):
    valid = ~np.isnan(X).any(axis=1)
    assert model.n_iter == int(n_iter)
    got = host(classify.predict_kmeans(ds, model, fdims, sc).values).reshape(-1)
    assert np.isnan(got[~valid]).all()
    np.testing.assert_array_equal(got[valid], labels)
    np.testing.assert_array_equal(model.counts, counts)
    assert np.abs(model.centers - centers).max() <= RTOL * np.abs(centers).max()
    assert abs(model.inertia - float(inertia)) <= RTOL * float(inertia)


@pytest.mark.parametrize('dtype', cases.DTYPES)
@pytest.mark.parametrize('name', list(kf.CASES))
def test_fit_kmeans_is_sklearn(golden, device, name, dtype):
    """data on the device in one layout, numpy data in the other"""
    on_device = (dtype == np.float32) == (list(kf.CASES).index(name) % 2 == 0)
    ds, X, fdims, key, sc = golden_case(golden, name, dtype, device if on_device else None,
                                        'tyx' if on_device else 'yxt')
    model = classify.fit_kmeans(ds, kf.CASES[name][3], fdims, init=golden[key + 'init'], n_init=5, scaler=sc)
    labels = golden[key + 'labels']
    check_model(model, ds, X, fdims, sc, golden[key + 'centers'], labels, golden[key + 'n_iter'],
                golden[key + 'inertia'], np.bincount(labels, minlength=model.centers.shape[0]))
    assert model.empty.size == 0
    if sc is not None:                              # the device's scaler is scikit-learn's
        built = classify._device_scaler(classify._Layout(ds, fdims))
        np.testing.assert_allclose(built.mean_, golden[key + 'mean'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(built.var_, golden[key + 'var'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(built.scale_, golden[key + 'scale'], rtol=RTOL, atol=0)
        assert built.n_samples_seen_ == labels.size


@pytest.mark.parametrize('tol,max_iter', [(0.0, 300), (1e-1, 300), (1e-4, 1), (1e-4, 4)])
def test_fit_kmeans_stopping_rules(golden, device, tol, max_iter):
    """tol = 0: the stop is strict; a large tol: the stop is by the shift and the closing pass runs; max_iter"""
    ds, X, fdims, key, sc = golden_case(golden, 'f4k5', np.float32, device)
    init = golden[key + 'init']
    want = kf.lloyd(X, init, max_iter=max_iter, tol=tol)
    full = int(golden[key + 'n_iter'])
    if max_iter < 300:
        assert want['n_iter'] == max_iter
    if tol == 0.0:
        assert want['n_iter'] >= full
    if tol == 1e-1:
        assert 1 <= want['n_iter'] < full
    model = classify.fit_kmeans(ds, 5, fdims, init=init, tol=tol, max_iter=max_iter)
    check_model(model, ds, X, fdims, None, want['centers'], want['labels'][want['labels'] >= 0], want['n_iter'],
                want['inertia'], want['counts'])


def test_fit_kmeans_keeps_the_centre_of_an_empty_cluster(golden, device):
    ds, X, fdims, key, _ = golden_case(golden, 'f2k3', np.float64, device)
    far = np.array([[1e3, -1e3]])
    init = np.concatenate([golden[key + 'init'], far])
    want = kf.lloyd(X, init)
    model = classify.fit_kmeans(ds, 4, fdims, init=init)
    np.testing.assert_array_equal(model.empty, [3])
    np.testing.assert_array_equal(model.centers[3], far[0])
    check_model(model, ds, X, fdims, None, want['centers'], want['labels'][want['labels'] >= 0], want['n_iter'],
                want['inertia'], want['counts'])
    assert model.n_iter == int(golden[key + 'n_iter'])          # the other clusters go their way


def test_fit_kmeans_repeats_bit_for_bit(golden, device):
    ds, X, fdims, key, sc = golden_case(golden, 'f8k6_scale', np.float32, device)
    runs = [classify.fit_kmeans(ds, 6, fdims, init=golden[key + 'init'], scaler=sc) for _ in range(2)]
    assert runs[0].centers.tobytes() == runs[1].centers.tobytes()
    assert runs[0].inertia == runs[1].inertia and runs[0].n_iter == runs[1].n_iter
    for init in ('random', 'k-means++'):
        pytest.importorskip('sklearn')
        runs = [classify.fit_kmeans(ds, 6, fdims, init=init, n_init=2, random_state=3, scaler=sc, init_size=500)
                for _ in range(2)]
        assert runs[0].centers.tobytes() == runs[1].centers.tobytes() and runs[0].centers.shape == (6, 8)
        assert runs[0].counts.sum() == (~np.isnan(X).any(axis=1)).sum() and np.isfinite(runs[0].centers).all()
        assert runs[0].inertia > 0
    with pytest.raises(ValueError, match='init'):
        classify.fit_kmeans(ds, 6, fdims, init=np.zeros((5, 8)))
    with pytest.raises(ValueError, match='init'):
        classify.fit_kmeans(ds, 6, fdims, init='farthest')


def test_classifier_device_kmeans(device, monkeypatch):
    pytest.importorskip('sklearn')
    from sklearn.preprocessing import StandardScaler
    from nd_amd import kernels
    ds, labels = mock_classes(device=device)

    def no_matrix(*a, **k):
        raise AssertionError('Classifier(DeviceKMeans).fit formed the host matrix')
    monkeypatch.setattr(kernels, 'classify_gather', no_matrix)
    c = classify.Classifier(classify.DeviceKMeans(3, random_state=0))
    pred = c.fit_predict(ds)
    pv = host(pred.values)
    assert pred.dims == ('y', 'x', 'time') and pv.shape == (30, 40, 3) and len(np.unique(pv)) == 3
    for k in range(3):
        assert len(np.unique(pv[labels.values == k + 1])) == 1
    km = c.clf
    assert km.cluster_centers_.shape == (3, 2) and km.n_iter_ >= 1 and km.inertia_ > 0
    model = classify.KMeansModel(km.cluster_centers_)
    np.testing.assert_array_equal(host(c.predict(ds).values), host(classify.predict_kmeans(ds, model).values))
    # the estimator's own predict, on a matrix
    X, _ = ref.build_X([(('y', 'x', 'time'), host(ds[v].values)) for v in ('C11', 'C22')], ('y', 'x', 'time'))
    np.testing.assert_array_equal(km.predict(X), pv.reshape(-1))
    # scaled, time as a feature: the scaler is scikit-learn's
    c2 = classify.Classifier(classify.DeviceKMeans(3, random_state=0), feature_dims=['time'], scale=True)
    p2 = host(c2.fit_predict(ds).values)
    assert p2.shape == (30, 40)
    for k in range(3):
        assert len(np.unique(p2[labels.values == k + 1])) == 1
    X2, _ = ref.build_X([(('y', 'x', 'time'), host(ds[v].values)) for v in ('C11', 'C22')], ('y', 'x'), ('time',))
    sk = StandardScaler().fit(X2)
    np.testing.assert_allclose(c2._scaler.mean_, sk.mean_, rtol=RTOL, atol=0)
    np.testing.assert_allclose(c2._scaler.var_, sk.var_, rtol=RTOL, atol=0)
    np.testing.assert_allclose(c2._scaler.scale_, sk.scale_, rtol=RTOL, atol=0)
    assert c2._scaler.n_samples_seen_ == sk.n_samples_seen_ and c2._scaler.n_features_in_ == 6
    np.testing.assert_array_equal(p2, host(classify.predict_kmeans(
        ds, classify.KMeansModel(c2.clf.cluster_centers_), ('time',), c2._scaler).values))
    with pytest.raises(TypeError, match='no labels'):
        classify.Classifier(classify.DeviceKMeans(3)).fit(ds, labels)
    with pytest.raises(NotImplementedError, match='4096'):
        classify.Classifier(classify.DeviceKMeans(1366)).fit(ds)
    with pytest.raises(AttributeError):
        c.predict(ds, func='predict_proba')
    monkeypatch.undo()
    # scikit-learn's KMeans keeps going through make_Xy
    from sklearn.cluster import KMeans
    calls = []
    gather = kernels.classify_gather
    monkeypatch.setattr(kernels, 'classify_gather', lambda *a, **k: calls.append(1) or gather(*a, **k))
    classify.Classifier(KMeans(3, n_init=1, random_state=0)).fit(ds)
    assert calls == [1]
