"""K-means training without a GPU: the numpy restatement (tests/kmeans_fit_ref.py) against scikit-learn 1.7.2's
recorded fits (tests/golden/kmeans_fit_sklearn.npz) and against live scikit-learn, the one deliberate difference
(an empty cluster keeps its centre), the estimator's surface, and the C ABI declarations and refusals."""
import os
import re

import numpy as np
import pytest

from nd_amd import classify
from tests import kmeans_fit_ref as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kmeans_fit_sklearn.npz')
NEW_SYMBOLS = ('nd_amd_kmeans_step', 'nd_amd_feature_moments', 'nd_amd_gather_rows')
CASES = [(n, dt) for n in kf.CASES for dt in kf.DTYPES]
RTOL = 1e-12


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def check_fit(run, centers, labels, n_iter, inertia):
    """the pin of a fit to scikit-learn's: n_iter and every label equal, centres within 1e-12 of the largest
    centre magnitude, inertia within 1e-12 relative"""
    assert run['n_iter'] == int(n_iter)
    np.testing.assert_array_equal(run['labels'], labels)
    assert np.abs(run['centers'] - centers).max() <= RTOL * np.abs(centers).max()
    assert abs(run['inertia'] - float(inertia)) <= RTOL * float(inertia)


def test_golden_is_sklearn_1_7_2(golden):
    assert str(golden['sklearn_version']) == '1.7.2'
    assert os.path.getsize(GOLDEN) < 2 ** 20


@pytest.mark.parametrize('name,dtype', CASES)
def test_restatement_matches_golden(golden, name, dtype):
    _, X, _, k, scale, init = kf.case(name, dtype)
    key = '%s/%s/' % (np.dtype(dtype).name, name)
    valid = ~np.isnan(X).any(axis=1)
    n, mean, var = kf.moments(X)
    assert n == valid.sum() and 0 < n < X.shape[0]
    np.testing.assert_allclose(mean, golden[key + 'mean'], rtol=RTOL, atol=0)
    np.testing.assert_allclose(var, golden[key + 'var'], rtol=RTOL, atol=0)
    sc = (None, None)
    if scale:
        np.testing.assert_array_equal(kf.scaler_scale(golden[key + 'var']), golden[key + 'scale'])
        sc = (golden[key + 'mean'], golden[key + 'scale'])
        init = kf.scaled_init(name, X, *sc)
    np.testing.assert_array_equal(init, golden[key + 'init'])
    run = kf.lloyd(X, init, mean=sc[0], scale_=sc[1])
    assert run['empty'].size == 0 and run['counts'].sum() == n      # so scikit-learn relocated nothing
    assert np.all(run['labels'][~valid] == -1)
    run['labels'] = run['labels'][valid]
    check_fit(run, golden[key + 'centers'], golden[key + 'labels'], golden[key + 'n_iter'], golden[key + 'inertia'])
    assert 1 < run['n_iter'] < 300


@pytest.mark.parametrize('dtype', kf.DTYPES)
def test_restatement_matches_live_sklearn(dtype):
    pytest.importorskip('sklearn')
    from sklearn.cluster import KMeans
    from sklearn.preprocessing import StandardScaler
    for name, tol, max_iter in (('f4k5', 1e-4, 300), ('f3k2', 0.0, 300), ('f2k3', 1e-1, 300), ('f4k5', 1e-4, 3),
                                ('f8k6_scale', 1e-4, 300)):
        _, X, _, k, scale, init = kf.case(name, dtype)
        Xp = X[~np.isnan(X).any(axis=1)]
        sc = (None, None)
        if scale:
            s = StandardScaler().fit(Xp)
            sc = (s.mean_, s.scale_)
            init = kf.scaled_init(name, X, *sc)
            Xp = s.transform(Xp)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')              # max_iter=3 does not converge, on purpose
            km = KMeans(k, init=init.copy(), n_init=1, algorithm='lloyd', tol=tol, max_iter=max_iter)
            km.fit(Xp.astype(np.float64))
        run = kf.lloyd(X, init, max_iter=max_iter, tol=tol, mean=sc[0], scale_=sc[1])
        run['labels'] = run['labels'][run['labels'] >= 0]
        check_fit(run, km.cluster_centers_, km.labels_, km.n_iter_, km.inertia_)


def test_restatement_keeps_the_centre_of_an_empty_cluster():
    _, X, _, k, _, init = kf.case('f2k3', np.float64)
    far = np.array([[1e3, -1e3]])
    run = kf.lloyd(X, np.concatenate([init, far]))
    np.testing.assert_array_equal(run['empty'], [k])
    np.testing.assert_array_equal(run['centers'][k], far[0])
    assert run['counts'][k] == 0 and not np.any(run['labels'] == k)
    alone = kf.lloyd(X, init)
    np.testing.assert_array_equal(run['centers'][:k], alone['centers'])
    assert run['n_iter'] == alone['n_iter'] and run['inertia'] == alone['inertia']


def test_restatement_step_and_moments_definitions():
    X = np.array([[0., 0.], [1., 0.], [np.nan, 5.], [4., 4.], [0.5, 0.]], np.float32)
    centers = np.array([[0.5, 0.], [0.5, 0.], [4., 4.]])           # a duplicate: the first minimum wins
    labels, sums, counts, inertia, changed, mag = kf.step(X, centers, np.full(5, -1))
    np.testing.assert_array_equal(labels, [0, 0, -1, 2, 0])
    np.testing.assert_array_equal(counts, [3, 0, 1])
    np.testing.assert_array_equal(sums, [[1.5, 0.], [0., 0.], [4., 4.]])
    assert inertia == 0.5 and changed == 4
    assert kf.step(X, centers, labels)[4] == 0
    n, mean, var = kf.moments(X)
    assert n == 4
    np.testing.assert_array_equal(mean, [1.375, 1.0])
    np.testing.assert_allclose(var, X[[0, 1, 3, 4]].astype(np.float64).var(axis=0), rtol=1e-15)
    np.testing.assert_array_equal(kf.scaler_scale(np.array([4.0, 0.0])), [2.0, 1.0])


def test_device_kmeans_surface():
    km = classify.DeviceKMeans(5, init='random', n_init=2, max_iter=7, tol=1e-3, random_state=4)
    assert km.get_params() == dict(n_clusters=5, init='random', n_init=2, max_iter=7, tol=1e-3, random_state=4)
    assert classify.DeviceKMeans().get_params()['n_clusters'] == 8
    assert km.cluster_centers_ is None and km.n_iter_ is None and km.inertia_ is None
    public = {a for a in dir(km) if not a.startswith('_')}
    assert public == set(km.get_params()) | {'get_params', 'predict', 'cluster_centers_', 'n_iter_', 'inertia_'}
    with pytest.raises(AttributeError, match='not fitted'):
        classify._model_for(km, 'predict')
    with pytest.raises(NotImplementedError, match='func'):
        classify._model_for(km, 'predict_proba')
    with pytest.raises(TypeError, match='takes no labels'):
        classify.Classifier(km).fit(None, labels=np.ones((2, 2)))
    km.cluster_centers_ = np.arange(6.0).reshape(3, 2)
    model = classify._model_for(km, 'predict')
    assert isinstance(model, classify.KMeansModel) and model.n_features == 2
    assert 'fit_kmeans' in classify.__all__ and 'DeviceKMeans' in classify.__all__


def test_header_and_binding_declare_the_new_symbols():
    from nd_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    for s in NEW_SYMBOLS + ('nd_amd_kmeans_fit_workspace_bytes',):
        assert re.search(r'\b%s\s*\(' % s, header), s
        assert s in _lib.SYMBOLS
    for i, (py, c) in enumerate((('kmeans_step', 'KMEANS_STEP'), ('feature_moments', 'FEATURE_MOMENTS'),
                                 ('gather_rows', 'GATHER_ROWS')), 23):
        assert _lib.KERNEL_NAMES[i] == py
        assert re.search(r'#define\s+ND_AMD_KERNEL_%s\s+%d\b' % (c, i), header)
    assert re.search(r'#define\s+ND_AMD_KMEANS_FIT_MAX_ACC\s+%d\b' % _lib.KMEANS_FIT_MAX_ACC, header)
    assert _lib.KMEANS_FIT_MAX_ACC == classify.KMEANS_FIT_MAX_ACC == 4096
    # the scratch check reads every kernel of the new translation unit
    for kernel in ('kmeans_step_kernel', 'feature_moments_kernel', 'gather_rows_kernel', 'fit_fold_kernel'):
        assert build.NO_SCRATCH['kmeans_fit.hip'] in kernel
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s)


def test_workspace_query():
    from nd_amd import _lib
    L = _lib.lib()
    q = L.nd_amd_kmeans_fit_workspace_bytes
    table = L.nd_amd_classify_workspace_bytes(4)
    assert q(4, 8, 0) > table and q(4, 8, 10 ** 9) >= q(4, 8, 1000) > q(4, 8, 0)
    assert q(4, 8, 10 ** 9) == q(4, 8, 10 ** 10)                  # the grid is capped
    assert q(4, 8, 10 ** 9) % 256 == 0 and q(1023, 4, 10 ** 9) <= 64 << 20
    for bad in ((0, 8, 10), (1025, 1, 10), (4, 0, 10), (4, 820, 10), (4, 8, -1)):
        assert q(*bad) == 0, bad
    assert q(4, 819, 10) > 0 and q(1023, 4, 10) > 0 and q(1024, 3, 10) > 0


def test_bad_arguments_are_refused_without_a_gpu():
    """every refusal happens before the first HIP call (the pointers are never read)"""
    import ctypes
    from nd_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    msg = lambda: L.nd_amd_last_error().decode()
    feat = (vp * 2)(256, 256)
    sz, st = _lib.i64_array([1, 1, 4, 4]), _lib.i64_array([0, 0, 4, 1])
    big = 1 << 30

    def step(nfeat=2, dtype=0, k=3, mean=None, table=feat, wsb=big, ws=256, sums=256, sizes=sz):
        return L.nd_amd_kmeans_step(table, nfeat, dtype, sizes, st, vp(256), k, mean, None, vp(256), vp(sums), vp(256),
                                    vp(256), vp(256), vp(ws), wsb, None)

    def moments(nfeat=2, dtype=0, mean=None, table=feat, wsb=big, ws=256, count=256, sizes=sz):
        return L.nd_amd_feature_moments(table, nfeat, dtype, sizes, st, mean, None, vp(count), vp(256), vp(256), vp(ws),
                                        wsb, None)

    def gather(nfeat=2, dtype=0, m=5, mean=None, table=feat, wsb=big, ws=256, X=256, sizes=sz):
        return L.nd_amd_gather_rows(table, nfeat, dtype, sizes, st, vp(256), m, mean, None, vp(X), vp(256), vp(ws), wsb,
                                    None)

    for call in (step, moments, gather):
        assert call(dtype=7) == _lib.EINVAL and 'dtype' in msg()
        assert call(nfeat=0) == _lib.EINVAL and 'features' in msg()
        assert call(table=None) == _lib.EINVAL and 'features' in msg()
        assert call(table=(vp * 2)(256, 0)) == _lib.EINVAL and 'NULL' in msg()
        assert call(wsb=8) == _lib.EWORKSPACE and 'workspace' in msg()
        assert call(ws=0) == _lib.EWORKSPACE and 'workspace' in msg()
        assert call(mean=vp(256)) == _lib.EINVAL and 'scaler' in msg()
        assert call(sizes=_lib.i64_array([1, 1, -4, 4])) == _lib.EINVAL and 'shape' in msg()
    assert step(k=0) == _lib.EINVAL and 'k = 0' in msg()
    assert step(k=-2) == _lib.EINVAL and 'k >= 1' in msg()
    assert step(k=1366) == _lib.EUNSUPPORTED and '4096' in msg()      # 1366 * (2 + 1) = 4098
    assert step(sums=0) == _lib.EINVAL and 'sums' in msg()
    table_only = L.nd_amd_classify_workspace_bytes(2)
    assert step(wsb=table_only) == _lib.EWORKSPACE and 'nd_amd_kmeans_fit_workspace_bytes' in msg()
    assert moments(wsb=table_only) == _lib.EWORKSPACE
    assert moments(count=0) == _lib.EINVAL and 'count' in msg()
    many = (vp * 1024)(*[256] * 1024)
    assert step(nfeat=1024, table=many, k=4) == _lib.EUNSUPPORTED                  # 4 * 1025 = 4100
    assert gather(m=-1) == _lib.EINVAL and 'm = -1' in msg()
    assert gather(X=0) == _lib.EINVAL
    assert gather(m=0, X=0) == _lib.OK
