"""Writes tests/golden/kmeans_fit_sklearn.npz with scikit-learn 1.7.2: for every case of tests/kmeans_fit_ref.py
and both data types the initial centres and what KMeans(k, init=array, n_init=1, algorithm='lloyd') makes of
them -- cluster_centers_, labels_, n_iter_, inertia_ -- fitted on the FLOAT64 COPY of the matrix (scikit-learn sums
in its input's type; for a scaled case the matrix is StandardScaler().fit(X).transform(X) in X's type, then cast),
with StandardScaler's mean_ and var_.  No case may end with an empty cluster: scikit-learn would relocate it.
Run from the repository root:
    python tests/golden/make_kmeans_fit_golden.py"""
import os
import sys
import warnings

import numpy as np
import sklearn
from sklearn import cluster, preprocessing

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import kmeans_fit_ref as kf      # noqa: E402


def main():
    assert sklearn.__version__ == '1.7.2', sklearn.__version__
    warnings.simplefilter('error')                       # a case that does not converge is changed, not recorded
    out = {'sklearn_version': np.array(sklearn.__version__)}
    for dtype in kf.DTYPES:
        for name in kf.CASES:
            _, X, _, k, scale, init = kf.case(name, dtype)
            key = '%s/%s/' % (np.dtype(dtype).name, name)
            Xp = X[~np.isnan(X).any(axis=1)]
            if scale:
                sc = preprocessing.StandardScaler().fit(Xp)
                out[key + 'mean'], out[key + 'var'], out[key + 'scale'] = sc.mean_, sc.var_, sc.scale_
                init = kf.scaled_init(name, X, sc.mean_, sc.scale_)
                Xp = sc.transform(Xp)
                assert Xp.dtype == dtype
            else:
                sc = preprocessing.StandardScaler().fit(Xp)
                out[key + 'mean'], out[key + 'var'] = sc.mean_, sc.var_
            km = cluster.KMeans(k, init=init.copy(), n_init=1, algorithm='lloyd').fit(Xp.astype(np.float64))
            counts = np.bincount(km.labels_, minlength=k)
            assert counts.min() > 0, (name, counts)
            out[key + 'init'] = init
            out[key + 'centers'] = km.cluster_centers_
            out[key + 'labels'] = km.labels_.astype(np.int8)
            out[key + 'n_iter'] = np.array(km.n_iter_)
            out[key + 'inertia'] = np.array(km.inertia_)
            print(key, 'n_iter', km.n_iter_, 'smallest cluster', counts.min())
    path = os.path.join(ROOT, 'tests', 'golden', 'kmeans_fit_sklearn.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
