"""Writes tests/golden/classify_sklearn.npz with scikit-learn 1.7.2: for every case of tests/classify_cases.py
the fitted model as arrays and scikit-learn's own predict / predict_proba (forests) or labels (k-means) on
the reference's (rows, features) matrix.  Run from the repository root:
    python tests/golden/make_classify_golden.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn import cluster, ensemble, preprocessing, tree

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import classify_cases as cases, classify_ref as ref      # noqa: E402


def make_forest(name):
    kw = dict(random_state=1, max_depth=8, min_samples_leaf=3)
    if name.startswith('rf'):
        return ensemble.RandomForestClassifier(12, **kw)
    if name.startswith('et'):
        return ensemble.ExtraTreesClassifier(8, **kw)
    return tree.DecisionTreeClassifier(**kw)


def make_kmeans(name, k):
    if name.startswith('mbk'):
        return cluster.MiniBatchKMeans(k, random_state=1, n_init=3)
    return cluster.KMeans(k, random_state=1, n_init=3)


def main():
    assert sklearn.__version__ == '1.7.2', sklearn.__version__
    out = {'sklearn_version': np.array(sklearn.__version__)}
    for dtype in cases.DTYPES:
        tag = np.dtype(dtype).name
        for name, (ncls, fdims, scale, nt, dtypes) in cases.FORESTS.items():
            if dtype not in dtypes:
                continue
            data, truth = cases.stack(ncls, dtype, seed=ncls, nt=nt)
            X, shape = ref.build_X(cases.variables(data), cases.data_dims(fdims), fdims)
            lab = ref.broadcast_array(cases.training_labels(truth, seed=ncls), shape).reshape(-1)
            Xt, yt, _ = ref.make_Xy(X, lab)
            key = '%s/%s/' % (tag, name)
            if scale:
                sc = preprocessing.StandardScaler().fit(Xt)
                out[key + 'mean'], out[key + 'scale'] = sc.mean_, sc.scale_
                Xt = sc.transform(Xt)
            clf = make_forest(name).fit(Xt, yt)
            keep = ~np.isnan(X).any(axis=1)
            Xp = X[keep]
            if scale:
                Xp = sc.transform(Xp)
            trees = [e.tree_ for e in getattr(clf, 'estimators_', [clf])]
            out[key + 'feature'] = np.concatenate([t.feature for t in trees]).astype(np.int32)
            out[key + 'threshold'] = np.concatenate([t.threshold for t in trees])
            out[key + 'left'] = np.concatenate([t.children_left for t in trees]).astype(np.int32)
            out[key + 'right'] = np.concatenate([t.children_right for t in trees]).astype(np.int32)
            out[key + 'value'] = np.concatenate([t.value[:, 0, :] for t in trees])
            out[key + 'tree_offsets'] = np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int32)
            out[key + 'classes'] = clf.classes_
            out[key + 'proba'] = clf.predict_proba(Xp)
            out[key + 'predict'] = clf.predict(Xp)
        for name, (k, fdims, scale, nt, dtypes) in cases.KMEANS.items():
            data, truth = cases.stack(k, dtype, seed=k, nt=nt)
            X, shape = ref.build_X(cases.variables(data), cases.data_dims(fdims), fdims)
            keep = ~np.isnan(X).any(axis=1)
            Xp = X[keep]
            key = '%s/%s/' % (tag, name)
            if scale:
                sc = preprocessing.StandardScaler().fit(Xp)
                out[key + 'mean'], out[key + 'scale'] = sc.mean_, sc.scale_
                Xp = sc.transform(Xp)
            clf = make_kmeans(name, k).fit(Xp)
            centers = clf.cluster_centers_.astype(np.float64)
            out[key + 'centers'] = centers
            out[key + 'labels'] = clf.predict(Xp).astype(np.int32)
            gap = ref.kmeans_gap(Xp, centers)
            # the caps the GPU tests allow for rows left out of a comparison
            assert (gap < 1e-12).mean() <= 1e-4, (name, (gap < 1e-12).mean())
            assert (gap < 1e-3).mean() <= 1e-2, (name, (gap < 1e-3).mean())
    path = os.path.join(ROOT, 'tests', 'golden', 'classify_sklearn.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
