"""Writes tests/golden/classify_knn_linear_sklearn.npz with scikit-learn 1.7.2: for every recipe of
tests/classify_knn_linear_ref.py the fitted model as arrays and scikit-learn's own predict, decision_function
and predict_proba (both for models of few classes only: they are most of the file; the decision values of
the others are scikit-learn's expression X @ coef_.T + intercept_, which the tests evaluate) on the reference's
(rows, features) matrix.
Run from the repository root:
    python tests/golden/make_classify_knn_linear_golden.py"""
import os
import sys
import warnings

import numpy as np
import sklearn
from sklearn import neighbors, preprocessing

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import classify_cases as cases, classify_knn_linear_ref as kl      # noqa: E402


def main():
    assert sklearn.__version__ == '1.7.2', sklearn.__version__
    warnings.simplefilter('error')                       # a recipe that does not converge is changed, not recorded
    out = {'sklearn_version': np.array(sklearn.__version__)}
    for dtype in cases.DTYPES:
        tag = np.dtype(dtype).name
        for name, (k, ncls, fdims, scale, algorithm) in kl.KNN.items():
            _, X, _, (Xt, yt) = kl.knn_case(name, dtype)
            key = '%s/%s/' % (tag, name)
            keep = ~np.isnan(X).any(axis=1)
            Xp = X[keep]
            if scale:
                sc = preprocessing.StandardScaler().fit(Xt)
                out[key + 'mean'], out[key + 'scale'] = sc.mean_, sc.scale_
                Xt, Xp = sc.transform(Xt), sc.transform(Xp)
            clf = neighbors.KNeighborsClassifier(k, algorithm=algorithm).fit(Xt, yt)
            assert clf._fit_X.dtype == dtype and clf.effective_metric_ == 'euclidean'
            out[key + 'train'] = clf._fit_X
            out[key + 'target'] = clf._y.astype(np.int16)
            out[key + 'classes'] = clf.classes_
            out[key + 'predict'] = clf.predict(Xp).astype(np.int16)
            if ncls <= kl.PROBA_CLASSES:
                out[key + 'proba'] = clf.predict_proba(Xp)
            gap = kl.knn_neighbours(Xp, clf._fit_X, k)[1]
            assert (gap < kl.KNN_GAP).mean() <= kl.KNN_GAP_ROWS, (name, (gap < kl.KNN_GAP).mean())
        for name, (kind, ncls, scale) in kl.LINEAR.items():
            _, X, _, (Xt, yt) = kl.linear_case(name, dtype)
            key = '%s/%s/' % (tag, name)
            keep = ~np.isnan(X).any(axis=1)
            Xp = X[keep]
            if scale:
                sc = preprocessing.StandardScaler().fit(Xt)
                out[key + 'mean'], out[key + 'scale'] = sc.mean_, sc.scale_
                Xt, Xp = sc.transform(Xt), sc.transform(Xp)
            clf = kl.make_linear(name).fit(Xt, yt)
            model_link = 'none'
            out[key + 'coef'], out[key + 'intercept'] = clf.coef_, clf.intercept_
            out[key + 'classes'] = clf.classes_
            if ncls <= kl.PROBA_CLASSES:
                out[key + 'decision'] = clf.decision_function(Xp)
            out[key + 'predict'] = clf.predict(Xp).astype(np.int16)
            if kind == 'LogisticRegression':
                from nd_amd import classify
                model_link = classify.LinearModel.from_sklearn(clf).link
                if ncls <= kl.PROBA_CLASSES:
                    out[key + 'proba'] = clf.predict_proba(Xp)
            out[key + 'link'] = np.array(model_link)
    path = os.path.join(ROOT, 'tests', 'golden', 'classify_knn_linear_sklearn.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
