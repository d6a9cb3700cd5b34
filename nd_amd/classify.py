"""
nd_amd/classify.py -- pixel classification (nd/classify.py) with prediction on the GPU.

  Classifier      nd.classify.Classifier: make_Xy, fit, predict, fit_predict, score
  fit_kmeans, DeviceKMeans
                  k-means trained on the device over every pixel: scikit-learn's Lloyd loop, no host matrix
  class_mean      nd.classify.class_mean
  ForestModel, KMeansModel, KNNModel, LinearModel,
  predict_forest, predict_kmeans, predict_knn, predict_linear
                  the device path for callers that hold a fitted model as plain arrays

Training is scikit-learn's and runs on the host: it sees only the labelled pixels and is not a hot path.
The exception is k-means, which trains on every pixel: Classifier(DeviceKMeans(k)) and fit_kmeans run the
Lloyd iterations on the device (one pass over the data each) and bring only the (k, n_features) sums back.
What the device does for it is the selection of those pixels -- label > 0 and not NaN, no NaN feature --
and their gather into a dense (n, n_features) matrix, in the reference's row order, straight from the
variables.  Prediction sees every pixel and runs on the device without ever forming the reference's
(n_pixels, n_features) matrix: the kernels read each feature where it lies.

Supported for `predict` (anything else raises NotImplementedError; there is no CPU fallback):
  DecisionTreeClassifier, ExtraTreeClassifier, RandomForestClassifier, ExtraTreesClassifier with one
  output and numeric classes_: func='predict' and func='predict_proba'.  Probabilities are bit-equal to
  scikit-learn 1.7.2 at n_jobs=1 (with n_jobs > 1 scikit-learn adds the trees in thread order and does
  not reproduce its own last bit); labels are equal everywhere, ties included.
  KMeans, MiniBatchKMeans: func='predict', the first nearest centre in float64.
  KNeighborsClassifier with uniform weights, the Euclidean metric, dense training data, one output, numeric
  classes_ and n_neighbors <= 32, on up to 128 features: func='predict' and func='predict_proba'.  With
  d_j = sum_f (x_f - t_jf)^2 in float64, summed in feature order, the neighbours are the k training samples
  smallest by (d_j, j) -- a tie in distance goes to the lower training index --, predict_proba is count_c / k
  and predict the first class with the largest count.  This does not depend on scikit-learn's search
  structure; scikit-learn agrees wherever the k-th and (k+1)-th distances are not within rounding.
  LogisticRegression: func='predict' and func='predict_proba'; LinearSVC, RidgeClassifier, SGDClassifier,
  Perceptron, PassiveAggressiveClassifier: func='predict'; one output, dense coef_, numeric classes_.
  s_c = b_c + sum_f x_f w_cf in float64, summed in feature order; predict is s > 0 for a binary model, else the
  first maximum; predict_proba applies the link LogisticRegression.predict_proba applies: softmax with the
  row maximum subtracted where the model is multinomial, expit normalised over the classes where it is
  one-vs-rest, [1 - p, p] for a binary model.

Row order and feature order are the reference's (_build_X, _get_data_dims): rows run over the data
dimensions in the order of the dataset's dimension coordinates (for an xr_lite object without coordinates:
the first variable's dimension order), feature = (position along feature_dims) * n_variables + variable.
Variables may be numpy arrays (copied up, results copied down) or torch ROCm tensors (results stay on the
device).  float32 and float64 are computed as they are, integers as float64.
"""
from collections import OrderedDict

import numpy as np

from . import _adapter, _device, xr_lite

__all__ = ['Classifier', 'class_mean', 'ForestModel', 'KMeansModel', 'KNNModel', 'LinearModel', 'predict_forest',
           'predict_kmeans', 'predict_knn', 'predict_linear', 'pack_forest', 'fit_kmeans', 'DeviceKMeans']

FORESTS = ('DecisionTreeClassifier', 'ExtraTreeClassifier', 'RandomForestClassifier', 'ExtraTreesClassifier')
KMEANS = ('KMeans', 'MiniBatchKMeans')
KNN = ('KNeighborsClassifier',)
LINEAR_PROBA = ('LogisticRegression',)
LINEAR_PREDICT = ('LinearSVC', 'RidgeClassifier', 'SGDClassifier', 'Perceptron', 'PassiveAggressiveClassifier')
KNN_MAX_K, KNN_MAX_FEATURES = 32, 128
_SUPPORTED = ('nd_amd.classify predicts on the device with %s (func "predict" or "predict_proba"; one output, '
              'numeric classes_), %s (func "predict"), %s (func "predict" or "predict_proba"; uniform weights, '
              'Euclidean metric, dense training data, n_neighbors <= %d, up to %d features, one output, numeric '
              'classes_), %s (func "predict" or "predict_proba") and %s (func "predict"; linear models with one '
              'output, dense coef_ and numeric classes_); there is no CPU fallback.  '
              % (', '.join(FORESTS), ', '.join(KMEANS), ', '.join(KNN), KNN_MAX_K, KNN_MAX_FEATURES,
                 ', '.join(LINEAR_PROBA), ', '.join(LINEAR_PREDICT)))


# ---------------------------------------------------------------------------
# models as plain arrays
# ---------------------------------------------------------------------------
def pack_forest(feature, threshold, left, right, tree_offsets):
    """-> (nodes (n, 4) int32, roots int32).  A node is {bits of t32, feature, left, right} with absolute
    child indices; a leaf has feature -1 and its own index in `left` (its row in the value table).
    scikit-learn goes left where float32(x) <= float64 threshold; for a float32 x that is x <= t32 with
    t32 the largest float32 not above the threshold."""
    feature, left, right = (np.asarray(a, np.int64) for a in (feature, left, right))
    threshold = np.asarray(threshold, np.float64)
    offsets = np.asarray(tree_offsets, np.int64)
    n = feature.size
    with np.errstate(over='ignore'):
        t32 = threshold.astype(np.float32)
    above = t32.astype(np.float64) > threshold
    t32[above] = np.nextafter(t32[above], np.float32(-np.inf))
    base = np.repeat(offsets[:-1], np.diff(offsets))
    leaf = left < 0
    nodes = np.empty((n, 4), np.int32)
    nodes[:, 0] = t32.view(np.int32)
    nodes[:, 1] = np.where(leaf, -1, feature)
    nodes[:, 2] = np.where(leaf, np.arange(n), left + base)
    nodes[:, 3] = np.where(leaf, np.arange(n), right + base)
    nodes[leaf, 0] = 0
    return nodes, offsets[:-1].astype(np.int32)


class ForestModel:
    """A fitted decision forest as arrays: the trees' nodes concatenated in estimator order.
    feature, threshold, left, right : (n_nodes,) as scikit-learn's tree_.feature / threshold / children_left /
        children_right (children are indices inside their own tree, -1 at a leaf)
    value : (n_nodes, n_classes) float64, tree_.value[:, 0, :]
    tree_offsets : (n_trees + 1,) first node of every tree, and n_nodes
    classes : (n_classes,) numeric classes_"""

    def __init__(self, feature, threshold, left, right, value, tree_offsets, classes, n_features=None):
        self.feature = np.ascontiguousarray(feature, np.int64)
        self.threshold = np.ascontiguousarray(threshold, np.float64)
        self.left = np.ascontiguousarray(left, np.int64)
        self.right = np.ascontiguousarray(right, np.int64)
        self.value = np.ascontiguousarray(value, np.float64)
        self.tree_offsets = np.ascontiguousarray(tree_offsets, np.int64)
        classes = np.asarray(classes)
        if classes.dtype.kind not in 'iufb':
            raise NotImplementedError(_SUPPORTED + 'classes_ of type %s are not numeric.' % classes.dtype)
        self.classes = np.ascontiguousarray(classes, np.float64)
        n = self.feature.size
        off = self.tree_offsets
        if not (self.threshold.shape == self.left.shape == self.right.shape == self.feature.shape == (n,)
                and self.value.shape == (n, self.classes.size) and n >= 1 and self.classes.size >= 1):
            raise ValueError('ForestModel: the node arrays must be (n_nodes,) and value (n_nodes, n_classes)')
        if off.ndim != 1 or off.size < 2 or off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 1):
            raise ValueError('ForestModel: tree_offsets must rise from 0 to n_nodes')
        if n >= 2 ** 31:
            raise ValueError('ForestModel: too many nodes')
        size = np.repeat(np.diff(off), np.diff(off))
        leaf = self.left < 0
        inner = ~leaf
        if (np.any(self.left[inner] >= size[inner]) or np.any(self.right[inner] >= size[inner])
                or np.any(self.right[inner] < 0) or np.any(self.feature[inner] < 0)):
            raise ValueError('ForestModel: a child index or feature lies outside its tree')
        local = np.arange(n) - np.repeat(off[:-1], np.diff(off))
        if np.any(self.left[inner] <= local[inner]) or np.any(self.right[inner] <= local[inner]):
            raise ValueError('ForestModel: a child must follow its parent (a walk must end)')
        if np.any(np.isnan(self.threshold[inner])):
            raise ValueError('ForestModel: NaN threshold')
        need = int(self.feature[inner].max()) + 1 if inner.any() else 1
        self.n_features = int(n_features) if n_features is not None else need
        if self.n_features < need:
            raise ValueError('ForestModel: a node asks for feature %d of %d' % (need - 1, self.n_features))
        self._packed = None
        self._device = {}

    n_trees = property(lambda self: self.tree_offsets.size - 1)
    n_classes = property(lambda self: self.classes.size)

    @classmethod
    def from_sklearn(cls, clf):
        names = {c.__name__ for c in type(clf).__mro__}
        if not names & set(FORESTS):
            raise NotImplementedError(_SUPPORTED + 'Got %s.' % type(clf).__name__)
        from sklearn.utils.validation import check_is_fitted
        check_is_fitted(clf)
        if getattr(clf, 'n_outputs_', 1) != 1:
            raise NotImplementedError(_SUPPORTED + 'Got a multi-output %s.' % type(clf).__name__)
        trees = [e.tree_ for e in getattr(clf, 'estimators_', [clf])]
        nc = len(clf.classes_)
        offsets = np.concatenate([[0], np.cumsum([t.node_count for t in trees])])
        cat = lambda key: np.concatenate([getattr(t, key) for t in trees])
        return cls(cat('feature'), cat('threshold'), cat('children_left'), cat('children_right'),
                   np.concatenate([t.value[:, 0, :nc] for t in trees]), offsets, clf.classes_,
                   n_features=clf.n_features_in_)

    def packed(self):
        if self._packed is None:
            self._packed = pack_forest(self.feature, self.threshold, self.left, self.right, self.tree_offsets)
        return self._packed

    def depth(self):
        """the longest root-to-leaf path of any tree, in edges"""
        nodes, roots = self.packed()
        front, d = roots.astype(np.int64), 0
        while True:
            inner = front[nodes[front, 1] >= 0]
            if not inner.size:
                return d
            front = np.concatenate([nodes[inner, 2], nodes[inner, 3]]).astype(np.int64)
            d += 1

    def _on(self, dev):
        import torch
        if dev not in self._device:
            nodes, roots = self.packed()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._device[dev] = (up(nodes.view(np.uint8).reshape(-1)), up(self.value), up(roots), up(self.classes))
        return self._device[dev]


class KMeansModel:
    """Fitted k-means centres, (k, n_features), held as float64."""

    def __init__(self, centers):
        self.centers = np.ascontiguousarray(centers, np.float64)
        if self.centers.ndim != 2 or self.centers.shape[0] < 1 or self.centers.shape[1] < 1:
            raise ValueError('KMeansModel: centers must be (k, n_features)')
        self.n_features = self.centers.shape[1]
        self._device = {}

    @classmethod
    def from_sklearn(cls, clf):
        names = {c.__name__ for c in type(clf).__mro__}
        if not names & set(KMEANS):
            raise NotImplementedError(_SUPPORTED + 'Got %s.' % type(clf).__name__)
        from sklearn.utils.validation import check_is_fitted
        check_is_fitted(clf)
        return cls(clf.cluster_centers_)

    def _on(self, dev):
        import torch
        if dev not in self._device:
            self._device[dev] = torch.from_numpy(self.centers).to(dev)
        return self._device[dev]


def _numeric_classes(classes):
    classes = np.asarray(classes)
    if classes.dtype.kind not in 'iufb':
        raise NotImplementedError(_SUPPORTED + 'classes_ of type %s are not numeric.' % classes.dtype)
    return np.ascontiguousarray(classes, np.float64)


def _is_sparse(a):
    return hasattr(a, 'toarray') and not isinstance(a, np.ndarray)


class KNNModel:
    """A fitted k-nearest-neighbours classifier as arrays (uniform weights, Euclidean metric).
    train : (n_train, n_features) the fitted samples, held as float64
    target : (n_train,) each sample's index into `classes`
    classes : (n_classes,) numeric classes_
    n_neighbors : 1 .. min(32, n_train)"""

    def __init__(self, train, target, classes, n_neighbors):
        if _is_sparse(train):
            raise NotImplementedError(_SUPPORTED + 'Got sparse training data.')
        self.train = np.ascontiguousarray(train, np.float64)
        self.target = np.ascontiguousarray(target, np.int64)
        self.classes = _numeric_classes(classes)
        if self.train.ndim != 2 or self.train.shape[0] < 1 or self.train.shape[1] < 1:
            raise ValueError('KNNModel: train must be (n_train, n_features)')
        if self.target.ndim == 2 and self.train.shape[0] == self.target.shape[0]:
            raise NotImplementedError(_SUPPORTED + 'Got a multi-output target.')
        if self.target.shape != (self.train.shape[0],) or self.classes.ndim != 1 or self.classes.size < 1:
            raise ValueError('KNNModel: target must be (n_train,) and classes (n_classes,)')
        if self.target.min() < 0 or self.target.max() >= self.classes.size:
            raise ValueError('KNNModel: a target lies outside classes')
        if not np.isfinite(self.train).all():
            raise ValueError('KNNModel: a training sample is not finite')
        if self.train.shape[0] >= 2 ** 31:
            raise ValueError('KNNModel: too many training samples')
        k = int(n_neighbors)
        if k != n_neighbors or not 1 <= k <= self.train.shape[0]:
            raise ValueError('KNNModel: n_neighbors = %r for %d training samples' % (n_neighbors, self.train.shape[0]))
        if k > KNN_MAX_K:
            raise NotImplementedError(_SUPPORTED + 'Got n_neighbors=%d.' % k)
        self.n_neighbors = k
        self.n_features = self.train.shape[1]
        self._device = {}

    n_train = property(lambda self: self.train.shape[0])
    n_classes = property(lambda self: self.classes.size)

    @classmethod
    def from_sklearn(cls, clf):
        names = {c.__name__ for c in type(clf).__mro__}
        if not names & set(KNN):
            raise NotImplementedError(_SUPPORTED + 'Got %s.' % type(clf).__name__)
        from sklearn.utils.validation import check_is_fitted
        check_is_fitted(clf)
        if clf.weights not in (None, 'uniform'):
            raise NotImplementedError(_SUPPORTED + 'Got weights=%r.' % (clf.weights,))
        metric, params = clf.effective_metric_, getattr(clf, 'effective_metric_params_', None) or {}
        if not (metric == 'euclidean' or (metric == 'minkowski' and params.get('p', 2) == 2
                                          and params.get('w') is None)):
            raise NotImplementedError(_SUPPORTED + 'Got metric=%r %r.' % (metric, params))
        if getattr(clf, 'outputs_2d_', False) or np.ndim(clf._y) != 1:
            raise NotImplementedError(_SUPPORTED + 'Got a multi-output %s.' % type(clf).__name__)
        if _is_sparse(clf._fit_X):
            raise NotImplementedError(_SUPPORTED + 'Got sparse training data.')
        return cls(clf._fit_X, clf._y, clf.classes_, clf.n_neighbors)

    def _on(self, dev):
        import torch
        if dev not in self._device:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._device[dev] = (up(self.train), up(self.target.astype(np.int32)), up(self.classes))
        return self._device[dev]


class LinearModel:
    """A fitted linear classifier as arrays.
    coef : (n_rows, n_features) float64; a binary model has one row
    intercept : (n_rows,) float64 (a scalar is repeated)
    classes : numeric classes_: 2 for one row, else n_rows
    link : what predict_proba applies to the decision values: 'none' (no predict_proba), 'softmax' or
        'ovr' (expit, normalised over the classes when there are more than two)"""

    def __init__(self, coef, intercept, classes, link='none'):
        if _is_sparse(coef):
            raise NotImplementedError(_SUPPORTED + 'Got a sparse coef_.')
        self.coef = np.array(coef, np.float64, order='C')         # a copy: partial_fit changes coef_ in place
        self.classes = _numeric_classes(classes)
        if self.coef.ndim != 2 or self.coef.shape[0] < 1 or self.coef.shape[1] < 1:
            raise ValueError('LinearModel: coef must be (n_rows, n_features)')
        n = self.coef.shape[0]
        self.intercept = np.ascontiguousarray(np.broadcast_to(np.asarray(intercept, np.float64).reshape(-1), (n,)))
        if self.classes.shape != ((2,) if n == 1 else (n,)):
            raise ValueError('LinearModel: %d rows of coefficients need %d classes, got %s'
                             % (n, 2 if n == 1 else n, self.classes.shape))
        if link not in ('none', 'softmax', 'ovr'):
            raise ValueError("LinearModel: link must be 'none', 'softmax' or 'ovr'")
        self.link = link
        self.n_features = self.coef.shape[1]
        self._device = {}

    n_classes = property(lambda self: self.classes.size)

    @classmethod
    def from_sklearn(cls, clf):
        names = {c.__name__ for c in type(clf).__mro__}
        if not names & set(LINEAR_PROBA + LINEAR_PREDICT):
            raise NotImplementedError(_SUPPORTED + 'Got %s.' % type(clf).__name__)
        from sklearn.utils.validation import check_is_fitted
        check_is_fitted(clf)
        if _is_sparse(clf.coef_):
            raise NotImplementedError(_SUPPORTED + 'Got a sparse coef_.')
        classes = clf.classes_
        if isinstance(classes, list) or np.ndim(classes) != 1 or np.ndim(clf.coef_) != 2:
            raise NotImplementedError(_SUPPORTED + 'Got a multi-output %s.' % type(clf).__name__)
        n = 1 if len(classes) <= 2 else len(classes)
        if clf.coef_.shape[0] != n:      # RidgeClassifier on a label indicator matrix: one row per output
            raise NotImplementedError(_SUPPORTED + 'Got a multi-output %s.' % type(clf).__name__)
        link = 'none'
        if names & set(LINEAR_PROBA):
            # LogisticRegression.predict_proba (scikit-learn 1.7.2)
            multi_class = getattr(clf, 'multi_class', 'deprecated')
            ovr = multi_class in ('ovr', 'warn') or (multi_class in ('auto', 'deprecated') and
                                                      (len(classes) <= 2 or clf.solver == 'liblinear'))
            link = 'ovr' if ovr else 'softmax'
        return cls(clf.coef_, clf.intercept_, classes, link)

    def _on(self, dev):
        import torch
        if dev not in self._device:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._device[dev] = (up(self.coef), up(self.intercept), up(self.classes))
        return self._device[dev]


def _fitted_state(clf):
    """what a model was built from: ('trees', the tree_ objects in estimator order), ('centres', a copy of
    cluster_centers_), ('knn', the fitted samples and targets themselves, and n_neighbors) or ('linear',
    copies of coef_ and intercept_); None for an estimator that holds none of them (unfitted)"""
    if hasattr(clf, 'estimators_'):
        return 'trees', [getattr(e, 'tree_', None) for e in clf.estimators_]
    if getattr(clf, 'tree_', None) is not None:
        return 'trees', [clf.tree_]
    if getattr(clf, 'cluster_centers_', None) is not None:
        return 'centres', np.array(clf.cluster_centers_, copy=True)
    if getattr(clf, '_fit_X', None) is not None:
        return 'knn', (clf._fit_X, getattr(clf, '_y', None), getattr(clf, 'n_neighbors', None))
    if getattr(clf, 'coef_', None) is not None and not _is_sparse(clf.coef_):
        return 'linear', (np.array(clf.coef_, copy=True), np.array(getattr(clf, 'intercept_', 0.0), copy=True))
    return None


def _same_state(a, b):
    if a is None or b is None or a[0] != b[0]:
        return False
    if a[0] == 'trees':
        return len(a[1]) == len(b[1]) and all(x is y and x is not None for x, y in zip(a[1], b[1]))
    if a[0] == 'knn':
        return a[1][0] is b[1][0] and a[1][1] is b[1][1] and a[1][1] is not None and a[1][2] == b[1][2]
    if a[0] == 'linear':
        return all(x.shape == y.shape and x.dtype == y.dtype and bool(np.array_equal(x, y))
                   for x, y in zip(a[1], b[1]))
    return a[1].shape == b[1].shape and a[1].dtype == b[1].dtype and bool(np.array_equal(a[1], b[1]))


def _model_for(clf, func, build=True):
    """the model of a fitted estimator for `func`; build=False only checks that the pair is served"""
    names = {c.__name__ for c in type(clf).__mro__}
    if isinstance(clf, DeviceKMeans):
        if func != 'predict':
            raise NotImplementedError(_SUPPORTED + 'Got func=%r for %s.' % (func, type(clf).__name__))
        return clf._model() if build else None
    if names & set(FORESTS):
        if func not in ('predict', 'predict_proba'):
            raise NotImplementedError(_SUPPORTED + 'Got func=%r.' % func)
        return ForestModel.from_sklearn(clf) if build else None
    if names & set(KMEANS):
        if func != 'predict':
            raise NotImplementedError(_SUPPORTED + 'Got func=%r for %s.' % (func, type(clf).__name__))
        return KMeansModel.from_sklearn(clf) if build else None
    if names & set(KNN):
        if func not in ('predict', 'predict_proba'):
            raise NotImplementedError(_SUPPORTED + 'Got func=%r for %s.' % (func, type(clf).__name__))
        return KNNModel.from_sklearn(clf) if build else None
    if names & set(LINEAR_PROBA + LINEAR_PREDICT):
        served = ('predict', 'predict_proba') if names & set(LINEAR_PROBA) else ('predict',)
        if func not in served:
            raise NotImplementedError(_SUPPORTED + 'Got func=%r for %s.' % (func, type(clf).__name__))
        return LinearModel.from_sklearn(clf) if build else None
    raise NotImplementedError(_SUPPORTED + 'Got %s.' % type(clf).__name__)


# ---------------------------------------------------------------------------
# layout: which element is feature f of row r
# ---------------------------------------------------------------------------
def _data_dims(ds, feature_dims):
    """nd/classify.py:62-65, the order of the dimension coordinates; without them (xr_lite), the first
    variable's dimension order"""
    every = [d for d in ds.dims if d not in feature_dims]
    dims = [d for d in ds.coords if d in every]
    if set(dims) == set(every):
        return tuple(dims)
    if _adapter.namespace(ds) is not xr_lite:
        raise ValueError('dimensions %s have no coordinates' % sorted(set(every) - set(dims)))
    if isinstance(ds, xr_lite.DataArray):
        return tuple(every)
    first = next(iter(ds.data_vars.values()))
    return tuple([d for d in first.dims if d in every] + [d for d in every if d not in first.dims])


def _variables(ds, data_dims):
    ns = _adapter.namespace(ds)
    if isinstance(ds, ns.DataArray):
        return [ds]
    names = _adapter.get_vars_for_dims(ds, data_dims)
    if not names:
        raise ValueError('no variable spans the data dimensions %s' % (data_dims,))
    return [ds[n] for n in names]


class _Layout:
    """The feature table of a dataset: device views, one per feature, that share the row strides."""

    def __init__(self, ds, feature_dims):
        import torch
        feature_dims = tuple(feature_dims)
        self.ns = _adapter.namespace(ds)
        self.data_dims = _data_dims(ds, feature_dims)
        if len(self.data_dims) > 4:
            raise ValueError('at most four data dimensions, got %s' % (self.data_dims,))
        variables = _variables(ds, self.data_dims)
        values = [v.values for v in variables]
        for v in values:
            if _device.np_dtype(v).kind == 'c':
                raise TypeError('Classifier: complex variables cannot be features; split them into real ones '
                                'first (disassemble_complex)')
            if _device.np_dtype(v).kind not in 'fiub' or _device.np_dtype(v) == np.float16:
                raise TypeError('Classifier: unsupported dtype %s' % _device.np_dtype(v))
        self.host = not any(_device.is_tensor(v) and v.is_cuda for v in values)
        self.device = _device.device_of(*values)
        sizes = ds.sizes
        self.shape = tuple(int(sizes[d]) for d in self.data_dims)
        self.coords = OrderedDict((d, ds.coords[d]) for d in self.data_dims if d in ds.coords)
        fdims = [d for d in feature_dims if d in ds.dims]
        fshape = [int(sizes[d]) for d in fdims]
        all32 = all(_device.np_dtype(v) == np.float32 for v in values)
        dtype = torch.float32 if all32 else torch.float64
        self.np_dtype = np.dtype(np.float32 if all32 else np.float64)
        with torch.cuda.device(self.device):
            views = []
            for da, v in zip(variables, values):
                t = _device.to_device(v, self.device)
                t = t if t.dtype == dtype else t.to(dtype)
                own = [d for d in fdims if d in da.dims]
                t = t.permute(*[da.dims.index(d) for d in own + list(self.data_dims)])
                views.append((t, own))
            nrow = len(self.data_dims)
            strides = {tuple(s for s, n in zip(t.stride()[t.dim() - nrow:], self.shape) if n > 1) for t, _ in views}
            if len(strides) > 1:
                views = [(t.contiguous(), own) for t, own in views]
            t0 = views[0][0]
            self.strides = tuple(int(s) for s in t0.stride()[t0.dim() - nrow:])
            # feature = (position along feature_dims) * n_variables + variable; a variable without one of the
            # feature dimensions is the same at every position along it, as xarray's to_array broadcasts it
            self.features = []
            for pos in np.ndindex(*fshape):
                for t, own in views:
                    idx = tuple(p for p, d in zip(pos, fdims) if d in own)
                    self.features.append(t[idx] if idx else t)
        self.n_features = len(self.features)

    def label_args(self, labels):
        """labels squeezed and broadcast over the data dimensions they lack (_broadcast_labels,
        nd/classify.py:74-100) -> (float64 device tensor, element strides per data dimension, label dtype)"""
        import torch
        if hasattr(labels, 'data_vars'):
            raise ValueError("`labels` should be an xarray.DataArray or numpy array of the same dimensions "
                             "as the dataset.")
        if hasattr(labels, 'dims') and hasattr(labels, 'values'):
            vals, dims = labels.values, tuple(labels.dims)
            keep = [i for i, n in enumerate(vals.shape) if n != 1]
            vals = vals.reshape([vals.shape[i] for i in keep])
            dims = [dims[i] for i in keep]
            extra = set(dims) - set(self.data_dims)
            if extra:
                raise ValueError('labels have dimensions %s the data lacks' % sorted(extra))
            for d, n in zip(dims, vals.shape):
                if n != self.shape[self.data_dims.index(d)]:
                    raise ValueError('labels have size %d along %s, the data %d'
                                     % (n, d, self.shape[self.data_dims.index(d)]))
            t = self._label_tensor(vals)
            strides = [t.stride(dims.index(d)) if d in dims else 0 for d in self.data_dims]
        else:
            vals = labels if _device.is_tensor(labels) else np.asarray(labels)
            vals = vals.reshape([n for n in vals.shape if n != 1])
            matching = list(self.shape)
            new_shape = [1] * len(matching)
            for n in vals.shape:
                i = matching.index(n)          # ValueError where no dimension has that size, as the reference
                new_shape[i] = n
                matching[i] = None
            t = self._label_tensor(vals).reshape(new_shape)
            strides = [t.stride(i) if new_shape[i] != 1 else 0 for i in range(len(new_shape))]
        strides = [s if n > 1 else 0 for s, n in zip(strides, self.shape)]
        return t, strides, _device.np_dtype(vals)

    def _label_tensor(self, vals):
        import torch
        with torch.cuda.device(self.device):
            return _device.to_device(vals, self.device).to(torch.float64).contiguous()

    def wrap(self, values, extra_dim=None):
        """values over the data dimensions (+ extra_dim) -> a DataArray of the input's kind"""
        dims = self.data_dims + ((extra_dim,) if extra_dim else ())
        coords = OrderedDict(self.coords)
        if extra_dim:
            coords[extra_dim] = np.arange(values.shape[-1])
        if self.host:
            values = _device.to_host(values)
        if self.ns is xr_lite:
            return xr_lite.DataArray(values, dims, coords)
        return self.ns.DataArray(values, dims=dims, coords=coords)


def _scaler_arrays(scaler):
    if scaler is None:
        return None, None
    mean, scale = getattr(scaler, 'mean_', None), getattr(scaler, 'scale_', None)
    if mean is None or scale is None:
        raise NotImplementedError('nd_amd.classify: the device scaler needs a StandardScaler with mean_ and scale_')
    return np.asarray(mean, np.float64), np.asarray(scale, np.float64)


def _check_features(layout, model):
    if layout.n_features != model.n_features:
        raise ValueError('the model was fitted on %d features, the dataset gives %d'
                         % (model.n_features, layout.n_features))


def predict_forest(ds, model, feature_dims=(), func='predict', scaler=None):
    """`model` (a ForestModel) applied to every pixel of `ds` on the device.  func: 'predict' or
    'predict_proba'.  scaler: None, or an object with mean_ and scale_ (a fitted StandardScaler).
    Returns a float64 DataArray over the data dimensions (with a trailing `label` dimension for
    predict_proba), NaN where any feature of the pixel is NaN."""
    from . import kernels
    if func not in ('predict', 'predict_proba'):
        raise NotImplementedError(_SUPPORTED + 'Got func=%r.' % func)
    layout = _Layout(ds, feature_dims)
    _check_features(layout, model)
    mean, scale = _scaler_arrays(scaler)
    nodes, values, roots, classes = model._on(layout.device)
    proba = func == 'predict_proba'
    labels, p = kernels.classify_forest(layout.features, layout.shape, layout.strides, nodes, values, roots,
                                        classes, mean, scale, want_labels=not proba, want_proba=proba)
    return layout.wrap(p, 'label') if proba else layout.wrap(labels)


def predict_kmeans(ds, model, feature_dims=(), scaler=None):
    """The index of the nearest centre of `model` (a KMeansModel) for every pixel of `ds`, the first
    where several are equally near; distances are summed in float64 in feature order.  Returns a float64
    DataArray over the data dimensions, NaN where any feature is NaN."""
    from . import kernels
    layout = _Layout(ds, feature_dims)
    _check_features(layout, model)
    mean, scale = _scaler_arrays(scaler)
    labels = kernels.classify_kmeans(layout.features, layout.shape, layout.strides, model._on(layout.device),
                                     mean, scale)
    return layout.wrap(labels)


def predict_knn(ds, model, feature_dims=(), func='predict', scaler=None):
    """`model` (a KNNModel) applied to every pixel of `ds` on the device.  func: 'predict' or 'predict_proba'.
    The neighbours of a pixel are the n_neighbors training samples smallest by (squared distance in float64,
    summed in feature order; training index): predict_proba is count_c / n_neighbors, predict the first class
    with the largest count.  Returns a float64 DataArray over the data dimensions (with a trailing `label`
    dimension for predict_proba), NaN where any feature of the pixel is NaN."""
    from . import kernels
    if func not in ('predict', 'predict_proba'):
        raise NotImplementedError(_SUPPORTED + 'Got func=%r.' % func)
    layout = _Layout(ds, feature_dims)
    _check_features(layout, model)
    if layout.n_features > KNN_MAX_FEATURES:
        raise NotImplementedError(_SUPPORTED + 'Got %d features.' % layout.n_features)
    mean, scale = _scaler_arrays(scaler)
    train, target, classes = model._on(layout.device)
    proba = func == 'predict_proba'
    labels, p = kernels.classify_knn(layout.features, layout.shape, layout.strides, train, target, classes,
                                     model.n_neighbors, mean, scale, want_labels=not proba, want_proba=proba)
    return layout.wrap(p, 'label') if proba else layout.wrap(labels)


def predict_linear(ds, model, feature_dims=(), func='predict', scaler=None):
    """`model` (a LinearModel) applied to every pixel of `ds` on the device.  func: 'predict',
    'predict_proba' (a model with a link) or 'decision_function' (s_c = b_c + sum_f x_f w_cf in float64,
    summed in feature order, with a trailing `label` dimension of one entry per row of coefficients).
    Returns a float64 DataArray over the data dimensions, NaN where any feature of the pixel is NaN."""
    from . import kernels
    if func not in ('predict', 'predict_proba', 'decision_function') or (func == 'predict_proba'
                                                                          and model.link == 'none'):
        raise NotImplementedError(_SUPPORTED + 'Got func=%r.' % func)
    layout = _Layout(ds, feature_dims)
    _check_features(layout, model)
    mean, scale = _scaler_arrays(scaler)
    coef, intercept, classes = model._on(layout.device)
    out = kernels.classify_linear(layout.features, layout.shape, layout.strides, coef, intercept, classes,
                                  model.link, func, mean, scale)
    return layout.wrap(out) if func == 'predict' else layout.wrap(out, 'label')


# ---------------------------------------------------------------------------
# k-means trained on the device
# ---------------------------------------------------------------------------
KMEANS_FIT_MAX_ACC = 4096


def _moments(layout, mean=None, scale=None):
    """-> (valid rows, mean, var) of the layout's features as host values (kernels.feature_moments)"""
    from . import kernels
    count, fmean, fvar = kernels.feature_moments(layout.features, layout.shape, layout.strides, mean, scale)
    return int(count.item()), fmean.cpu().numpy(), fvar.cpu().numpy()


def _device_scaler(layout):
    """a StandardScaler as StandardScaler().fit(X) leaves it, from the device's moments of every valid row"""
    from sklearn import preprocessing
    n, mean, var = _moments(layout)
    if n < 1:
        raise ValueError('no row without NaN to fit the scaler on')
    sc = preprocessing.StandardScaler()
    sc.mean_, sc.var_ = mean, var
    scale = np.sqrt(var)
    scale[scale == 0.0] = 1.0            # a constant feature is left as it is, as scikit-learn leaves it
    sc.scale_ = scale
    sc.n_samples_seen_ = n
    sc.n_features_in_ = layout.n_features
    return sc


def _valid_rows(layout, index, mean, scale):
    """the rows at `index` (host int64) without NaN -> (X as float64 on the host, their indices)"""
    import torch
    from . import kernels
    idx = torch.from_numpy(np.ascontiguousarray(index, np.int64)).to(layout.device)
    X, valid = kernels.gather_rows(layout.features, layout.shape, layout.strides, idx, mean, scale)
    keep = valid.cpu().numpy().astype(bool)
    return X.cpu().numpy().astype(np.float64)[keep], np.asarray(index)[keep]


def _initial_centres(layout, k, init, rng, init_size, mean, scale):
    rows = int(np.prod(layout.shape, dtype=np.int64))
    if init == 'random':
        need, chosen = k, np.empty((0, layout.n_features))
        seen = set()
        for _ in range(8):                          # rows with NaN are drawn again
            draw = rng.choice(rows, size=min(rows, 2 * need + 64), replace=False)
            draw = np.array([i for i in draw if i not in seen], np.int64)
            seen.update(draw.tolist())
            X, _ = _valid_rows(layout, draw, mean, scale)
            chosen = np.concatenate([chosen, X[:need]])
            need = k - chosen.shape[0]
            if need == 0 or len(seen) >= rows:
                break
        if need:
            raise ValueError('fit_kmeans: fewer than %d rows without NaN to draw the centres from' % k)
        return chosen
    if init == 'k-means++':
        size = min(rows, max(3 * k, 65536) if init_size is None else int(init_size))
        draw = np.arange(rows) if size >= rows else rng.choice(rows, size=size, replace=False)
        X, _ = _valid_rows(layout, draw, mean, scale)
        if X.shape[0] < k:
            raise ValueError('fit_kmeans: the sample of %d rows has %d without NaN, fewer than n_clusters=%d'
                             % (size, X.shape[0], k))
        from sklearn.cluster import kmeans_plusplus
        return kmeans_plusplus(X, k, random_state=int(rng.integers(2 ** 31 - 1)))[0]
    raise ValueError("fit_kmeans: init must be 'k-means++', 'random' or a (k, n_features) array, got %r" % (init,))


def _lloyd(layout, centres, max_iter, threshold, mean, scale):
    """scikit-learn 1.7.2's _kmeans_single_lloyd in float64, the pass over the rows on the device.
    -> (centres, n_iter, inertia, counts)"""
    import torch
    from . import kernels
    dev = layout.device
    k, nfeat = centres.shape
    labels = torch.full(layout.shape, -1, dtype=torch.int32, device=dev)

    def step(c):
        sums, counts, inertia, changed = kernels.kmeans_step(layout.features, layout.shape, layout.strides,
                                                             torch.from_numpy(c).to(dev), labels, mean, scale)
        # the one read of an iteration: k * n_features + k + 2 numbers (a count is exact in float64 below 2^53)
        got = torch.cat([sums.reshape(-1), inertia.reshape(1), counts.double(), changed.double().reshape(1)])
        got = got.cpu().numpy()
        return (got[:k * nfeat].reshape(k, nfeat), got[k * nfeat + 1:-1].astype(np.int64), float(got[k * nfeat]),
                int(got[-1]))

    strict, n_iter = False, 0
    counts, inertia = np.zeros(k, np.int64), 0.0
    for n_iter in range(1, max_iter + 1):
        sums, counts, inertia, changed = step(centres)
        new = centres.copy()
        full = counts > 0                      # an empty cluster keeps its centre (scikit-learn relocates it)
        new[full] = sums[full] / counts[full, None]
        shift = float(((new - centres) ** 2).sum())
        centres = new
        if changed == 0:
            strict = True
            break
        if shift <= threshold:
            break
    if not strict:                             # labels, counts and inertia of the final centres
        _, counts, inertia, _ = step(centres)
    return centres, n_iter, inertia, counts


def _fit_kmeans(layout, n_clusters, init, n_init, max_iter, tol, random_state, scaler, init_size):
    k = int(n_clusters)
    if k != n_clusters or k < 1:
        raise ValueError('fit_kmeans: n_clusters = %r' % (n_clusters,))
    if int(max_iter) < 1 or int(n_init) < 1:
        raise ValueError('fit_kmeans: max_iter and n_init must be at least 1')
    if k * (layout.n_features + 1) > KMEANS_FIT_MAX_ACC:
        raise NotImplementedError('nd_amd.classify fits k-means on the device for n_clusters * (n_features + 1) <= %d; '
                                  'got n_clusters=%d and %d features.  There is no CPU fallback.'
                                  % (KMEANS_FIT_MAX_ACC, k, layout.n_features))
    import torch
    mean, scale = _scaler_arrays(scaler)
    if mean is not None:                       # uploaded once for every pass
        mean, scale = (torch.from_numpy(np.ascontiguousarray(v)).to(layout.device) for v in (mean, scale))
    n, _, var = _moments(layout, mean, scale)
    if n < k:
        raise ValueError('fit_kmeans: %d rows without NaN for n_clusters=%d' % (n, k))
    threshold = float(tol) * float(np.mean(var))
    if not isinstance(init, str):
        init = np.array(init, np.float64, order='C')
        if init.shape != (k, layout.n_features):
            raise ValueError('fit_kmeans: init must be (%d, %d), got %s' % (k, layout.n_features, init.shape))
        n_init = 1
    rng = random_state if isinstance(random_state, np.random.Generator) else np.random.default_rng(random_state)
    best = None
    for _ in range(int(n_init)):
        start = init if not isinstance(init, str) else np.ascontiguousarray(
            _initial_centres(layout, k, init, rng, init_size, mean, scale), np.float64)
        run = _lloyd(layout, start, int(max_iter), threshold, mean, scale)
        if best is None or run[2] < best[2]:
            best = run
    model = KMeansModel(best[0])
    model.n_iter, model.inertia, model.counts = best[1], best[2], best[3]
    model.empty = np.flatnonzero(best[3] == 0)
    return model


def fit_kmeans(ds, n_clusters, feature_dims=(), init='k-means++', n_init=1, max_iter=300, tol=1e-4,
               random_state=None, scaler=None, init_size=None):
    """K-means over every pixel of `ds` without a NaN feature, trained on the device: scikit-learn 1.7.2's Lloyd
    loop restated in float64.  Per iteration one pass assigns every row to its first nearest centre (the rule of
    predict_kmeans) and sums the rows of every cluster in a fixed order; the new centre is sums / counts.  It
    stops when no label changed ("strict convergence"), when sum((new - old)^2) <= tol * mean(var), var the
    population variances of the features, or after max_iter iterations; unless the stop was strict one more
    pass gives the counts and the inertia of the final centres.  Nothing of the size of the data leaves the
    device, and the same inputs give the same bits.
    init: a (n_clusters, n_features) array (forces n_init = 1), 'random' (distinct rows drawn with
    random_state) or 'k-means++' (sklearn.cluster.kmeans_plusplus on a drawn sample of init_size rows, default
    max(3 * n_clusters, 65536)).  With n_init > 1 the run of the lowest inertia wins.
    scaler: None, or an object with mean_ and scale_; the centres are then those of the scaled features.
    Unlike scikit-learn, a cluster that loses all its rows keeps its centre; such clusters are listed in `.empty`.
    -> a KMeansModel with .centers, .n_iter, .inertia, .counts and .empty.
    Serves n_clusters * (n_features + 1) <= 4096; more raises NotImplementedError (there is no CPU fallback)."""
    return _fit_kmeans(_Layout(ds, feature_dims), n_clusters, init, n_init, max_iter, tol, random_state, scaler,
                       init_size)


class DeviceKMeans:
    """The estimator Classifier trains on the device: Classifier(DeviceKMeans(8)).fit_predict(ds) clusters every
    pixel of `ds` through fit_kmeans, without the (n_pixels, n_features) matrix.  Parameters as
    sklearn.cluster.KMeans; see fit_kmeans for `init` and for the one difference (empty clusters)."""

    def __init__(self, n_clusters=8, init='k-means++', n_init=1, max_iter=300, tol=1e-4, random_state=None):
        self.n_clusters, self.init, self.n_init = n_clusters, init, n_init
        self.max_iter, self.tol, self.random_state = max_iter, tol, random_state
        self.cluster_centers_ = self.n_iter_ = self.inertia_ = None

    def get_params(self, deep=True):
        return {p: getattr(self, p) for p in ('n_clusters', 'init', 'n_init', 'max_iter', 'tol', 'random_state')}

    def _fit_layout(self, layout, scaler):
        model = _fit_kmeans(layout, self.n_clusters, self.init, self.n_init, self.max_iter, self.tol,
                            self.random_state, scaler, None)
        self.cluster_centers_, self.n_iter_, self.inertia_ = model.centers, model.n_iter, model.inertia

    def _model(self):
        if self.cluster_centers_ is None:
            raise AttributeError('DeviceKMeans is not fitted: call Classifier.fit first')
        return KMeansModel(self.cluster_centers_)

    def predict(self, X):
        """the first nearest centre of every row of the matrix X (n, n_features), on the device; NaN for a row
        with a NaN feature"""
        import torch
        from . import kernels
        model = self._model()
        X = np.asarray(X)
        X = np.ascontiguousarray(X, np.float32 if X.dtype == np.float32 else np.float64)
        if X.ndim != 2 or X.shape[1] != model.n_features:
            raise ValueError('DeviceKMeans.predict: X must be (n, %d)' % model.n_features)
        dev = _device.device_of(X)
        with torch.cuda.device(dev):
            t = torch.from_numpy(X).to(dev)
            labels = kernels.classify_kmeans([t[:, f] for f in range(X.shape[1])], (X.shape[0],), (X.shape[1],),
                                             model._on(dev))
        return labels.cpu().numpy()


# ---------------------------------------------------------------------------
# nd.classify.Classifier
# ---------------------------------------------------------------------------
class Classifier:
    """
    Parameters
    ----------
    clf : sklearn classifier
        An initialized classifier object as provided by ``scikit-learn``.  Must provide ``fit``; see the
        module docstring for the estimators ``predict`` serves.
    feature_dims : list, optional
        Additional dimensions to use as features: with ``'time'`` every time step is an independent
        variable; otherwise time steps are further data dimensions like ``'x'`` and ``'y'``.
    scale : bool, optional
        If True, scale the input data to zero mean and unit variance (default: False).

    Fitting (``clf.fit``, ``StandardScaler().fit``) is scikit-learn's, on the host, on the labelled pixels
    only: it is not a hot path.  Selecting and gathering those pixels, and ``predict``, run on the device.
    With a ``DeviceKMeans`` as `clf`, ``fit(ds)`` trains on every pixel on the device (``fit_kmeans``), the
    scaler included, and forms no matrix.
    """

    def __init__(self, clf, feature_dims=[], scale=False):
        self.clf = clf
        self.feature_dims = feature_dims
        self.scale = scale
        self._scaler = None
        self._model = None          # (clf, the fitted state it was built from, model): see _cached_model

    def make_Xy(self, ds, labels=None):
        """scikit-learn compatible X and y (numpy arrays, X in the data's type) from `ds` and `labels`
        (a DataArray or numpy array; pixels whose label is NaN or <= 0, or with a NaN feature, are left
        out).  The rows are selected and gathered on the device; only they reach the host."""
        from . import kernels
        layout = _Layout(ds, self.feature_dims)
        lab = strides = ldtype = None
        if labels is not None:
            lab, strides, ldtype = layout.label_args(labels)
        X, y, _ = kernels.classify_gather(layout.features, layout.shape, layout.strides, lab, strides)
        X = np.asarray(_device.to_host(X))
        y = np.asarray(_device.to_host(y)).astype(ldtype) if y is not None else None
        if self.scale:
            from sklearn import preprocessing
            self._scaler = preprocessing.StandardScaler()
            self._scaler.fit(X)
            X = self._scaler.transform(X)
        return (X, y)

    def fit(self, ds, labels=None):
        """Train the classifier with scikit-learn on the pixels make_Xy selects (labels may be omitted for
        an unsupervised estimator such as KMeans)."""
        if isinstance(self.clf, DeviceKMeans):
            if labels is not None:
                raise TypeError('Classifier: DeviceKMeans is unsupervised and takes no labels')
            layout = _Layout(ds, self.feature_dims)
            self._scaler = _device_scaler(layout) if self.scale else None
            self._model = None
            self.clf._fit_layout(layout, self._scaler)
            return self
        X, y = self.make_Xy(ds, labels=labels)
        self._model = None
        self.clf.fit(X, y)
        return self

    def predict(self, ds, func='predict'):
        """The predicted class labels of every pixel (func='predict'), or the class probabilities with a
        trailing `label` dimension (func='predict_proba'), computed on the device: a float64 DataArray over
        the data dimensions, NaN where any feature is NaN."""
        if func not in dir(self.clf):
            raise AttributeError('Classifier has no method {}.'.format(func))
        model = self._cached_model(func)
        scaler = None
        if self.scale:
            if self._scaler is None:
                raise AttributeError('Classifier(scale=True) has no fitted scaler: call fit first')
            scaler = self._scaler
        if isinstance(model, ForestModel):
            return predict_forest(ds, model, self.feature_dims, func, scaler)
        if isinstance(model, KNNModel):
            return predict_knn(ds, model, self.feature_dims, func, scaler)
        if isinstance(model, LinearModel):
            return predict_linear(ds, model, self.feature_dims, func, scaler)
        return predict_kmeans(ds, model, self.feature_dims, scaler)

    def _cached_model(self, func):
        """The arrays of the fitted estimator, packed and uploaded once while the fitted state stays what it
        was.  The state is compared by content where scikit-learn may change it in place: the tree objects
        of every estimator, one by one (warm_start extends estimators_ in place), a copy of the k-means
        centres and of a linear model's coef_ and intercept_ (partial_fit updates them in place).  A k-NN fit
        replaces _fit_X and _y, so they are compared by identity, with n_neighbors beside them."""
        clf = self.clf
        _model_for(clf, func, build=False)
        state = _fitted_state(clf)
        if self._model is not None and state is not None:
            old_clf, old_state, model = self._model
            if old_clf is clf and _same_state(state, old_state):
                return model
        model = _model_for(clf, func)
        self._model = (clf, state, model)
        return model

    def fit_predict(self, ds, labels=None):
        self.fit(ds, labels)
        return self.predict(ds)

    def score(self, ds, labels=None, method='accuracy'):
        """The classification score (a scikit-learn scorer name) on the labelled pixels.  As in the
        reference this goes through make_Xy, which with scale=True re-fits the scaler on `ds`."""
        from sklearn import metrics
        try:
            scorer = metrics.get_scorer(method)
        except Exception:
            raise ValueError("'{}' is not a valid scoring method".format(method))
        X, y = self.make_Xy(ds, labels=labels)
        return scorer(self.clf, X, y)


# ---------------------------------------------------------------------------
# class_mean
# ---------------------------------------------------------------------------
def class_mean_fill(sums, counts, nans, dtype):
    """The closed form of the reference's loop (nd/classify.py:36-44) for one variable.  Round l gives every
    pixel of class l -- and every pixel of ANY class that is still NaN -- the mean m_l of the class's
    non-NaN pixels.  So the NaN pixels of a class take the first non-NaN mean of an earlier round and then
    count, at that value, in their own class's mean; a class whose mean is NaN ends at the first non-NaN
    mean after it.  -> fill values (n + 1,) of `dtype`: one per class, and the value NaN pixels of no
    class end at."""
    n = len(sums)
    fill = np.full(n + 1, np.nan, np.float64)
    first = np.nan
    for l in range(n):
        s, c = float(sums[l]), int(counts[l])
        if nans[l] and not np.isnan(first):
            s += int(nans[l]) * float(first)
            c += int(nans[l])
        m = np.dtype(dtype).type(s / c) if c else np.nan
        fill[l] = m
        if np.isnan(first) and not np.isnan(m):
            first = m
    fill[np.isnan(fill)] = first
    return fill.astype(dtype)


def _n_labels(vals):
    """len(np.unique(labels)), NaN counting once"""
    if _device.is_tensor(vals):
        import torch
        v = vals.reshape(-1)
        if v.is_floating_point():
            nan = torch.isnan(v)
            return int(torch.unique(v[~nan]).numel()) + int(bool(nan.any()))
        return int(torch.unique(v).numel())
    return len(np.unique(np.asarray(vals)))


def _class_label_strides(da, ldims, lshape, lstrides, name):
    """element strides of the labels along every dimension of the variable `da` (0 where they are broadcast).
    ldims: the labels' dimension names (matched by name, sizes must agree) or None for an array of shape
    `lshape` matched by size as _broadcast_array does.  lstrides None: only validate."""
    shape = tuple(da.shape)
    lstrides = lstrides if lstrides is not None else (0,) * len(lshape)
    if ldims is not None:
        missing = [d for d in ldims if d not in da.dims]
        if missing:
            raise ValueError('class_mean: variable %r lacks the label dimensions %s' % (name, missing))
        for d, size in zip(ldims, lshape):
            if size != shape[da.dims.index(d)]:
                raise ValueError('class_mean: labels have size %d along %s, variable %r has %d'
                                 % (size, d, name, shape[da.dims.index(d)]))
        return [lstrides[ldims.index(d)] if d in ldims else 0 for d in da.dims]
    matching, ls = list(shape), [0] * len(shape)
    for ax, size in enumerate(lshape):
        if size not in matching:
            raise ValueError('class_mean: no dimension of variable %r %s has the labels\' size %d'
                             % (name, shape, size))
        i = matching.index(size)
        ls[i], matching[i] = lstrides[ax], None
    return ls


def class_mean(ds, labels):
    """Replace every pixel of the dataset with the mean of its class (or cluster, or segment).

    ds : Dataset or DataArray.  labels : DataArray whose dimensions may be a subset of those of `ds`
    (such as ('y', 'x') against a stack with a 'time' dimension), or an array matched to the dimensions by
    size.  Returns an object like `ds` in the data's type (integers as float64).

    The reference's loop is reproduced with its consequences: with n = len(np.unique(labels)) only the
    labels 0 .. n-1 are classes, pixels with another label keep their value; a NaN pixel of any class takes
    the mean of the first class that has one (class 0 in the first round) and then counts, at that value,
    in its own class's mean.  Per-class sums are float64, formed on the device in one pass; a second pass
    fills."""
    import torch
    from . import kernels
    ns = _adapter.namespace(ds)
    single = isinstance(ds, ns.DataArray)
    variables = OrderedDict([(None, ds)]) if single else OrderedDict((k, ds[k]) for k in ds.data_vars)
    named = hasattr(labels, 'dims') and hasattr(labels, 'values')
    lvals = labels.values if named else (labels if _device.is_tensor(labels) else np.asarray(labels))
    # dimensions of size 1 are squeezed, as make_Xy squeezes them
    ldims = tuple(d for d, size in zip(labels.dims, lvals.shape) if size != 1) if named else None
    lvals = lvals.reshape([size for size in lvals.shape if size != 1])
    for name, da in variables.items():          # before any device work: a wrong extent would read past the labels
        _class_label_strides(da, ldims, tuple(lvals.shape), None, name)
    n = _n_labels(lvals)
    values = [v.values for v in variables.values()]
    host = not any(_device.is_tensor(v) and v.is_cuda for v in values)
    dev = _device.device_of(*values)
    out = OrderedDict()
    with torch.cuda.device(dev):
        lab = _device.to_device(lvals, dev).to(torch.float64).contiguous()
        for name, da in variables.items():
            v = da.values
            if _device.np_dtype(v).kind == 'c':
                raise TypeError('class_mean: complex variables are not supported (disassemble_complex)')
            t = _device.to_device(v, dev)
            if t.dtype not in (torch.float32, torch.float64):
                t = t.to(torch.float64)
            if torch.empty_like(t).stride() != t.stride():
                t = t.contiguous()
            ls = _class_label_strides(da, ldims, tuple(lab.shape), lab.stride(), name)
            s, c, k = kernels.class_stats(t, lab, ls, n)
            fill = class_mean_fill(s.cpu().numpy(), c.cpu().numpy(), k.cpu().numpy(), _device.np_dtype(t))
            res = kernels.class_fill(t, lab, ls, torch.from_numpy(fill).to(dev))
            out[name] = _device.to_host(res) if host else res
    if single:
        if ns is xr_lite:
            return xr_lite.DataArray(out[None], ds.dims, ds.coords, ds.attrs, ds.name)
        return ds.copy(data=out[None])
    if ns is xr_lite:
        res = xr_lite.Dataset(coords=ds.coords, attrs=ds.attrs)
        for k, v in out.items():
            res[k] = (tuple(ds[k].dims), v, ds[k].attrs)
        return res
    res = ds.copy()
    for k, v in out.items():
        res[k] = (ds[k].dims, v, ds[k].attrs)
    return res
