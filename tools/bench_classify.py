"""Classification timing on the headline stack (k x n x n, four variables from nd_amd.synth, device resident):

    python tools/bench_classify.py [--k 24] [--n 4096] [--reps 5] [--trees 20] [--knn-n N] [--json out.json]

  forest      Classifier(RandomForestClassifier(trees)).predict, fitted by scikit-learn on 10 % of a
              256 x 256 crop (labels: terciles of the crop's C11), at feature_dims=[] (k n^2 rows x 4 features)
              and feature_dims=['time'] (n^2 rows x 4 k features); node count and depth are recorded
  kmeans      Classifier(KMeans(3)).predict at feature_dims=[]
  class_mean  class_mean of the stack under the forest's (y, x) labels
  knn         Classifier(KNeighborsClassifier(3)).predict fitted on 1 000 and on 10 000 labelled pixels of the crop
              at feature_dims=[], and on 1 000 at feature_dims=['time'] (n^2 rows x 4 k features); the line also
              gives the kernel's float64 operations per second (3 per row, sample and feature: subtract,
              multiply, add) as a fraction of --fp64-peak
  logistic    Classifier(LogisticRegression()).predict, three classes, at feature_dims=[]
  kmeans fit  fit_kmeans(ds, 8, init=array) at feature_dims=[] and ['time']: the time of one Lloyd iteration (the
              kmeans_step kernels of a fit, from the library's timers) and of the whole fit (at most --fit-iters
              iterations), against scikit-learn's KMeans(8, init=array, n_init=1, algorithm='lloyd') on the matrix
              of --host-rows rows at 16 threads, per iteration and row; the line also gives the bytes a step must
              move (every feature once, the labels read and written) over its time as a fraction of --hbm-peak
              (--fit-only runs these lines alone and keeps the other rows of an existing --json file)

Every case: device events around whole calls, one warm-up, min and median of --reps; the kernels' own time from
the library's event timers (KernelTimer).  Yardstick, measured in the same run: the reference path on the host,
scikit-learn's predict on the (rows, features) matrix of a crop at 16 threads (n_jobs=16 for the forest), as
rows per second.  Building that matrix is not counted in the host's favour."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARS = ('C11', 'C12re', 'C12im', 'C22')


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return min(out), sorted(out)[len(out) // 2]


def kernel_ms(fn, name):
    from nd_amd import _lib
    _lib.timing_enable(64)
    fn()
    per = _lib.timing_collect()
    _lib.timing_enable(0)
    return sum(ms for n, ms in per if n == name)


def host_rate(predict, X, reps=3):
    predict(X[:1000])
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        predict(X)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return X.shape[0] / best


def main():
    import numpy as np
    import torch
    from sklearn.cluster import KMeans
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.linear_model import LogisticRegression
    from sklearn.neighbors import KNeighborsClassifier
    from nd_amd import classify, synth, xr_lite
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=24)
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--trees', type=int, default=20)
    ap.add_argument('--crop', type=int, default=256)
    ap.add_argument('--host-rows', type=int, default=2000000)
    ap.add_argument('--knn-host-rows', type=int, default=200000)
    ap.add_argument('--knn-n', type=int, default=None,
                    help='the k-NN lines predict on the leading knn-n x knn-n pixels of the stack (default: all '
                         'of it; the 10 000-sample line is 5e16 float64 operations there)')
    ap.add_argument('--knn-reps', type=int, default=1)
    ap.add_argument('--fp64-peak', type=float, default=78.6e12,
                    help='float64 vector operations per second the k-NN rate is set against (MI355X: 78.6e12)')
    ap.add_argument('--skip-knn', action='store_true')
    ap.add_argument('--fit-only', action='store_true')
    ap.add_argument('--fit-iters', type=int, default=50)
    ap.add_argument('--hbm-peak', type=float, default=8.0e12,
                    help='bytes per second the k-means step is set against (MI355X: 8.0e12)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    k, n, crop = a.k, a.n, min(a.crop, a.n)
    stack = synth.wishart_c2_stack(k, n, n, device=dev)
    dims = ('time', 'y', 'x')
    ds = xr_lite.Dataset()
    small = xr_lite.Dataset()
    for i, v in enumerate(VARS):
        ds[v] = (dims, stack[i])
        small[v] = (dims, stack[i][:, :crop, :crop])
    rng = np.random.default_rng(0)
    c11 = stack[0][:, :crop, :crop].mean(0).cpu().numpy()
    truth = 1 + (c11 > np.quantile(c11, 1 / 3)).astype(np.int64) + (c11 > np.quantile(c11, 2 / 3))
    train = np.where(rng.random(truth.shape) < 0.1, truth, 0)
    rows = []

    def record(case, nrows, nfeat, ms, kms, host, extra=None):
        row = dict(case=case, rows=nrows, features=nfeat, ms_min=ms[0], ms_median=ms[1], kernel_ms=kms,
                   device_rows_per_s=nrows / (ms[0] * 1e-3), host_rows_per_s=host,
                   device_over_host=nrows / (ms[0] * 1e-3) / host if host else None)
        row.update(extra or {})
        rows.append(row)
        print(json.dumps(row), flush=True)

    def kmeans_fit_lines():
        from nd_amd import _lib
        elem = stack[0].element_size()
        for fdims in ([], ['time']):
            Xh = classify.Classifier(KMeans(8), feature_dims=fdims).make_Xy(small)[0]
            init = Xh[rng.choice(Xh.shape[0], 8, replace=False)].astype(np.float64)
            fit = lambda: classify.fit_kmeans(ds, 8, fdims, init=init, max_iter=a.fit_iters)
            model = fit()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                model = fit()
            torch.cuda.synchronize()
            fit_ms = (time.perf_counter() - t0) * 1e3 / a.reps
            _lib.timing_enable(4 * a.fit_iters + 64)
            fit()
            steps = [ms for name, ms in _lib.timing_collect() if name == 'kmeans_step']
            _lib.timing_enable(0)
            nrows, nfeat = n * n * (1 if fdims else k), len(VARS) * (k if fdims else 1)
            Xh = np.concatenate([Xh] * max(1, a.host_rows // Xh.shape[0]))[:a.host_rows]
            km = KMeans(8, init=init.copy(), n_init=1, algorithm='lloyd', max_iter=a.fit_iters)
            t0 = time.perf_counter()
            km.fit(Xh)
            host_s = time.perf_counter() - t0
            host = Xh.shape[0] * km.n_iter_ / host_s                        # rows per second of one iteration
            step_ms = min(steps)
            moved = nrows * (nfeat * elem + 8)
            record('kmeans fit k=8 feature_dims=%s, one iteration' % fdims, nrows, nfeat,
                   (step_ms, sorted(steps)[len(steps) // 2]), sum(steps), host,
                   dict(fit_ms=fit_ms, n_iter=model.n_iter, passes=len(steps), host_rows=int(Xh.shape[0]),
                        host_n_iter=int(km.n_iter_), host_fit_s=host_s, step_bytes=moved,
                        fraction_of_hbm_peak=moved / (step_ms * 1e-3) / a.hbm_peak))

    def predict_lines():
        labels_yx = None
        for fdims in ([], ['time']):
            c = classify.Classifier(RandomForestClassifier(a.trees, random_state=0, n_jobs=16), feature_dims=fdims)
            c.fit(small, train)
            model = classify.ForestModel.from_sklearn(c.clf)
            Xh = c.make_Xy(small)[0]
            reps_h = max(1, a.host_rows // Xh.shape[0])
            Xh = np.concatenate([Xh] * reps_h)[:a.host_rows]
            host = host_rate(c.clf.predict, Xh)
            ms = timed(lambda: c.predict(ds), a.reps)
            kms = kernel_ms(lambda: c.predict(ds), 'classify_forest')
            nrows = n * n * (1 if fdims else k)
            record('forest feature_dims=%s' % fdims, nrows, len(VARS) * (k if fdims else 1), ms, kms, host,
                   dict(trees=a.trees, nodes=int(model.feature.size), depth=model.depth(),
                        forest_mb=model.feature.size * (16 + 8 * model.n_classes) / 1e6))
            if fdims:
                labels_yx = c.predict(ds)
        c = classify.Classifier(KMeans(3, n_init=2, random_state=0))
        c.fit(small)
        Xh = c.make_Xy(small)[0]
        Xh = np.concatenate([Xh] * max(1, a.host_rows // Xh.shape[0]))[:a.host_rows]
        host = host_rate(c.clf.predict, Xh)
        ms = timed(lambda: c.predict(ds), a.reps)
        record('kmeans k=3 feature_dims=[]', k * n * n, len(VARS), ms, kernel_ms(lambda: c.predict(ds), 'classify_kmeans'),
               host)
        lab = xr_lite.DataArray(labels_yx.values - 1, ('y', 'x'))
        ms = timed(lambda: classify.class_mean(ds, lab), a.reps)
        record('class_mean 3 classes', len(VARS) * k * n * n, 1, ms, kernel_ms(lambda: classify.class_mean(ds, lab), 'class_mean'),
               None)

        def labelled(count):
            """the crop's truth on `count` of its pixel columns (every date of one at feature_dims=[]), 0 elsewhere"""
            pick = np.zeros(truth.size, bool)
            pick[rng.choice(truth.size, count, replace=False)] = True
            return np.where(pick.reshape(truth.shape), truth, 0)

        kn = min(a.knn_n or n, n)
        part = xr_lite.Dataset()
        for i, v in enumerate(VARS):
            part[v] = (dims, stack[i][:, :kn, :kn])
        for ntrain, fdims in (() if a.skip_knn else ((1000, []), (10000, []), (1000, ['time']))):
            c = classify.Classifier(KNeighborsClassifier(3, n_jobs=16), feature_dims=fdims)
            c.fit(small, labelled(ntrain if fdims else -(-ntrain // k)))
            model = classify.KNNModel.from_sklearn(c.clf)
            Xh = c.make_Xy(small)[0]
            Xh = np.concatenate([Xh] * max(1, a.knn_host_rows // Xh.shape[0]))[:a.knn_host_rows]
            host = host_rate(c.clf.predict, Xh, reps=1)
            ms = timed(lambda: c.predict(part), a.knn_reps)
            kms = kernel_ms(lambda: c.predict(part), 'classify_knn')
            nrows = kn * kn * (1 if fdims else k)
            flops = 3.0 * nrows * model.n_train * model.n_features / (kms * 1e-3)
            record('knn k=3 feature_dims=%s' % fdims, nrows, model.n_features, ms, kms, host,
                   dict(n_train=model.n_train, fp64_ops_per_s=flops, fraction_of_fp64_peak=flops / a.fp64_peak))
        c = classify.Classifier(LogisticRegression(max_iter=300))
        c.fit(small, train)
        Xh = c.make_Xy(small)[0]
        Xh = np.concatenate([Xh] * max(1, a.host_rows // Xh.shape[0]))[:a.host_rows]
        host = host_rate(c.clf.predict, Xh)
        ms = timed(lambda: c.predict(ds), a.reps)
        record('logistic 3 classes feature_dims=[]', k * n * n, len(VARS), ms,
               kernel_ms(lambda: c.predict(ds), 'classify_linear'), host)

    if a.fit_only:
        kmeans_fit_lines()
        if a.json and os.path.exists(a.json):
            rows[:0] = [r for r in json.load(open(a.json)).get('rows', []) if not r['case'].startswith('kmeans fit')]
    else:
        predict_lines()
        kmeans_fit_lines()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(dict(k=k, n=n, threads=int(os.environ.get('OMP_NUM_THREADS', '0') or 0), rows=rows),
                  open(a.json, 'w'), indent=1)


if __name__ == '__main__':
    main()
