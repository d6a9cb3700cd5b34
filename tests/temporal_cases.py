"""What the temporal GPU tests share: series a selection or a sum can go wrong on, the device call in every layout, the
comparison with the restatement (tests/temporal_ref.py: float64 and integer outputs bit for bit, order statistics by
==) and the random cases of tests/test_temporal_fuzz_gpu.py."""
import numpy as np

from tests import temporal_ref as ref

# (time, y, x); (y, x, time); (y, time, x); a crop of each of the first two whose first element is not 16-byte aligned;
# every second column of a wider (time, y, x) buffer
LAYOUTS = ('tyx', 'yxt', 'ytx', 'crop', 'crop_yxt', 'step')
DTYPES = ('float32', 'float64', 'int16', 'int32', 'uint8', 'bool')
ALL = ref.STATS
ORDER = ('median',)


def speckle(rng, shape, dtype='float32', nan=0.15, ties=0.1):
    """finite gamma speckle of 4 looks with a share of NaN and a share of one constant (ties); shape: (k, ny, nx)"""
    x = rng.gamma(4.0, 0.25, size=shape).astype(dtype)
    if ties:
        x[rng.random(shape) < ties] = 0.5
    if nan:
        x[rng.random(shape) < nan] = np.nan
    return x


def with_special_pixels(x):
    """pixel (0, 0) all NaN and the next pixel with one valid date, where the plane has them"""
    k = x.shape[0]
    flat = x.reshape(k, -1)
    flat[:, 0] = np.nan
    if flat.shape[1] > 1:
        flat[:, 1] = np.nan
        flat[k // 2, 1] = 1.25
    return x


def _device():
    import torch
    return torch, torch.device('cuda', torch.cuda.current_device())


def upload(stack, layout='tyx'):
    """stack: numpy (k, ny, nx) -> (a 3-D device view, the series' axis)"""
    torch, dev = _device()
    stack = np.asarray(stack)
    k, ny, nx = stack.shape
    filler = np.array(7, stack.dtype)
    if layout == 'tyx':
        return torch.from_numpy(np.ascontiguousarray(stack)).to(dev), 0
    if layout == 'yxt':
        return torch.from_numpy(np.ascontiguousarray(stack.transpose(1, 2, 0))).to(dev), 2
    if layout == 'ytx':
        return torch.from_numpy(np.ascontiguousarray(stack.transpose(1, 0, 2))).to(dev), 1
    if layout == 'crop':
        big = np.full((k + 1, ny + 2, nx + 3), filler)
        big[1:, 1:ny + 1, 1:nx + 1] = stack
        return torch.from_numpy(big).to(dev)[1:, 1:ny + 1, 1:nx + 1], 0
    if layout == 'crop_yxt':
        big = np.full((ny + 1, nx + 2, k), filler)
        big[1:, 1:nx + 1] = stack.transpose(1, 2, 0)
        return torch.from_numpy(big).to(dev)[1:, 1:nx + 1], 2
    if layout == 'step':
        big = np.full((k, ny, 2 * nx + 1), filler)
        big[:, :, 1::2] = stack
        return torch.from_numpy(big).to(dev)[:, :, 1::2], 0
    raise ValueError(layout)


def device_stats(K, stack, stats=ALL, q=(), skipna=True, ddof=0, layout='tyx', form='auto'):
    """stack numpy (k, ny, nx) through kernels.temporal_stats -> a dict of numpy (ny, nx)"""
    t, axis = upload(stack, layout)
    got = K.temporal_stats(t, stats, q, skipna=skipna, ddof=ddof, axis=axis, _form=form)
    return {s: v.cpu().numpy() for s, v in got.items()}


def want_stats(stack, stats=ALL, q=(), skipna=True, ddof=0):
    want = ref.stats(np.asarray(stack), 0, skipna, ddof, q)
    return {s: want[s] for s in tuple(stats) + tuple(ref.name(p) for p in q)}


def check(K, stack, stats=ALL, q=(), skipna=True, ddof=0, layout='tyx', form='auto', want=None):
    got = device_stats(K, stack, stats, q, skipna, ddof, layout, form)
    want = want_stats(stack, stats, q, skipna, ddof) if want is None else want
    ref.same(got, want, '%s %s' % (layout, form))
    return got


def serves_order(K, dtype, k):
    """whether order statistics of k dates of numpy type `dtype` are served"""
    import torch
    t = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    return k <= K.TEMPORAL_LDS_MAX[t]


# ---- the random cases of the fuzz test -----------------------------------------------------------------------------
def random_case(rng, K):
    ny, nx = (int(v) for v in rng.integers(1, 151, size=2))
    k = int(rng.integers(1, 141))
    dtype = str(rng.choice(DTYPES, p=[0.35, 0.35, 0.075, 0.075, 0.075, 0.075]))
    shape = (k, ny, nx)
    if dtype in ('float32', 'float64'):
        stack = speckle(rng, shape, dtype, float(rng.choice([0.0, 0.01, 0.15, 0.6])), float(rng.choice([0.0, 0.1])))
        if rng.random() < 0.3:
            stack[rng.random(shape) < 0.02] = np.inf
            stack[rng.random(shape) < 0.02] = -np.inf
        if rng.random() < 0.3:
            with_special_pixels(stack)
    elif dtype == 'bool':
        stack = rng.random(shape) < 0.2
    elif dtype == 'uint8':
        stack = rng.integers(0, 256, size=shape).astype(np.uint8)
    else:
        stack = rng.integers(-1000, 1000, size=shape).astype(dtype)
    stats = tuple(s for s in ALL if rng.random() < 0.5)
    nq = int(rng.choice([0, 0, 1, 2, 5, 9]))
    q = tuple(float(v) for v in rng.choice([0, 2, 5, 25, 33.3, 50, 75, 97.5, 98, 100], size=nq, replace=False))
    if not serves_order(K, stack.dtype, k):  # beyond the LDS form: the moments alone are served
        stats = tuple(s for s in stats if s not in ORDER)
        q = ()
    if not stats and not q:
        stats = ('mean',)
    return {'stack': stack, 'stats': stats, 'q': q, 'skipna': bool(rng.random() < 0.7), 'ddof': int(rng.integers(0, 2)),
            'layout': str(rng.choice(LAYOUTS))}


def describe(case):
    return {key: val for key, val in case.items() if key != 'stack'} | {
        'shape': case['stack'].shape, 'dtype': str(case['stack'].dtype)}


def run_case(K, case):
    """the kernel-level call of a random case against the restatement (AssertionError)"""
    stack = case['stack']
    check(K, stack, case['stats'], case['q'], case['skipna'], case['ddof'], case['layout'])
