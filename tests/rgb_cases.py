"""
tests/rgb_cases.py -- the case families of the to_rgb tests: named 2-D planes, built the same way for the
CPU tests (restatement against numpy), the golden file and the GPU tests (device against restatement).
"""
import numpy as np

PERCENTILES = (0, 2, 2.5, 50, 98, 99.9, 100)
DTYPES = (np.float32, np.float64)


def planes(dtype, seed=0):
    """-> ordered dict name -> 2-D array of `dtype`"""
    rng = np.random.default_rng(seed)
    out = {}

    def expo(shape):
        return rng.exponential(size=shape).astype(dtype)

    out['exponential'] = expo((37, 53))
    a = expo((41, 29)); a[rng.random(a.shape) < 0.2] = np.nan
    out['some_nan'] = a
    out['all_nan'] = np.full((5, 7), np.nan, dtype)
    a = expo((23, 31)); a[rng.random(a.shape) < 0.1] = np.inf; a[rng.random(a.shape) < 0.1] = -np.inf
    out['infinities'] = a
    out['mostly_inf'] = np.where(rng.random((9, 11)) < 0.9, np.inf, 1.0).astype(dtype)
    out['negative'] = (rng.standard_normal((33, 17)) * 3).astype(dtype)
    tiny = np.finfo(dtype).tiny
    a = rng.standard_normal((19, 21)).astype(dtype) * dtype(tiny) * dtype(0.25)
    a[rng.random(a.shape) < 0.3] = 0.0
    a[rng.random(a.shape) < 0.3] = -0.0
    out['denormal_zero'] = a
    out['ties16'] = rng.integers(0, 16, (64, 48)).astype(dtype)
    out['constant'] = np.full((24, 40), 3.25, dtype)
    out['size1'] = np.array([[1.5]], dtype)
    out['size2'] = np.array([[2.0, -1.0]], dtype)
    out['odd'] = expo((7, 9))
    out['scaled_1e-6'] = expo((32, 32)) * dtype(1e-6)
    out['scaled_1e6'] = expo((32, 32)) * dtype(1e6)
    out['one_binade'] = (1 + rng.random((48, 64))).astype(dtype)
    return out
