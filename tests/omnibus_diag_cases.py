"""The cases of the intensity-only omnibus test: seeded inputs and the list of what
tests/golden/omnibus_diag.npz records (numpy only; shared by the recorder, the CPU test that
reproduces the file and the GPU tests that compare with it)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'omnibus_diag.npz')
GOLDEN_F64 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'omnibus_diag_f64.npz')

CORE_SHAPES = [(1, 3, 5), (2, 3, 67), (3, 5, 64), (10, 5, 130), (24, 9, 300), (25, 4, 257)]
CORE_ALPHAS = (0.01, 0.5, 0.9, 0.99)
CORE_LOOKS = (1, 4.4, 9)
# the one-launch form takes k q sizeof(T) <= 192 bytes below alpha = 0.75 (nd_amd/csrc/omnibus_diag.hip):
# (q, dtype) -> the longest series it serves; the cases sit on both sides
FUSED_MAX_K = {(1, 'float32'): 48, (2, 'float32'): 24, (3, 'float32'): 16,
               (1, 'float64'): 24, (2, 'float64'): 12, (3, 'float64'): 8}


def gamma_stack(seed, q, k, ny, nx, looks, dtype):
    """q intensity planes (k, ny, nx): gamma(looks, 1 / looks) speckle around channel means 1, 0.5, 0.25;
    15 % of the pixels step up by 4 at a random date, 7 % drop to 0.3 (both channels alike)."""
    rng = np.random.default_rng(seed)
    gain = np.ones((k, ny, nx))
    t = np.arange(k)[:, None, None]
    m1 = rng.random((ny, nx)) < 0.15
    t1 = rng.integers(1, max(k, 2), size=(ny, nx))
    gain = gain * np.where((t >= t1[None]) & m1[None], 4.0, 1.0)
    m2 = rng.random((ny, nx)) < 0.07
    t2 = rng.integers(1, max(k, 2), size=(ny, nx))
    gain = gain * np.where((t >= t2[None]) & m2[None], 0.3, 1.0)
    return [np.ascontiguousarray((rng.gamma(looks, 1.0 / looks, (k, ny, nx)) * gain * 0.5 ** c).astype(dtype))
            for c in range(q)]


def step_stack(seed, q, dtype):
    """nd/tests/test_change_omnibus.py for intensities: 5 x 5 pixels, 10 dates, normal with sigma 0.1 around
    1, stepping to 10 at date 5."""
    rng = np.random.default_rng(seed)
    mean = np.where(np.arange(10) >= 5, 10.0, 1.0)[:, None, None]
    return [np.ascontiguousarray(rng.normal(mean, 0.1, (10, 5, 5)).astype(dtype)) for _ in range(q)]


def degenerate_stack(seed, q, dtype):
    """10 x 6 x 70 with NaN, 0, negative and inf samples in 5 % of the values."""
    planes = gamma_stack(seed, q, 10, 6, 70, 4.4, dtype)
    rng = np.random.default_rng(seed + 1)
    for val in (np.nan, 0.0, -1.0, np.inf):
        for p in planes:
            p[rng.random(p.shape) < 0.0125] = val
    return planes


def make_input(case, seed=None):
    seed = case['seed'] if seed is None else seed
    dtype = np.dtype(case['dtype'])
    if case['kind'] == 'step':
        return step_stack(seed, case['q'], dtype)
    if case['kind'] == 'degenerate':
        return degenerate_stack(seed, case['q'], dtype)
    return gamma_stack(seed, case['q'], case['k'], case['ny'], case['nx'], case['n'], dtype)


def cases():
    """Every recorded case: name, kind, q, dtype, (k, ny, nx), n, alphas, base seed."""
    out = []

    def add(name, kind, q, dtype, k, ny, nx, n, alphas):
        out.append(dict(name=name, kind=kind, q=q, dtype=dtype, k=k, ny=ny, nx=nx, n=n, alphas=tuple(alphas),
                        seed=1000 + 7 * len(out)))
    for q in (1, 2, 3):
        for dtype in ('float32', 'float64'):
            for (k, ny, nx) in CORE_SHAPES:
                for n in CORE_LOOKS:
                    add('core_q%d_%s_k%d_%dx%d_n%g' % (q, dtype, k, ny, nx, n), 'gamma', q, dtype, k, ny, nx, n,
                        CORE_ALPHAS)
    for (q, dtype), kmax in sorted(FUSED_MAX_K.items()):
        for k in (kmax, kmax + 1):
            add('limit_q%d_%s_k%d' % (q, dtype, k), 'gamma', q, dtype, k, 4, 130, 4.4, (0.01, 0.7, 0.8, 0.99))
    for q in (2, 3):
        for k in (33, 97, 200):
            add('long_q%d_float32_k%d' % (q, k), 'gamma', q, 'float32', k, 4, 130, 4.4, (0.01, 0.99))
        add('long_q%d_float64_k97' % q, 'gamma', q, 'float64', 97, 4, 130, 4.4, (0.01, 0.99))
    for q in (1, 2):
        for dtype in ('float32', 'float64'):
            add('step_q%d_%s' % (q, dtype), 'step', q, dtype, 10, 5, 5, 9, (0.9,))
    for q, dtype in ((2, 'float32'), (3, 'float64'), (1, 'float32')):
        add('degenerate_q%d_%s' % (q, dtype), 'degenerate', q, dtype, 10, 6, 70, 4.4, (0.01, 0.9))
    return out


def ulp(alpha, dtype):
    return float(np.spacing(np.dtype(dtype).type(alpha)))


class Golden:
    """The recorded file(s): per case the seed that was used, per (case, alpha) the packed map and the smallest
    |P - alpha| the search met, per case z and P of the whole-series test."""

    def __init__(self):
        self.a = dict(np.load(GOLDEN))
        self.a.update(np.load(GOLDEN_F64))
        self.names = [str(s) for s in self.a['names']]
        self.seeds = dict(zip(self.names, self.a['seeds'].tolist()))

    def case(self, name):
        c = next(c for c in cases() if c['name'] == name)
        return dict(c, seed=self.seeds[name])

    def expected(self, name, alpha):
        c = self.case(name)
        bits = self.a['map/%s/%g' % (name, alpha)]
        n = c['ny'] * c['nx'] * c['k']
        m = np.unpackbits(bits)[:n].reshape(c['ny'], c['nx'], c['k'])
        return m, self.a['z/' + name], self.a['P/' + name], float(self.a['closest/%s/%g' % (name, alpha)])


def compare(got_map, got_z, got_P, want_map, want_z, want_P, closest, alpha, dtype):
    """The comparison rule of the GPU tests: z / P within 1e-5 relative (float64: 1e-10) with equal NaN
    positions; maps equal, a differing pixel tolerated only where the restatement's deciding test has
    |P - alpha| <= 2 ulp(T), and for at most 1 pixel in 10^5."""
    rtol = 1e-5 if np.dtype(dtype) == np.float32 else 1e-10
    if got_z is not None:
        np.testing.assert_array_equal(np.isnan(got_z), np.isnan(want_z))
        np.testing.assert_allclose(got_z, want_z, rtol=rtol, atol=0, equal_nan=True)
        np.testing.assert_array_equal(np.isnan(got_P), np.isnan(want_P))
        # (below the smallest normal number of T one ulp is more than 1e-5 relative)
        np.testing.assert_allclose(got_P, want_P, rtol=rtol, atol=float(np.finfo(np.dtype(dtype)).tiny), equal_nan=True)
    ndiff = int((got_map.reshape(-1, got_map.shape[-1]) != want_map.reshape(-1, want_map.shape[-1])).any(axis=1).sum())
    if ndiff:
        npix = want_map.size // want_map.shape[-1]
        assert closest <= 2 * ulp(alpha, dtype) and ndiff <= npix / 1e5, \
            '%d pixels differ; the closest decision of the restatement is %g from alpha' % (ndiff, closest)
