"""Seeded inputs of the change_segments tests (numpy only; shared by the CPU and the GPU tests).

Speckle: 9-look Wishart samples from tests/synth.py (the intensity cases take the diagonal of the full-pol
sample).  The map is a seeded Bernoulli(0.25) map, not a detector's output, and the power of every segment of
THAT map is multiplied by a factor drawn per pixel and per change from {1/4, 1, 4} -- for half of the pixels one
factor for the whole matrix (the difference is then definite most of the time), for the other half one factor
per channel (indefinite differences).  A single intensity cannot be indefinite: there a share of the pixels is
constant, so that the difference is exactly zero (code 3)."""
import numpy as np

from tests import synth

STRUCTURES = [('diag', 1), ('diag', 2), ('diag', 3), ('c2', 4), ('c3', 9)]
CORE_SHAPES = [(1, 1, 1), (2, 1, 63), (3, 3, 65), (10, 5, 130), (25, 4, 257), (33, 2, 64)]   # (k, ny, nx)
FACTORS = np.array([0.25, 1.0, 4.0])


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bit_equal(got, want, what=''):
    """the comparison rule of the means: same type and shape, NaN where the restatement has NaN, elsewhere the
    same bits -- no tolerance, no excluded pixel"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    np.testing.assert_array_equal(_bits(np.where(nan, 0, got)), _bits(np.where(nan, 0, want)), err_msg=what)


def bernoulli_map(rng, k, ny, nx, p=0.25):
    return (rng.random((ny, nx, k)) < p).astype(np.uint8)


def channel_gains(rng, change, q):
    """(q, k, ny, nx): the power factor of every channel at every date, constant over each segment of `change`."""
    ny, nx, k = change.shape
    per_channel = rng.random((ny, nx)) < 0.5
    gains = np.empty((q, k, ny, nx))
    cur = np.ones((q, ny, nx))
    for t in range(k):
        whole = FACTORS[rng.integers(0, 3, (ny, nx))]
        each = FACTORS[rng.integers(0, 3, (q, ny, nx))]
        new = np.where(per_channel[None], each, whole[None])
        opens = (change[..., t] != 0) if t >= 1 else np.ones((ny, nx), bool)
        cur = np.where(opens[None], new, cur)
        gains[:, t] = cur
    return gains


def make(structure, nplanes, dtype, k, ny, nx, seed):
    """-> (planes: nplanes arrays (k, ny, nx) of `dtype`, change: uint8 (ny, nx, k))."""
    rng = np.random.default_rng(seed)
    change = bernoulli_map(rng, k, ny, nx)
    shape = (k, ny, nx)
    if structure == 'c2':
        c11, re, im, c22 = synth.wishart_c2(rng, shape, 9, np.float64)
        g = channel_gains(rng, change, 2)
        g12 = np.sqrt(g[0] * g[1])
        planes = [c11 * g[0], re * g12, im * g12, c22 * g[1]]
    elif structure == 'c3':
        w = synth.wishart_c3(rng, shape, 9, np.float64)
        g = channel_gains(rng, change, 3)
        g12, g13, g23 = np.sqrt(g[0] * g[1]), np.sqrt(g[0] * g[2]), np.sqrt(g[1] * g[2])
        planes = [w[0] * g[0], w[1] * g[1], w[2] * g[2], w[3] * g12, w[4] * g12, w[5] * g13, w[6] * g13,
                  w[7] * g23, w[8] * g23]
    else:
        w = synth.wishart_c3(rng, shape, 9, np.float64)
        g = channel_gains(rng, change, nplanes)
        planes = [w[c] * g[c] for c in range(nplanes)]
        if nplanes == 1:
            flat = rng.random((ny, nx)) < 0.3
            planes[0] = np.where(flat[None], 0.5, planes[0])
    return [np.ascontiguousarray(p.astype(dtype)) for p in planes], change


def core_cases():
    """(structure, planes, dtype, k, ny, nx, seed).  The seeds are such that also the cases with a dozen flagged
    positions hold every code (tests/test_change_segments_cpu.py checks the shares)."""
    out = []
    for structure, nplanes in STRUCTURES:
        for dtype in (np.float32, np.float64):
            for (k, ny, nx) in CORE_SHAPES:
                out.append((structure, nplanes, dtype, k, ny, nx, 4117 + 13 * len(out)))
    return out


def case_id(case):
    structure, nplanes, dtype, k, ny, nx, _ = case
    return '%s%d-%s-%dx%dx%d' % (structure, nplanes, np.dtype(dtype).name, k, ny, nx)


def step_stack(kind, dtype=np.float32, seed=7):
    """The stack of nd/tests/test_change_omnibus.py with a step of x 4: 10 dates of 5 x 5 pixels, normal with
    sigma 0.1 around C11 = C22 = 1, C12 = 0; from date 5 on the power is x 4 ('up'); 'down' runs from 4 to 1;
    'mixed' has C11 x 4 with C22 x 1/4."""
    rng = np.random.default_rng(seed)
    late = (np.arange(10) >= 5)[:, None, None]
    m1, m2 = {'up': ((1.0, 4.0), (1.0, 4.0)), 'down': ((4.0, 1.0), (4.0, 1.0)), 'mixed': ((1.0, 4.0), (4.0, 1.0))}[kind]
    mean = [np.where(late, m1[1], m1[0]), 0.0, 0.0, np.where(late, m2[1], m2[0])]
    return [np.ascontiguousarray(rng.normal(m, 0.1, (10, 5, 5)).astype(dtype)) for m in mean]


def degenerate(planes, seed):
    """NaN, +inf, -inf, 0 and negative values in 5 % of the samples of a copy of the planes."""
    rng = np.random.default_rng(seed)
    planes = [p.copy() for p in planes]
    for val in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        for p in planes:
            p[rng.random(p.shape) < 0.01] = val
    return planes
