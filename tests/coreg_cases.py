"""Cases for the coregistration edge tests (tests/test_coregister_edges_cpu.py, ..._gpu.py): small
stacks at odd sizes and at every width of the upsampled region, with a rule that says, from the numpy
restatement (tests/coreg_ref.py) alone, which dates have a shift that any correct implementation must
reproduce exactly.  No GPU, no scikit-image.

The near-tie rule
-----------------
The shift of a date is the argmax of |cc| (whole-pixel correlation) followed by the argmax of |CC|
(upsampled region, cells 1/u apart).  An implementation with another FFT algorithm may order two
nearly equal cells the other way round.  `decided(src, ref, u)` therefore measures, per date,

  gap   (largest - second largest) / largest of |cc|, and the same of |CC|
  diff  max |normalised |cc| from the float32 inputs - the same from those values held in float64|,
        and the same for |CC|: the error of the float32 path of the restatement itself

and calls the date decided when gap > FACTOR * diff for both quantities (and both paths agree on the
whole-pixel peak).  FACTOR = 4: the float32 FFT of the device is another algorithm with an error of
the same order, so it may differ from the restatement's float32 path by about twice `diff`; 4 leaves
a factor 2 over that.  For float64 inputs the threshold is F64_GAP = 1e-10 relative.  Along an axis
of length 1 every cell ties exactly and the shift is forced to 0: the gaps are taken along the other
axis only.  A decided date must match the restatement exactly, an undecided one within one 1/u step.

Measured (k = 6, reference 0, seed 100 ny + nx + u; minimum gap and maximum diff over the 5 dates):
  31x37_u7       float32  coarse gap 2.7e-04 diff 5.0e-07   fine gap 4.6e-07 diff 3.0e-09   decided 5 of 5
  31x37_u7       float64  coarse gap 2.7e-04 diff 0.0e+00   fine gap 4.6e-07 diff 0.0e+00   decided 5 of 5
  17x65_u16      float32  coarse gap 1.3e-04 diff 3.6e-07   fine gap 3.6e-07 diff 2.3e-09   decided 5 of 5
  65x33_u22      float32  coarse gap 2.5e-04 diff 4.0e-07   fine gap 5.2e-08 diff 6.1e-10   decided 5 of 5
  64x63_u33      float32  coarse gap 2.3e-04 diff 3.7e-07   fine gap 2.1e-07 diff 8.0e-10   decided 5 of 5
  64x63_u33      float64  coarse gap 2.3e-04 diff 0.0e+00   fine gap 2.1e-07 diff 0.0e+00   decided 5 of 5
  129x31_u43     float32  coarse gap 1.1e-04 diff 6.5e-07   fine gap 1.9e-08 diff 5.1e-10   decided 5 of 5
  33x95_u54      float32  coarse gap 8.3e-05 diff 4.3e-07   fine gap 7.2e-08 diff 1.1e-09   decided 5 of 5
  65x127_u85     float32  coarse gap 1.0e-04 diff 7.5e-07   fine gap 5.9e-09 diff 5.3e-10   decided 5 of 5
  35x67_u128     float32  coarse gap 2.1e-05 diff 6.5e-07   fine gap 3.7e-09 diff 8.8e-10   decided 5 of 5
  35x67_u128     float64  coarse gap 2.1e-05 diff 0.0e+00   fine gap 3.7e-09 diff 0.0e+00   decided 5 of 5
  63x1_u10       float32  coarse gap 1.4e-03 diff 2.1e-07   fine gap 2.6e-06 diff 7.9e-10   decided 5 of 5
  1x65_u10       float32  coarse gap 4.1e-04 diff 2.4e-07   fine gap 1.4e-06 diff 2.6e-09   decided 5 of 5
  fourier 31x37_u7       float64  coarse gap 6.0e-04 diff 0.0e+00   fine gap 8.9e-05 diff 0.0e+00   decided 4 of 4  exact True
  fourier 31x37_u7       float32  coarse gap 6.0e-04 diff 3.6e-07   fine gap 8.9e-05 diff 9.6e-10   decided 4 of 4  exact True
  fourier 31x37_u43      float64  coarse gap 1.7e-04 diff 0.0e+00   fine gap 2.5e-06 diff 0.0e+00   decided 4 of 4  exact True
  fourier 31x37_u43      float32  coarse gap 1.7e-04 diff 3.2e-07   fine gap 2.5e-06 diff 1.9e-09   decided 4 of 4  exact True
  fourier 35x67_u128     float64  coarse gap 6.8e-05 diff 0.0e+00   fine gap 1.2e-07 diff 0.0e+00   decided 4 of 4  exact True
  fourier 35x67_u128     float32  coarse gap 6.8e-05 diff 4.0e-07   fine gap 1.2e-07 diff 5.2e-10   decided 4 of 4  exact True
The Fourier-shift stacks (`fourier ...`, 4 dates) return the applied shift exactly in both types.
"""
import collections
import functools

import numpy as np
import scipy.ndimage as ndi

from tests import coreg_ref

FACTOR = 4.0
F64_GAP = 1e-10
K = 6

# (ny, nx, u): the region is R = ceil(1.5 u) cells wide
#   31 x 37,  u = 7    R = 11  dft_x MI = 1; prime sizes
#   17 x 65,  u = 16   R = 24  dft_x MI = 2; nh = 33 spans three 16-column chunks
#   65 x 33,  u = 22   R = 33  dft_x MI = 3; the second block of 64 rows holds one row
#   64 x 63,  u = 33   R = 50  dft_x MI = 4; even x odd
#   129 x 31, u = 43   R = 65  dft_x MI = 5; three row blocks
#   33 x 95,  u = 54   R = 81  dft_x MI = 4 with two blocks along the region
#   65 x 127, u = 85   R = 128 dft_y with exactly two lane groups; n = 8255: two argmax partials
#   35 x 67,  u = 128  R = 192 dft_y with one lane group and 64 idle lanes; the maximum factor
#   63 x 1 and 1 x 65, u = 10  degenerate axes
CASES = ((31, 37, 7), (17, 65, 16), (65, 33, 22), (64, 63, 33), (129, 31, 43), (33, 95, 54), (65, 127, 85),
         (35, 67, 128), (63, 1, 10), (1, 65, 10))
F64_CASES = ((31, 37, 7), (64, 63, 33), (35, 67, 128))
FOURIER_CASES = ((31, 37, 7), (31, 37, 43), (35, 67, 128))
FOURIER_CPU_SIZES = tuple(sorted({(ny, nx) for ny, nx, _ in CASES if ny > 1 and nx > 1}))
FOURIER_CPU_FACTORS = (2, 7, 16, 43, 128)
VARS = ('C11', 'C12__re', 'C12__im', 'C22')


def case_id(case):
    return '%dx%d_u%d' % case


def case_seed(ny, nx, u):
    return 100 * ny + nx + u


# ------------------------------------------------------------------ generators
def stack(seed, k, ny, nx, dtype, nvars=1):
    """The recipe of tests/golden/make_coreg_golden.py: {name: planar (k, ny, nx)}, values multiples of
    2^-8 (float32 and float64 hold the same numbers), C11 / C22 positive, C12 signed."""
    rng = np.random.RandomState(seed)
    base = ndi.gaussian_filter(rng.normal(size=(ny + 16, nx + 16)), 2.5)
    base = (base - base.min()) / (base.max() - base.min())
    planes = {}
    for v in VARS[:nvars]:
        p = np.empty((k, ny, nx))
        for t in range(k):
            dy, dx = rng.uniform(-3, 3, 2)
            moved = ndi.shift(base, (dy, dx), order=3, mode='nearest')[8:8 + ny, 8:8 + nx]
            noise = rng.normal(scale=0.05, size=(ny, nx))
            p[t] = 0.2 + 3.0 * moved + noise if v in ('C11', 'C22') else 2.0 * moved - 1.0 + noise
        planes[v] = (np.round(p * 256) / 256).astype(dtype)
    planes['C11'] = np.abs(planes['C11']) + np.asarray(1 / 256, dtype)
    return planes


@functools.lru_cache(maxsize=None)
def c11_stack(ny, nx, u, dtype, k=K):
    a = stack(case_seed(ny, nx, u), k, ny, nx, dtype)['C11']
    a.setflags(write=False)
    return a


def bandlimited(rng, ny, nx):
    """A positive periodic float64 image whose spectrum fills a quarter of each axis.  Every frequency
    of the band carries weight, so the correlation has one narrow peak and the whole-pixel argmax lands
    within 0.75 pixels of the shift, which is as far as the upsampled region reaches (a spectrum of a
    few lines has a correlation with side peaks of nearly the same height, and the method itself may
    then start from a cell too far away)."""
    F = np.zeros((ny, nx), complex)
    hy, hx = ny // 4, nx // 4
    for i in range(-hy, hy + 1):
        for j in range(-hx, hx + 1):
            F[i, j] = rng.normal() + 1j * rng.normal()
    a = np.real(np.fft.ifft2(F))
    return a - a.min() + 0.1


def fourier_shift(a, dy, dx):
    """`a` moved by (dy, dx) with a phase ramp: phase_shift(fourier_shift(a, dy, dx), a) is (dy, dx)."""
    ny, nx = a.shape
    fy, fx = np.fft.fftfreq(ny)[:, None], np.fft.fftfreq(nx)[None, :]
    return np.real(np.fft.ifft2(np.fft.fft2(a) * np.exp(-2j * np.pi * (fy * dy + fx * dx))))


def grid_shifts(rng, u, count):
    """`count` (dy, dx) on the 1/u grid within [-3, 3].  Odd multiples of 1/2 are left out: there two
    whole-pixel cells tie (the shift found is the same from either, but the date is not decided)."""
    out = []
    while len(out) < count:
        m = rng.integers(-3 * u, 3 * u + 1, 2)
        if not (((2 * m) % u == 0) & (m % u != 0)).any():
            out.append(m / u)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def fourier_stack(ny, nx, u, k=5):
    """(float64 planar (k, ny, nx) stack, applied (k, 2) shifts): date 0 is the reference."""
    rng = np.random.default_rng(case_seed(ny, nx, u))
    ref = bandlimited(rng, ny, nx)
    applied = np.concatenate([np.zeros((1, 2)), grid_shifts(rng, u, k - 1)])
    a = np.stack([ref] + [fourier_shift(ref, dy, dx) for dy, dx in applied[1:]])
    a.setflags(write=False)
    return a, applied


# ------------------------------------------------------------------ the near-tie rule
Margins = collections.namedtuple('Margins', 'shift whole coarse_gap coarse_diff fine_gap fine_diff')


def _correlations(src, ref, u):
    """The steps of coreg_ref.phase_shift: (whole-pixel shift, |cc| / max, |CC| / max or None)."""
    fft = coreg_ref._fft
    P = fft.fftn(src) * fft.fftn(ref).conj()
    cc = np.abs(fft.ifftn(P))
    peak = np.unravel_index(np.argmax(cc), cc.shape)
    s = np.array(peak, np.float64)
    mid = np.array([np.fix(n / 2) for n in cc.shape])
    s[s > mid] -= np.array(cc.shape)[s > mid]
    CC = None
    if u > 1:
        region = np.ceil(u * 1.5)
        d = np.fix(region / 2.0)
        CC = np.abs(coreg_ref.upsampled_dft(P.conj(), int(region), np.float64(u), d - s * u))
        if src.shape[0] == 1:
            CC = CC[:1]
        if src.shape[1] == 1:
            CC = CC[:, :1]
        CC = CC / CC.max()
    return s, cc / cc.max(), CC


def _gap(a):
    top = np.partition(a.ravel(), -2)[-2:]
    return float(top[1] - top[0]) / float(top[1])


def margins(src, ref, u):
    """The reference shift of `src` against `ref` and the figures the rule compares."""
    shift = coreg_ref.phase_shift(src, ref, u)
    s, cc, CC = _correlations(src, ref, u)
    if src.dtype == np.float64:
        return Margins(shift, s, _gap(cc), 0.0, None if CC is None else _gap(CC), 0.0)
    s64, cc64, CC64 = _correlations(src.astype(np.float64), ref.astype(np.float64), u)
    same = bool((s == s64).all())
    fine_diff = None if CC is None else (float(np.abs(CC - CC64).max()) if same else np.inf)
    return Margins(shift, s, _gap(cc), float(np.abs(cc - cc64).max()), None if CC is None else _gap(CC), fine_diff)


def decided(src, ref, u):
    """(reference shift of the date, whether every correct implementation must find exactly it)."""
    m = margins(src, ref, u)
    if src.dtype == np.float64:
        ok = m.coarse_gap > F64_GAP and (m.fine_gap is None or m.fine_gap > F64_GAP)
    else:
        ok = m.coarse_gap > FACTOR * m.coarse_diff and (m.fine_gap is None or m.fine_gap > FACTOR * m.fine_diff)
    return m.shift, bool(ok)


def decided_stack(c11, reference, u):
    """((k, 2) reference shifts, (k,) decided flags) of a planar stack; the reference date is decided."""
    k = c11.shape[0]
    sh, ok = np.zeros((k, 2)), np.ones(k, bool)
    for t in range(k):
        if t != reference:
            sh[t], ok[t] = decided(c11[t], c11[reference], u)
    return sh, ok


@functools.lru_cache(maxsize=None)
def case_reference(ny, nx, u, dtype):
    """decided_stack of the case's C11 stack, computed once per session."""
    return decided_stack(c11_stack(ny, nx, u, dtype), 0, u)


@functools.lru_cache(maxsize=None)
def fourier_reference(ny, nx, u, dtype):
    a, applied = fourier_stack(ny, nx, u)
    return decided_stack(a.astype(dtype), 0, u)


def check_shifts(got, want, ok, u, shape):
    """The rule: decided dates exact, the others within one 1/u step; 0 along an axis of length 1."""
    got, want = np.asarray(got), np.asarray(want)
    off = np.abs(got - want)
    assert (off[ok] < 1e-12).all(), (got, want, ok)
    assert (off <= 1.0 / u + 1e-12).all(), (got, want, ok)
    for axis in (0, 1):
        if shape[axis] == 1:
            assert (got[:, axis] == 0).all(), got
    return off.max(axis=1) < 1e-12


# ------------------------------------------------------------------ warp
WARP_SHAPES = ((15, 63), (16, 64), (17, 65), (33, 129), (1, 65), (63, 1), (2, 3), (129, 130))
WARP_PM_SHAPES = ((17, 65), (2, 3))
WARP_REF = 6


def warp_shifts(nr, nc):
    """12 dates: every row of the table of shifts, the reference (its row is ignored) at WARP_REF."""
    e = 2.0 ** -20
    return np.array([(0.0, 0.0), (1.0, -1.0), (0.5, -0.5), (3 - e, -3 + e), (2.3, -1.7), (-6.25, 7.75),
                     (0.75, -0.25), (nr + 5.0, 0.0), (0.0, -(nc + 5.0)), (np.nan, 1.5), (np.inf, -np.inf),
                     (0.25, 0.25)])


def warp_planes(nr, nc, dtype, k=12):
    """Four planar (k, nr, nc) variables for the clip: positive (exact zeros of the padding are kept),
    signed with an exact 0, constant per date (lo == hi), positive with one NaN on date 4."""
    rng = np.random.RandomState(1000 * nr + nc)
    q = lambda a: (np.round(a * 256) / 256).astype(dtype)
    pos = q(0.25 + rng.uniform(0, 3, (k, nr, nc)))
    sgn = q(rng.normal(0, 1, (k, nr, nc)))
    sgn[:, nr // 2, nc // 2] = 0
    const = np.empty((k, nr, nc), dtype)
    const[:] = (np.where(np.arange(k) % 3 == 2, -1.0, 1.0) * (np.arange(k) + 2) / 4)[:, None, None]
    nan = q(0.5 + rng.uniform(0, 2, (k, nr, nc)))
    nan[4, nr // 3, nc // 2] = np.nan
    return {'pos': pos, 'sgn': sgn, 'const': const, 'nan': nan}


MINMAX_SHIFTS = np.array([(0.3, -0.4), (-0.6, 0.7), (0.5, 0.5)])


def minmax_planes(dtype, nr=129, nc=130):
    """(3, nr, nc): the extremes of plane 0 at the first and last element, of plane 1 the other way
    round, of plane 2 at elements 8191 and 8192 (both sides of the partition of two blocks)."""
    rng = np.random.RandomState(7)
    a = (np.round((1.0 + rng.uniform(0, 1, (3, nr * nc))) * 256) / 256).astype(dtype)
    for t, (i_lo, i_hi) in enumerate(((0, nr * nc - 1), (nr * nc - 1, 0), (8191, 8192))):
        a[t, i_lo], a[t, i_hi] = 0.5, 4.0
    return a.reshape(3, nr, nc)
