"""The wave-search form of the dual-pol omnibus test's first pass (omnibus_c2_retain_wsearch_kernel): a wave that
finds 1 .. 15 candidates searches them itself.  Every map is compared byte for byte with the C oracle, and every case
asks the library's own predicate (nd_amd_omnibus_c2_uses_wave_search) which form served it.

The form covers float32, 2 <= k <= 24, no rasters, alpha >= 0.99 (the measured switch; the cases at 0.95 assert the
old form and the same map).  Series of 25 .. 32 dates keep the two-pass form
(their 128 series registers leave nothing of the budget of four waves per SIMD: the instantiation spilled); the
cases at k = 25 and 32 therefore assert the OLD form through the predicate, and the same map.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import synth

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX_WAVE = 24           # the longest series the form takes
ALPHA_MIN = 0.99         # the measured switch (profiles/wave_search_forms.txt): below it the two-pass form is faster


def _uses(dtype, k, alpha, n, stats=False, stride_x=1):
    from nd_amd import _lib
    return bool(_lib.lib().nd_amd_omnibus_c2_uses_wave_search(0 if dtype == np.float32 else 1, int(k), int(stride_x),
                                                              float(alpha), int(n), int(bool(stats))))


def _rule(dtype, k, alpha, n, stats):
    """DESIGN 5, K1 (for looks whose screens can decide: n >= 2 here)."""
    return dtype == np.float32 and 2 <= k <= KMAX_WAVE and not stats and alpha >= ALPHA_MIN


def _want(oracle, planes, alpha, n):
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    with np.errstate(all='ignore'):
        return np.asarray(oracle.change_detection_planes(yxt, alpha, n, njobs=8)).astype(np.uint8)


def _gpu_map(planes, alpha, n, device, view='plain', stats=False):
    """planes: four (time, y, x) arrays.  view: 'plain'; 'crop' -- a column crop of a wider stack (row stride > nx, the
    launch that is not flat); 'sx2' -- every second column of a wider stack (stride_x = 2, the kernel without buffer loads)."""
    import torch
    from nd_amd import kernels
    ts = []
    for p in planes:
        k, ny, nx = p.shape
        if view == 'plain':
            t = torch.from_numpy(np.ascontiguousarray(p)).to(device)
        elif view == 'crop':
            wide = torch.full((k, ny, nx + 7), 1.0, dtype=torch.from_numpy(p).dtype, device=device)
            wide[:, :, 3:3 + nx] = torch.from_numpy(np.ascontiguousarray(p)).to(device)
            t = wide[:, :, 3:3 + nx]
        else:
            wide = torch.full((k, ny, 2 * nx), 1.0, dtype=torch.from_numpy(p).dtype, device=device)
            wide[:, :, ::2] = torch.from_numpy(np.ascontiguousarray(p)).to(device)
            t = wide[:, :, ::2]
        ts.append(t)
    out = kernels.change_detection(*ts, alpha=alpha, n=n, stats=stats)
    torch.cuda.synchronize()
    return (out[0] if stats else out).cpu().numpy()


def _check(oracle, device, planes, alpha, n, view='plain', want=None):
    k = planes[0].shape[0]
    dtype = planes[0].dtype.type
    assert _uses(dtype, k, alpha, n, stride_x=2 if view == 'sx2' else 1) == _rule(dtype, k, alpha, n, False)
    if want is None:
        want = _want(oracle, planes, alpha, n)
    got = _gpu_map(planes, alpha, n, device, view)
    assert got.shape == want.shape and got.dtype == np.uint8
    nbad = int((got != want).sum())
    assert nbad == 0, '%d change-map bytes differ (k=%d alpha=%g n=%d %s)' % (nbad, k, alpha, n, view)
    return want


# ---- stacks built for the form -------------------------------------------------------------------------
def quiet_background(seed, k, ny, nx, dtype=np.float32):
    """Stationary Wishart background of 200 looks: tested with n <= 9 its statistic stays far below every threshold
    used here, so no background pixel is a candidate and the candidates are exactly the planted pixels."""
    return [np.array(p, dtype=np.float64) for p in synth.omnibus_stack(seed, k, ny, nx, looks=200, dtype=np.float64,
                                                                        change_frac=0)]


def plant_steps(planes, pixels, factor=16.0, t0s=None):
    """x factor from date t0 on at the given (y, x) pixels; t0 cycles through the middle third of the series, where a
    step makes the whole-series test fire for certain (a single low date at the start would not)"""
    k = planes[0].shape[0]
    for i, (y, x) in enumerate(pixels):
        t0 = t0s[i] if t0s is not None else k // 3 + i % (k // 3 + 1)
        for p in planes:
            p[t0:, y, x] *= factor
    return planes


def wave_pixels(counts, first_last=True):
    """One row of len(counts) (+ 2) waves of 64 pixels; wave w holds exactly counts[w] planted pixels, spread over its
    lanes; the two extra waves hold one candidate each, in lane 0 and in lane 63."""
    px = []
    for w, c in enumerate(counts):
        lanes = np.linspace(0, 63, c).round().astype(int) if c > 1 else ([31] if c == 1 else [])
        assert len(set(lanes)) == c
        px += [(0, 64 * w + int(l)) for l in lanes]
    nw = len(counts)
    if first_last:
        px += [(0, 64 * nw), (0, 64 * (nw + 1) + 63)]
        nw += 2
    return px, nw


COUNTS = [0, 1, 2, 3, 15, 16, 64]


def counted_stack(k, seed=5):
    px, nw = wave_pixels(COUNTS)
    planes = plant_steps(quiet_background(seed, k, 1, 64 * nw), px)
    return [p.astype(np.float32) for p in planes], px, nw


# ---- the cases -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('alpha', [0.95, 0.99, 0.999])
@pytest.mark.parametrize('n', [4, 9])
@pytest.mark.parametrize('k', [2, 3, 8, 9, 16, 17, 24, 25, 32])
def test_series_lengths_and_looks(oracle, device, k, n, alpha):
    """Both sides of every KMAX, one group per wave (k = 24: two) and many, k = 2 with its single start; 5 x 333: two
    blocks per row, the last wave of a row partly outside, slices that are not 16-byte aligned."""
    planes = synth.omnibus_stack(seed=90 + k, k=k, ny=5, nx=333, dtype=np.float32, change_frac=0.08, factor=16.0)
    want = _check(oracle, device, planes, alpha, n)
    if k >= 3:
        assert 0 < int(want.sum()) < want.size


@gpu
@pytest.mark.parametrize('view', ['plain', 'crop', 'sx2'])
@pytest.mark.parametrize('shape', [(1, 1), (3, 64), (5, 333), (2, 257)])
@pytest.mark.parametrize('k', [9, 24])
def test_rasters_and_strides(oracle, device, k, shape, view):
    """idle lanes, a last wave partly outside, unaligned slices (the per-lane store), a row stride beyond nx, stride_x = 2"""
    ny, nx = shape
    planes = synth.omnibus_stack(seed=7 * k + nx, k=k, ny=ny, nx=nx, dtype=np.float32, change_frac=0.1)
    _check(oracle, device, planes, 0.99, 9, view)


@gpu
@pytest.mark.parametrize('k', [9, 16, 24])
def test_candidates_per_wave_by_construction(oracle, device, k):
    """Exactly 0, 1, 2, 3, 15, 16 and 64 candidates in a wave (odd counts leave a group idle; 15 is the last in-wave count,
    16 and 64 take the dense path of the same call), candidates in lane 0 and in lane 63; 9 waves: three blocks that differ."""
    planes, px, nw = counted_stack(k)
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    _, _, P = oracle.change_detection_planes(yxt, 0.99, 9, njobs=8, stats=True)
    # the construction holds: the whole-series test fires in the planted pixels (P = 1 to rounding) and nowhere near
    # the threshold elsewhere, so the screen's candidates are these pixels
    planted = np.zeros(64 * nw, dtype=bool)
    planted[[x for _, x in px]] = True
    assert (P[0][planted] > 0.9999).all() and (P[0][~planted] < 0.5).all()
    assert [int(planted[64 * w:64 * w + 64].sum()) for w in range(nw)] == COUNTS + [1, 1]
    want = _check(oracle, device, planes, 0.99, 9)
    assert (want.reshape(-1, k).sum(axis=1)[planted] >= 1).all()
    assert want.reshape(-1, k)[~planted].sum() == 0


@gpu
@pytest.mark.parametrize('k', [8, 17, 24])
def test_many_segments_per_pixel(oracle, device, k):
    """series that alternate between two levels every 1, 2 and 3 dates -- long chains, changes at date 1 and at the last
    date -- a few per wave, between steps at the first and the last date"""
    ny, nx = 2, 300
    planes = quiet_background(11 + k, k, ny, nx)
    rng = np.random.default_rng(k)
    xs = rng.choice(nx, size=24, replace=False)
    for i, x in enumerate(xs):
        y = i % ny
        period = 1 + i % 3
        level = np.where((np.arange(k) // period) % 2 == 1, 16.0, 1.0)
        if i % 8 == 6:
            level = np.where(np.arange(k) >= 1, 1.0, 16.0)             # one change, at date 1
        if i % 8 == 7:
            level = np.where(np.arange(k) >= k - 1, 16.0, 1.0)         # one change, at the last date
        for p in planes:
            p[:, y, x] *= level
    planes = [p.astype(np.float32) for p in planes]
    want = _check(oracle, device, planes, 0.99, 9)
    rows = want.reshape(-1, k)
    assert rows[:, 1].any() and rows[:, k - 1].any()
    if k >= 8:
        assert rows.sum(axis=1).max() >= k // 2                         # a chain over most of the series


@gpu
@pytest.mark.parametrize('k', [9, 24])
def test_degenerate_values(oracle, device, k):
    """zero, negative and NaN determinants, +-inf, values x 1e-6 and x 1e6, inside candidate pixels and in their
    neighbours: they reach the exact evaluation.  The oracle decides what is right."""
    ny, nx = 3, 200
    planes = quiet_background(23 + k, k, ny, nx)
    px = [(y, x) for y in range(ny) for x in range(5, nx - 5, 9)]
    plant_steps(planes, px, factor=6.0)
    c11, c12r, c12i, c22 = planes
    for i, (y, x) in enumerate(px):
        t = (3 * i) % k
        for xx in (x, x + 1):                                            # the candidate and a neighbour
            kind = (i + (xx - x) * 5) % 10
            if kind == 0:
                for p in planes:
                    p[t, y, xx] = 0.0                                    # zero determinant
            elif kind == 1:
                c11[t, y, xx] = -c11[t, y, xx]                           # negative determinant
            elif kind == 2:
                c12r[t, y, xx] = np.nan
            elif kind == 3:
                c11[t, y, xx] = np.inf
            elif kind == 4:
                c22[t, y, xx] = -np.inf
            elif kind == 5:
                for p in planes:
                    p[:, y, xx] *= 1e-6
            elif kind == 6:
                for p in planes:
                    p[:, y, xx] *= 1e6
            elif kind == 7:
                c12r[t, y, xx] = 10.0 * c11[t, y, xx]                    # |c12|^2 > c11 c22
            elif kind == 8:
                for p in planes:
                    p[t, y, xx] *= 1e-6                                  # one date far below the others
            # kind 9: left as it is
    with np.errstate(all='ignore'):
        planes = [p.astype(np.float32) for p in planes]
    want = _check(oracle, device, planes, 0.99, 9)
    assert want.sum() > 0
    _check(oracle, device, planes, 0.95, 4)


_CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from nd_amd import kernels, _lib
d = np.load(sys.argv[1])
for i in range(int(d['ncase'])):
    planes = [torch.from_numpy(d['p%%d_%%d' %% (i, v)]).cuda() for v in range(4)]
    alpha, n = float(d['alpha%%d' %% i]), int(d['n%%d' %% i])
    k = planes[0].shape[0]
    assert _lib.lib().nd_amd_omnibus_c2_uses_wave_search(0, k, 1, alpha, n, 0) == 0
    got = kernels.change_detection(*planes, alpha=alpha, n=n).cpu().numpy()
    assert np.array_equal(got, d['want%%d' %% i]), (i, int((got != d['want%%d' %% i]).sum()))
print('ok')
'''


@gpu
def test_two_pass_form_stays_pinned(oracle, device):
    """ND_AMD_WAVE_SEARCH=0 (read once per process, hence the child): the two-pass form on three of the cases above,
    against the same oracle maps"""
    cases = [(counted_stack(24)[0], 0.99, 9),
             (list(synth.omnibus_stack(seed=90 + 9, k=9, ny=5, nx=333, dtype=np.float32, change_frac=0.08, factor=16.0)), 0.99, 4),
             (list(synth.omnibus_stack(seed=7 * 24 + 257, k=24, ny=2, nx=257, dtype=np.float32, change_frac=0.1)), 0.99, 9)]
    data = {'ncase': len(cases)}
    for i, (planes, alpha, n) in enumerate(cases):
        want = _check(oracle, device, planes, alpha, n)                 # the new form, in this process
        data['want%d' % i] = want
        data['alpha%d' % i] = alpha
        data['n%d' % i] = n
        for v in range(4):
            data['p%d_%d' % (i, v)] = planes[v]
    with tempfile.TemporaryDirectory(prefix='nd_amd_ws_') as tmp:
        path = os.path.join(tmp, 'cases.npz')
        np.savez(path, **data)
        out = subprocess.run([sys.executable, '-c', _CHILD % ROOT, path], env=dict(os.environ, ND_AMD_WAVE_SEARCH='0'),
                             capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr[-2000:]


@gpu
def test_rasters_and_float64_keep_the_old_form(oracle, device):
    """stats=True and float64 at 24 dates: the predicate says "old form", and the maps equal the oracle's"""
    planes = list(synth.omnibus_stack(seed=61, k=24, ny=4, nx=300, dtype=np.float32, change_frac=0.1))
    assert not _uses(np.float32, 24, 0.99, 9, stats=True)
    want = _want(oracle, planes, 0.99, 9)
    assert np.array_equal(_gpu_map(planes, 0.99, 9, device, stats=True), want)
    planes64 = list(synth.omnibus_stack(seed=62, k=24, ny=4, nx=300, dtype=np.float64, change_frac=0.1))
    assert not _uses(np.float64, 24, 0.99, 9)
    want64 = _want(oracle, planes64, 0.99, 9)
    assert np.array_equal(_gpu_map(planes64, 0.99, 9, device), want64)
    assert want.sum() > 0 and want64.sum() > 0


def test_predicate_matches_the_rule():
    """host only: dtype x k x alpha x stats x stride against the rule of DESIGN 5, K1"""
    for dtype in (np.float32, np.float64):
        for k in (1, 2, 3, 8, 9, 16, 17, 24, 25, 32, 33, 48):
            for alpha in (0.01, 0.5, 0.9, 0.93, 0.95, 0.97, 0.9899, 0.99, 0.999):
                for stats in (False, True):
                    for sx in (1, 2, 24):
                        for n in (4, 9):
                            assert _uses(dtype, k, alpha, n, stats, sx) == _rule(dtype, k, alpha, n, stats), \
                                (dtype, k, alpha, stats, sx, n)
    # single-look data on a long series: no screen can decide the whole-series test, pass A evaluates it exactly
    assert not _uses(np.float32, 24, 0.99, 1)
    assert not _uses(np.float32, 24, float('nan'), 9)
