"""The reference side of the coregistration edge tests, without a GPU: the numpy restatement
(tests/coreg_ref.py) is right at odd sizes, and the cases of tests/coreg_cases.py are ones whose
shifts the near-tie rule decides."""
import numpy as np
import pytest

from tests import coreg_cases as cases
from tests import coreg_ref


@pytest.mark.parametrize('size', cases.FOURIER_CPU_SIZES, ids=lambda s: '%dx%d' % s)
def test_restatement_recovers_fourier_shifts(size):
    """An oracle that owes nothing to scikit-image: a band-limited periodic image moved with a phase
    ramp by multiples of 1 / u comes back with exactly that shift, at the odd sizes of the case table."""
    ny, nx = size
    rng = np.random.default_rng(1000 * ny + nx)
    for u in cases.FOURIER_CPU_FACTORS:
        ref = cases.bandlimited(rng, ny, nx)
        for dy, dx in cases.grid_shifts(rng, u, 4):
            got = coreg_ref.phase_shift(cases.fourier_shift(ref, dy, dx), ref, u)
            np.testing.assert_allclose(got, (dy, dx), rtol=0, atol=1e-9, err_msg='%dx%d u=%d' % (ny, nx, u))


@pytest.mark.parametrize('case', cases.CASES, ids=cases.case_id)
def test_cases_are_decided(case):
    """The condition on the cases: at least 4 of the 5 non-reference dates are decided in every type
    the GPU tests run (the counts are recorded in coreg_cases' docstring)."""
    ny, nx, u = case
    for dtype in (np.float32, np.float64) if case in cases.F64_CASES else (np.float32,):
        sh, ok = cases.case_reference(ny, nx, u, dtype)
        print('%s %s: %d of %d dates decided' % (cases.case_id(case), np.dtype(dtype).name, ok[1:].sum(), cases.K - 1))
        assert ok[0] and ok[1:].sum() >= 4
        np.testing.assert_array_equal(sh, coreg_ref.shifts(cases.c11_stack(ny, nx, u, dtype), 0, u))
        assert (sh[0] == 0).all() and np.abs(sh[1:]).max() > 0.5
        np.testing.assert_allclose(sh * u, np.round(sh * u), rtol=0, atol=1e-9)
        for axis in (0, 1):
            if case[axis] == 1:
                assert (sh[:, axis] == 0).all()


@pytest.mark.parametrize('case', cases.FOURIER_CASES, ids=cases.case_id)
def test_fourier_cases_are_decided(case):
    ny, nx, u = case
    a, applied = cases.fourier_stack(ny, nx, u)
    for dtype in (np.float64, np.float32):
        sh, ok = cases.fourier_reference(ny, nx, u, dtype)
        assert ok.all()
        np.testing.assert_allclose(sh, applied, rtol=0, atol=1e-9)


def test_rule_sees_a_tie():
    """A half-pixel Fourier shift ties two whole-pixel cells: the rule must not call that decided."""
    rng = np.random.default_rng(5)
    ref = cases.bandlimited(rng, 31, 37)
    src = cases.fourier_shift(ref, 1.5, 0.0)
    for dtype in (np.float64, np.float32):
        sh, ok = cases.decided(src.astype(dtype), ref.astype(dtype), 2)
        assert not ok
        np.testing.assert_allclose(sh, (1.5, 0.0), rtol=0, atol=1e-9)


@pytest.mark.parametrize('shape', [(17, 65), (33, 129), (1, 65), (63, 1)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_warp_stack_agrees_with_warp_pixels(shape, dtype):
    """warp_stack (whole planes, what the GPU tests compare with) against warp_pixels on the seam rows
    and columns of the 16 x 64 tiles, for every row of the table of shifts."""
    nr, nc = shape
    planes = cases.warp_planes(nr, nc, dtype)
    sh = cases.warp_shifts(nr, nc)
    rows = np.array(sorted({r for r in (0, 1, 15, 16, 17, 31, 32, 33, nr - 1) if 0 <= r < nr}))
    cols = np.array(sorted({c for c in (0, 1, 63, 64, 65, 127, 128, nc - 1) if 0 <= c < nc}))
    for name, a in planes.items():
        whole = coreg_ref.warp_stack(a, sh, cases.WARP_REF)
        np.testing.assert_array_equal(whole[cases.WARP_REF], a[cases.WARP_REF])
        for t in range(len(sh)):
            if t != cases.WARP_REF:
                part = coreg_ref.warp_pixels(a[t], sh[t, 0], sh[t, 1], rows, cols)
                np.testing.assert_array_equal(whole[t][rows][:, cols], part, err_msg='%s date %d' % (name, t))
    # what the table promises of its rows
    pos = coreg_ref.warp_stack(planes['pos'], sh, cases.WARP_REF)
    assert (pos[7] == 0).all() and (pos[8] == 0).all()                    # the whole plane outside
    for t in (0, 10):                                                     # no shift, or a non-finite one
        np.testing.assert_array_equal(pos[t], planes['pos'][t])
    nan = coreg_ref.warp_stack(planes['nan'], sh, cases.WARP_REF)
    assert not np.isnan(nan[[0, 1, 2, 3, 5]]).any()
    assert np.isnan(nan[4]).any() == (nr > 4)                             # a single row is moved outside


def test_minmax_planes_place_the_extremes():
    """... and a bound taken from all but the extreme element changes the warped plane, so a lost
    partial of the min / max reduction cannot go unseen."""
    a = cases.minmax_planes(np.float32)
    flat = a.reshape(3, -1)
    n = flat.shape[1]
    assert n // (256 * 32) == 2                                           # two partial blocks per plane
    assert [(int(f.argmin()), int(f.argmax())) for f in flat] == [(0, n - 1), (n - 1, 0), (8191, 8192)]
    want = coreg_ref.warp_stack(a, cases.MINMAX_SHIFTS, -1)
    for t, (dy, dx) in enumerate(cases.MINMAX_SHIFTS):
        raw = coreg_ref.interpolate(a[t], dy, dx)
        lo2, hi2 = np.partition(flat[t], 1)[1], np.partition(flat[t], -2)[-2]
        assert not np.array_equal(coreg_ref.clip_preserve(raw.copy(), lo2, flat[t].max()), want[t])
        assert not np.array_equal(coreg_ref.clip_preserve(raw.copy(), flat[t].min(), hi2), want[t])
