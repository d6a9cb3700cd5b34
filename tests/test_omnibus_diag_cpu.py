"""The intensity-only omnibus test (pol='diag') without a GPU: the numpy restatement
tests/omnibus_diag_ref.py pinned to the oracle for the reference's 2 x 2 structure, the constants and the
calibration of the block-diagonal test, the golden file the GPU tests compare with, and the argument
checks of the C entry point and of the public interface (both run before anything touches a device)."""
import ctypes as C

import numpy as np
import pytest

from tests import omnibus_diag_cases as cases
from tests import omnibus_diag_ref as R
from tests import synth


def _inject(planes, seed):
    """NaN, 0, negative and inf samples in a copy of the planes."""
    rng = np.random.default_rng(seed)
    planes = [p.copy() for p in planes]
    for val in (np.nan, 0.0, -1.0, np.inf):
        for p in planes:
            p[rng.random(p.shape) < 0.02] = val
    return planes


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('k', [2, 5, 12])
@pytest.mark.parametrize('inject', [False, True])
def test_restatement_equals_the_oracle_for_the_2x2_structure(oracle, dtype, k, inject):
    """Structure (2,) is the reference's own test: map, z and P equal oracle.change_detection bit for bit, which
    pins the restatement's rounding points, its search and its CDF."""
    planes = list(synth.omnibus_stack(seed=k, k=k, ny=6, nx=7, dtype=dtype))
    if inject:
        planes = _inject(planes, k)
    values = np.stack([np.moveaxis(p, 0, -1) for p in planes], axis=-1)       # (y, x, time, 4)
    changes = 0
    for n in (1, 9):
        series = R.Series(planes, (2,), n)
        for alpha in (0.01, 0.9):
            with np.errstate(all='ignore'):
                want, z0, P0 = oracle.change_detection(values, alpha, n, stats=True)
            got, z, P = R.change_detection(planes, (2,), alpha, n, series=series)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(z, z0)
            np.testing.assert_array_equal(P, P0)
            changes += int(want.sum())
    assert changes > 0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_q2_log_q_equals_the_2x2_log_q_with_zero_off_diagonals(dtype):
    planes = cases.gamma_stack(3, 2, 12, 6, 7, 4.4, dtype)
    zero = np.zeros_like(planes[0])
    for n in (1, 4.4, 9):
        a = R.log_q(planes, (1, 1), n)
        b = R.log_q([planes[0], zero, zero, planes[1]], (2,), n)
        np.testing.assert_array_equal(a, b)
        assert np.isfinite(a).all()


@pytest.mark.parametrize('q, j, n, f, rho, omega2', [
    (1, 2, 1, 1.0, 0.75, -1.0 / 36.0),
    (2, 10, 4.4, 18.0, 1.0 - (10 / 4.4 - 1 / 44.0) / 54.0, -0.00850661625708),
    (3, 24, 9, 69.0, 1.0 - (24 / 9.0 - 1 / 216.0) / 138.0, -0.00667387419286),
])
def test_constants(oracle, q, j, n, f, rho, omega2):
    got = R.constants((1,) * q, j, n)
    assert got[0] == f
    assert got[1] == pytest.approx(rho, rel=1e-12)
    assert got[2] == pytest.approx(-(q * (j - 1) / 4.0) * (1.0 - 1.0 / rho) ** 2, rel=1e-12)
    assert got[2] == pytest.approx(omega2, rel=1e-11)          # the literal is cut after twelve digits


@pytest.mark.parametrize('q, k, n', [(1, 10, 4.4), (2, 10, 4.4), (3, 24, 9)])
def test_calibration_under_the_null(oracle, q, k, n):
    """200 000 gamma(n, 1/n) series in float64: the share of P > a is within 0.004 of 1 - a (three standard
    deviations of the sampling, 0.0034 at a = 0.5, plus the residual of the expansion), and the uncorrected
    statistic (rho = 1, omega2 = 0) misses that band at a = 0.5."""
    rng = np.random.default_rng(100 * q + k)
    planes = [rng.gamma(n, 1.0 / n, (k, 200000)) for _ in range(q)]
    z, P = R.single_test(planes, (1,) * q, n)
    for a in (0.5, 0.9, 0.99):
        assert abs(float((P > a).mean()) - (1.0 - a)) <= 0.004, a
    f = R.constants((1,) * q, k, n)[0]
    raw = R._p_of((-2.0 * R.log_q(planes, (1,) * q, n)), np.float64, f, 0.0)
    assert abs(float((raw > 0.5).mean()) - 0.5) > 0.004


def test_golden_file_reproduces(oracle):
    """tests/golden/omnibus_diag.npz is what the restatement gives for the recorded seeds, and no recorded
    decision lies within 16 ulp(T) of its threshold."""
    golden = cases.Golden()
    assert golden.names == [c['name'] for c in cases.cases()]
    for name in golden.names:
        case = golden.case(name)
        planes = cases.make_input(case)
        series = R.Series(planes, (1,) * case['q'], case['n'])
        for alpha in case['alphas']:
            want, z0, P0, closest = golden.expected(name, alpha)
            got, z, P = R.change_detection(planes, (1,) * case['q'], alpha, case['n'], series=series)
            np.testing.assert_array_equal(got, want, err_msg=name)
            np.testing.assert_array_equal(z, z0, err_msg=name)
            np.testing.assert_array_equal(P, P0, err_msg=name)
            assert series.closest == closest and closest > 16 * cases.ulp(alpha, case['dtype']), name


def test_step_change_on_the_restatement(oracle):
    """nd/tests/test_change_omnibus.py for q = 1 and 2: exactly one change per pixel, at date 5."""
    for q in (1, 2):
        planes = cases.step_stack(11, q, np.float64)
        got = R.change_detection(planes, (1,) * q, 0.9, 9)[0]
        assert (got.sum(axis=-1) == 1).all() and (got[..., 5] == 1).all()


def test_c_entry_validation():
    """nd_amd_omnibus_diag rejects a bad channel count, dtype and number of looks before any HIP call (this
    machine has no device to call), and an empty raster is served."""
    from nd_amd import _lib
    L = _lib.lib()
    buf = np.ones(64, np.float32)
    out = np.zeros(64, np.uint8)
    ws = np.zeros(1 << 16, np.uint8)
    ptrs = (C.c_void_p * 4)(*[buf.ctypes.data] * 4)

    def call(nch=2, dtype=_lib.F32, shape=(2, 4, 4), n=4.4):
        return L.nd_amd_omnibus_diag(ptrs, nch, dtype, shape[0], shape[1], shape[2], 4, 1, 16, n, 0.5,
                                     C.c_void_p(out.ctypes.data), None, None, C.c_void_p(ws.ctypes.data), ws.nbytes,
                                     None)
    assert call(nch=0) == _lib.EINVAL and b'channels' in L.nd_amd_last_error()
    assert call(nch=4) == _lib.EINVAL
    assert call(dtype=7) == _lib.EINVAL
    for n in (0.0, -1.0, float('inf'), float('nan')):
        assert call(n=n) == _lib.EINVAL and b'n_looks' in L.nd_amd_last_error()
    assert call(shape=(-1, 4, 4)) == _lib.EINVAL
    for shape in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert call(shape=shape) == _lib.OK
    assert L.nd_amd_omnibus_diag_workspace_bytes(_lib.F32, 2, 16, 16, 10) > 0
    assert L.nd_amd_omnibus_diag_workspace_bytes(_lib.F32, 4, 16, 16, 10) == 0
    assert L.nd_amd_omnibus_diag_workspace_bytes(9, 2, 16, 16, 10) == 0


def test_python_errors():
    """The channel checks of OmnibusTest(pol='diag') name the variables and come before any device work."""
    from nd_amd import xr_lite
    from nd_amd.change import OmnibusTest, omnibus_statistics
    a = np.ones((3, 4, 5), np.float32)
    ds = xr_lite.Dataset()
    ds['C12'] = (('y', 'x', 'time'), a.astype(np.complex64))
    with pytest.raises(KeyError, match='C12'):
        OmnibusTest(pol='diag').apply(ds)
    ds['VV'] = (('y', 'x', 'time'), a)
    with pytest.raises(KeyError, match='VH'):
        OmnibusTest(pol='diag', channels=['VV', 'VH']).apply(ds)
    with pytest.raises(TypeError, match='C12'):
        OmnibusTest(pol='diag', channels=['VV', 'C12']).apply(ds)
    with pytest.raises(ValueError, match='one to three'):
        omnibus_statistics(ds, pol='diag', channels=['VV'] * 4)
    with pytest.raises(ValueError, match="'dual'.*'full'.*'diag'"):
        OmnibusTest(pol='quad').apply(ds)
