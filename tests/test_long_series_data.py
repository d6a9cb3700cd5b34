"""The long-series generator (tests.synth.long_series_stack) under the CPU oracle, no GPU: what makes
tests/test_long_series_gpu.py and the fuzz family 'omnibus_long' worth running must stay true of the data
-- changes in many pixels, after date 192 and after date 2047, few P = NaN, counts that move with the
threshold, and the planted pixels whose running product of determinants goes subnormal, to 0 or to inf."""
import numpy as np
import pytest

from tests import synth

TINY = np.finfo(np.float64).tiny


@pytest.mark.parametrize('k, dtype, alphas', [(300, np.float32, (0.5, 0.99)),
                                              (1100, np.float64, (0.01, 0.99)),
                                              (2100, np.float32, (0.5, 0.99))])
def test_long_series_stack_is_not_vacuous(oracle, k, dtype, alphas):
    ny, nx = 2, 40
    planes, planted = synth.long_series_stack(seed=k, k=k, ny=ny, nx=nx, dtype=dtype)
    assert all(p.shape == (k, ny, nx) and p.dtype == dtype for p in planes)
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    maps = {}
    with np.errstate(all='ignore'):
        for a in alphas:
            maps[a], z, P = oracle.change_detection_planes(yxt, a, 9, njobs=4, stats=True)
    synth.long_series_nonvacuity(k, maps, P, ny * nx)
    # the ordinary pixels (rows 1 ..) keep every running product from date 0 in the normal range
    for x in range(nx):
        rp = np.abs(synth.running_products(planes, 1, x))
        assert ((rp >= TINY) & (rp < np.inf)).all(), (1, x)
    # the planted ones reach what they were planted for, and the subnormal dip comes back
    for y, x in planted['subnormal']:
        rp = np.abs(synth.running_products(planes, y, x))
        assert ((rp > 0) & (rp < TINY)).any() and (rp > 0).all() and TINY <= rp[-1] < np.inf, (y, x)
        assert np.isfinite(z[y, x])
    assert any(maps[alphas[-1]][y, x].any() for y, x in planted['subnormal'])
    for y, x in planted['underflow']:
        rp = synth.running_products(planes, y, x)
        assert (rp == 0).any() and ((rp > 0) & (rp < TINY)).any(), (y, x)
    for y, x in planted['overflow']:
        assert np.isinf(synth.running_products(planes, y, x)).any(), (y, x)
    for y, x in planted['nodata']:
        assert all((p[:, y, x] == 0).all() for p in planes)
    for kind in ('nan', 'inf'):
        for y, x in planted[kind]:
            assert np.isnan(P[y, x]), (kind, y, x)
            assert not any(m[y, x].any() for m in maps.values())
