"""Long series -- 193 to 5200 dates -- through the HIP path against the CPU oracle.

Above 192 dates the fast forms of pass B end (fused, chain, starts and time-split forms; the float32
screen's table; the LDS image of the series from 147 float32 / 74 float64 dates on) and the per-pixel
sweep from memory (MODE 1 of omnibus_c2_search_kernel) takes every listed pixel, with pass A reading
the per-j table from device memory.  The series lengths sit on both sides of every edge on the way:
192 / 193 (the float32 screen), 256, 1024 (the tabulated 2 / m of the incomplete-gamma recurrences),
2047 / 2048 (MODE 1's screen constants, 32 (k + 1) bytes, beyond 64 KB of LDS) and 5200 (beyond the
CU's 160 KB: the constants read from global memory).

The data come from tests.synth.long_series_stack, which keeps the reference's double product of the
determinants in range (on plain data it leaves the range, P turns NaN and an all-zero map would pass);
every case first asserts from the oracle's own output that the maps are worth comparing
(synth.long_series_nonvacuity).  Change maps byte for byte, z / P to 1e-5 relative."""
import time

import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

ALPHAS = (1e-4, 0.01, 0.5, 0.99)
# (from 2000 dates on 1e-4 is left out: at 0.01 nearly every date is a change already, and then the sweep of a
#  pixel costs k^2 / 2 dates on one lane -- at 2048 dates one call ~1 s, at 5200 dates ~10 s)
LONG = (0.01, 0.5, 0.99)
NJOBS = 16
# (k, dtype, layout, ny, nx, thresholds): one stack per series length, each length with one element
# type and one layout; both workspaces at every threshold of the sparse regime, one of them (alternating)
# below it.  About 70 s in all on one MI355X (the oracle on 16 threads).
CASES = [
    (193, np.float32, 'tyx', 4, 64, ALPHAS),
    (194, np.float64, 'yxt', 4, 64, ALPHAS),
    (255, np.float32, 'pad', 4, 64, ALPHAS),
    (256, np.float64, 'tyx', 4, 64, ALPHAS),
    (257, np.float32, 'yxt', 4, 64, ALPHAS),
    (365, np.float64, 'pad', 4, 64, ALPHAS),
    (1023, np.float32, 'tyx', 4, 64, ALPHAS),
    (1024, np.float64, 'yxt', 4, 64, ALPHAS),
    (1025, np.float32, 'pad', 4, 64, ALPHAS),
    (2046, np.float32, 'yxt', 4, 48, LONG),
    (2047, np.float64, 'pad', 4, 48, LONG),
    (2048, np.float32, 'tyx', 4, 48, LONG),
    (4096, np.float64, 'yxt', 4, 32, LONG),
    (5200, np.float32, 'tyx', 2, 64, (0.5, 0.99)),
]
# n = 1 (the exact whole-series test of pass A) on some of the lengths
N1_LENGTHS = (193, 1024, 2048)


def _device_planes(planes, layout, device):
    """The four planar (time, y, x) arrays as device tensors in `layout`; returns (tensors, dims)."""
    import torch
    k, ny, nx = planes[0].shape
    if layout == 'tyx':
        return [torch.from_numpy(p).to(device) for p in planes], ('time', 'y', 'x')
    if layout == 'yxt':
        return ([torch.from_numpy(np.ascontiguousarray(np.moveaxis(p, 0, -1))).to(device) for p in planes],
                ('y', 'x', 'time'))
    # a strided view into a padded buffer, as tools/fuzz_parity.py's 'pad'
    big = torch.zeros((4, k, ny + 2, nx + 5), dtype=torch.from_numpy(planes[0]).dtype, device=device)
    for v in range(4):
        big[v, :, 1:ny + 1, 3:nx + 3] = torch.from_numpy(planes[v]).to(device)
    return [big[v, :, 1:ny + 1, 3:nx + 3] for v in range(4)], ('time', 'y', 'x')


def _oracle(oracle, planes, alpha, n):
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    with np.errstate(all='ignore'):
        return oracle.change_detection_planes(yxt, alpha, n, njobs=NJOBS, stats=True)


def _compare(got, want, what):
    ch, z, P = (t.cpu().numpy() for t in got)
    ch0, z0, P0 = want
    assert ch.shape == ch0.shape and ch.dtype == np.uint8
    nbad = int((ch != ch0).sum())
    assert nbad == 0, '%s: %d change-map bytes differ (%d changes expected)' % (what, nbad, int(ch0.sum()))
    np.testing.assert_allclose(z, z0, rtol=1e-5, atol=0, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(P, P0, rtol=1e-5, atol=1e-30, equal_nan=True, err_msg=what)


@pytest.mark.parametrize('k, dtype, layout, ny, nx, alphas', CASES, ids=[str(c[0]) for c in CASES])
def test_long_series_parity(oracle, device, k, dtype, layout, ny, nx, alphas):
    import torch
    from nd_amd import kernels
    t0 = time.perf_counter()
    planes, planted = synth.long_series_stack(seed=k, k=k, ny=ny, nx=nx, dtype=dtype)
    want = {a: _oracle(oracle, planes, a, 9) for a in alphas}
    t_oracle = time.perf_counter() - t0
    counts, nnan = synth.long_series_nonvacuity(k, {a: w[0] for a, w in want.items()}, want[alphas[-1]][2], ny * nx)
    # the planted pixels whose product dips into the subnormal range keep a finite test and do change
    sub = planted['subnormal']
    assert all(np.isfinite(want[alphas[-1]][1][y, x]) for y, x in sub)
    assert any(want[alphas[-1]][0][y, x].any() for y, x in sub)
    dev, dims = _device_planes(planes, layout, device)
    t1 = time.perf_counter()
    for i, alpha in enumerate(alphas):
        wss = ('recommended', 'minimal') if alpha >= 0.5 else (('recommended', 'minimal')[(k + i) % 2],)
        for ws in wss:
            got = kernels.change_detection(*dev, alpha=alpha, n=9, dims=dims, stats=True, workspace=ws)
            torch.cuda.synchronize()
            _compare(got, want[alpha], 'k %d %s %s alpha %g %s' % (k, np.dtype(dtype).name, layout, alpha, ws))
    t_gpu = time.perf_counter() - t1
    if k in N1_LENGTHS:
        # n = 1 on nine-look data: omega2 of the long tests leaves [0, 1] and the reference's P is 0 -- no change
        # anywhere; what is compared is the exact evaluation of pass A (z and P of every pixel)
        for alpha in (0.01, 0.99):
            w1 = _oracle(oracle, planes, alpha, 1)
            assert np.isfinite(w1[1]).sum() >= 0.8 * ny * nx and np.unique(w1[1][np.isfinite(w1[1])]).size > ny * nx // 2
            for ws in ('recommended', 'minimal'):
                got = kernels.change_detection(*dev, alpha=alpha, n=1, dims=dims, stats=True, workspace=ws)
                torch.cuda.synchronize()
                _compare(got, w1, 'k %d n 1 alpha %g %s' % (k, alpha, ws))
    print('\nk %d %s %s %dx%d: changes / changed pixels by alpha %s, P = NaN in %d pixels; oracle %.2f s, GPU %.2f s'
          % (k, np.dtype(dtype).name, layout, ny, nx, counts, nnan, t_oracle, t_gpu))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_pixel_major_declines_long_series(oracle, device, dtype):
    """kernels.change_detection_pixel_major returns None beyond its register / LDS sizes (k > 192, or k not a
    multiple of the 16-byte vector) and never a wrong map; within them its map is the oracle's."""
    import torch
    from nd_amd import kernels
    ve = 16 // np.dtype(dtype).itemsize
    for k in (30 if ve == 4 else 29, 192, 193, 200, 365):
        planes, _ = synth.long_series_stack(seed=50 + k, k=k, ny=3, nx=40, dtype=dtype)
        yxt = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(p, 0, -1))).to(device) for p in planes]
        for alpha in (0.5, 0.99):
            res = kernels.change_detection_pixel_major(*yxt, alpha=alpha, n=9, stats=True)
            if k > 192 or k % ve:
                assert res is None, 'k %d: the pixel-major kernel took a series it does not serve' % k
            elif res is not None:
                torch.cuda.synchronize()
                _compare(res, _oracle(oracle, planes, alpha, 9), 'pixel-major k %d alpha %g' % (k, alpha))


@pytest.mark.parametrize('k', [365, 2048])
def test_omnibus_class_long_series(oracle, device, k):
    """OmnibusTest(n=9).apply on a (y, x, time) dataset -- numpy planes, and device tensors with a complex C12 --
    equals the oracle: the pixel-major kernel declines, the class transposes and takes the planar path."""
    import torch
    from nd_amd import xr_lite
    from nd_amd.change import OmnibusTest
    planes, _ = synth.long_series_stack(seed=900 + k, k=k, ny=3, nx=48, dtype=np.float32)
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    host = xr_lite.Dataset()
    for v, a in zip(('C11', 'C12__re', 'C12__im', 'C22'), yxt):
        host[v] = (('y', 'x', 'time'), a)
    dev = xr_lite.Dataset()
    dev['C11'] = (('y', 'x', 'time'), torch.from_numpy(yxt[0]).to(device))
    dev['C12'] = (('y', 'x', 'time'), torch.complex(torch.from_numpy(yxt[1]), torch.from_numpy(yxt[2])).to(device))
    dev['C22'] = (('y', 'x', 'time'), torch.from_numpy(yxt[3]).to(device))
    for alpha in (0.5, 0.99):
        with np.errstate(all='ignore'):
            want = oracle.change_detection_planes(yxt, alpha, 9, njobs=NJOBS).astype(bool)
        assert want.any(axis=-1).sum() >= 30 and want[..., 192:].any()
        got = OmnibusTest(alpha=alpha, n=9).apply(host)
        assert got.dims == ('y', 'x', 'time')
        np.testing.assert_array_equal(got.values, want, err_msg='host k %d alpha %g' % (k, alpha))
        got = OmnibusTest(alpha=alpha, n=9).apply(dev)
        assert got.values.is_cuda
        np.testing.assert_array_equal(got.values.cpu().numpy(), want, err_msg='device k %d alpha %g' % (k, alpha))


def test_omnibus_class_multilooked_long_series(oracle, device):
    """OmnibusTest(ml=3) at 365 dates: the fused multilooking kernel stops at 24 dates, so this is the two-step
    path (boxcar kernel, then the plain test with n = 9); equal to scipy's boxcar followed by the oracle."""
    import scipy.ndimage as ndi
    import torch
    from nd_amd import xr_lite
    from nd_amd.change import OmnibusTest
    k = 365
    # (two-look data: the boxcar brings them to about the n = 9 the test assumes)
    planes, _ = synth.long_series_stack(seed=365, k=k, ny=10, nx=40, looks=2, dtype=np.float32, plant=False)
    kern = (np.ones((3, 3), dtype=np.float64) / 9).reshape(1, 3, 3)
    mlp = [np.ascontiguousarray(np.moveaxis(ndi.convolve(p, kern), 0, -1)) for p in planes]
    ds = xr_lite.Dataset()
    for v, p in zip(('C11', 'C12__re', 'C12__im', 'C22'), planes):
        ds[v] = (('time', 'y', 'x'), torch.from_numpy(p).to(device))
    for alpha in (0.5, 0.99):
        with np.errstate(all='ignore'):
            want = oracle.change_detection_planes(mlp, alpha, 9, njobs=NJOBS).astype(bool)
        assert want.any(axis=-1).sum() >= 20 and want[..., 192:].any()
        got = OmnibusTest(ml=3, alpha=alpha).apply(ds)
        np.testing.assert_array_equal(got.values.cpu().numpy(), want, err_msg='alpha %g' % alpha)


@pytest.mark.parametrize('k', [97, 200])
def test_full_pol_beyond_table_is_an_error(device, k):
    """The full-pol test ends at 96 dates (its per-j table travels as a kernel argument): beyond, a clear error
    through the kernel entry point and through OmnibusTest(pol='full'), not an output."""
    import torch
    from nd_amd import kernels, xr_lite
    from nd_amd._lib import NdAmdError
    from nd_amd.change import OmnibusTest
    planes = synth.wishart_c3(np.random.default_rng(k), (k, 3, 20))
    dev = [torch.from_numpy(p).to(device) for p in planes]
    with pytest.raises(NdAmdError, match='exceeds the supported 96 dates'):
        kernels.change_detection_c3(dev, alpha=0.9, n=9)
    names = ('C11', 'C22', 'C33', 'C12', 'C13', 'C23')
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    ds = xr_lite.Dataset()
    for i, name in enumerate(names[:3]):
        ds[name] = (('y', 'x', 'time'), yxt[i])
    for i, name in enumerate(names[3:]):
        ds[name] = (('y', 'x', 'time'), (yxt[3 + 2 * i] + 1j * yxt[4 + 2 * i]).astype(np.complex64))
    with pytest.raises(NdAmdError, match='exceeds the supported 96 dates'):
        OmnibusTest(n=9, alpha=0.9, pol='full').apply(ds)
