"""GaussianFilter on the GPU: bit-equal to scipy.ndimage.gaussian_filter
(nd/tests/test_gaussian_filter.py:10-27 demand equality with scipy)."""
from collections import OrderedDict

import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu


def _gpu_gauss(a, sigma, device, **kw):
    import torch
    from nd_amd import kernels
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = kernels.gaussian_filter(t, sigma, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_against_scipy(device, dtype):
    import scipy.ndimage as ndi
    rng = np.random.default_rng(2)
    for shape, sigma in [((20, 20, 10), (1, 1, 0)), ((33, 17), 2.5), ((5, 40, 41), (0, 1.5, 0.7)),
                         ((64,), 3), ((3, 4, 5, 6), (0, 1, 0, 2)), ((10, 10), (0, 0)), ((4, 6), 8.0)]:
        a = rng.normal(size=shape).astype(dtype)
        np.testing.assert_array_equal(_gpu_gauss(a, sigma, device), ndi.gaussian_filter(a, sigma))
    a = rng.normal(size=(30, 31)).astype(dtype)
    for mode in ('reflect', 'constant', 'nearest', 'mirror', 'wrap'):
        np.testing.assert_array_equal(_gpu_gauss(a, 1.3, device, mode=mode, cval=0.3, truncate=3.0),
                                      ndi.gaussian_filter(a, 1.3, mode=mode, cval=0.3, truncate=3.0))


def test_correlate1d_general_kernels(device):
    import torch
    import scipy.ndimage as ndi
    from nd_amd import kernels
    rng = np.random.default_rng(3)
    a = rng.normal(size=(13, 29)).astype(np.float64)
    t = torch.from_numpy(a).to(device)
    for w in (rng.normal(size=5), rng.normal(size=4), np.array([1.0, 0.0, -1.0]), np.array([0.25, 0.5, 0.25])):
        for axis in (0, 1):
            out = torch.empty_like(t)
            kernels.correlate1d(t, w, axis, out)
            np.testing.assert_array_equal(out.cpu().numpy(), ndi.correlate1d(a, w, axis=axis))


@pytest.mark.parametrize('mode', ['reflect', 'constant', 'nearest', 'mirror', 'wrap'])
def test_per_element_1d_kernel_on_lines_shorter_than_the_kernel(device, mode):
    """The per-element correlate1d kernel and its line extension (extend_line, borders.hpp) many periods away from
    the line: lines of 1, 2 and 3 elements under kernels of 3, 8 and 13 taps, along each axis.  The arrays are views
    whose last axis is not contiguous, which the tiled kernel does not take.  Bit-equal to scipy."""
    import torch
    import scipy.ndimage as ndi
    from nd_amd import kernels
    rng = np.random.default_rng(1813)
    for shape in [(1, 2, 3), (3, 1, 2), (2, 3, 1)]:
        a = rng.normal(size=shape)
        wide = torch.zeros(shape[:2] + (2 * shape[2],), dtype=torch.float64, device=device)
        t = wide[..., ::2]
        t.copy_(torch.from_numpy(a))
        assert t.stride(-1) == 2
        for n in (3, 8, 13):
            w = rng.normal(size=n)
            for axis in (0, 1, 2):
                out = torch.empty_like(wide)[..., ::2]
                kernels.correlate1d(t, w, axis, out, mode, 0.75)
                np.testing.assert_array_equal(out.cpu().numpy(), ndi.correlate1d(a, w, axis=axis, mode=mode, cval=0.75),
                                              err_msg=str((shape, n, axis)))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_long_kernels_in_the_tiled_1d_kernel(device, dtype):
    """Kernels of 33 .. 97 taps (round 6: Gaussian sigma > 3.75 took the per-element kernel): sigma 5 / 8 / 12 along
    every axis of 3-D arrays (size classes 65 and 97, the filtered axis shorter than the kernel included), general
    (non-symmetric, antisymmetric, even) kernels of up to 97 taps, the border modes -- bit-equal to scipy."""
    import time
    import torch
    import scipy.ndimage as ndi
    from nd_amd import kernels
    rng = np.random.default_rng(97)
    for shape in [(3, 150, 200), (2, 40, 300), (20, 33, 129)]:
        a = rng.normal(size=shape).astype(dtype)
        for sigma in ((0, 5, 5), (0, 8, 0), (0, 0, 12), (5, 0, 0), (3.9, 4.1, 6.0)):
            for mode in ('reflect', 'wrap', 'constant'):
                np.testing.assert_array_equal(_gpu_gauss(a, sigma, device, mode=mode, cval=0.5),
                                              ndi.gaussian_filter(a, sigma, mode=mode, cval=0.5), err_msg=str((shape, sigma, mode)))
    a = rng.normal(size=(60, 170)).astype(dtype)
    t = torch.from_numpy(a).to(device)
    anti = rng.normal(size=48)
    anti = np.concatenate([-anti[::-1], [0.0], anti])
    for w in (rng.normal(size=33), rng.normal(size=64), rng.normal(size=97), anti, np.ones(41) / 41):
        for axis in (0, 1):
            for mode in ('nearest', 'mirror'):
                out = torch.empty_like(t)
                kernels.correlate1d(t, w, axis, out, mode)
                np.testing.assert_array_equal(out.cpu().numpy(), ndi.correlate1d(a, w, axis=axis, mode=mode))
    # the tiled kernel took them: sigma = 8 on 4 x 1024^2 in well under 5 ms
    x = torch.from_numpy(rng.normal(size=(4, 1024, 1024)).astype(dtype)).to(device)
    kernels.gaussian_filter(x, (0, 8, 8))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kernels.gaussian_filter(x, (0, 8, 8))
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 5e-3


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_tiled_1d_kernel_on_both_sides_of_its_size_classes(device, dtype):
    """The tiled 1-D kernel is instantiated for up to 9, 17, 25, 31, 65 and 97 taps: the last count of each class
    and the first of the next, along x and along y (from 32 taps on, the tile along y takes more than 64 KB of
    LDS), general kernels on planes of more than one tile -- bit-equal to scipy."""
    import torch
    import scipy.ndimage as ndi
    from nd_amd import kernels
    rng = np.random.default_rng(965)
    a = rng.normal(size=(2, 40, 140)).astype(dtype)
    t = torch.from_numpy(a).to(device)
    for n in (9, 10, 17, 18, 25, 26, 31, 32, 65, 66):
        w = rng.normal(size=n)
        for axis in (1, 2):
            out = torch.empty_like(t)
            kernels.correlate1d(t, w, axis, out)
            np.testing.assert_array_equal(out.cpu().numpy(), ndi.correlate1d(a, w, axis=axis), err_msg=str((n, axis)))


def test_gaussian_filter_class(device):
    """nd/tests/test_gaussian_filter.py:10-27 re-stated."""
    import scipy.ndimage as ndi
    from nd_amd.filters import GaussianFilter, gaussian
    ds = synth.lite_test_dataset(dims=OrderedDict([('y', 20), ('x', 20), ('time', 10)]))
    out = GaussianFilter(dims=('y', 'x'), sigma=1).apply(ds)
    np.testing.assert_array_equal(out.C11.values, ndi.gaussian_filter(ds.C11.values, (1, 1, 0)))
    out2 = gaussian(ds, dims=('y', 'x', 'time'), sigma=(1, 2, 0.5))
    np.testing.assert_array_equal(out2.C22.values, ndi.gaussian_filter(ds.C22.values, (1, 2, 0.5)))
    # njobs: halo int(4 sigma + 0.5) per chunk
    a = GaussianFilter(dims=('y', 'x'), sigma=1).apply(ds, njobs=2)
    for v in ds.data_vars:
        np.testing.assert_allclose(a[v].values, out[v].values, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('npdt', [np.float32, np.float64])
@pytest.mark.parametrize('mode', ['reflect', 'nearest', 'mirror', 'wrap'])
def test_fused_y_then_x_kernel(device, mode, npdt):
    """GaussianFilter(dims=('y', 'x')) on x-contiguous float32 / float64 planes runs both passes in one
    kernel (nd_amd_correlate1d_yx); every radius it is instantiated for, strip borders (248 / 240
    written columns per wave), planes shorter than the kernel, unaligned pitches, non-finite
    values -- bit-equal to scipy, whose intermediate array is in the array dtype too."""
    import scipy.ndimage as ndi
    import torch
    from nd_amd import kernels
    rng = np.random.default_rng(41)
    tdt = torch.float32 if npdt == np.float32 else torch.float64
    for shape in [(2, 70, 248), (1, 40, 249), (3, 5, 500), (1, 3, 9), (2, 140, 8), (1, 33, 1003), (2, 9, 241)]:
        a = rng.normal(size=shape).astype(npdt)
        for sigma in (0.3, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0):         # radii 1, 2, 3, 4, 5, 6, 8
            np.testing.assert_array_equal(_gpu_gauss(a, (0, sigma, sigma), device, mode=mode),
                                          ndi.gaussian_filter(a, (0, sigma, sigma), mode=mode))
    a = rng.normal(size=(2, 60, 300)).astype(npdt)
    # different sigmas with one radius (fused), with different radii (two passes), truncate
    for sigma, tr in (((0, 1.0, 1.1), 4.0), ((0, 1.0, 2.0), 4.0), ((0, 1.6, 1.6), 2.0)):
        np.testing.assert_array_equal(_gpu_gauss(a, sigma, device, mode=mode, truncate=tr),
                                      ndi.gaussian_filter(a, sigma, mode=mode, truncate=tr))
    b = a.copy()
    b[0, 10, 20] = np.inf
    b[1, 30, 200] = np.nan
    b[1, 5, 5] = -np.inf
    with np.errstate(all='ignore'):
        want = ndi.gaussian_filter(b, (0, 1, 1), mode=mode)
    got = _gpu_gauss(b, (0, 1, 1), device, mode=mode)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    # views with odd pitches in and out
    base = torch.from_numpy(rng.normal(size=(2, 50, 263)).astype(npdt)).to(device)
    view = base[:, 3:47, 1:260]
    obuf = torch.empty((2, 44, 261), dtype=tdt, device=device)
    out = obuf[:, :, :259]
    kernels.gaussian_filter(view, (0, 1, 1), out=out, mode=mode)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(),
                                  ndi.gaussian_filter(view.cpu().numpy(), (0, 1, 1), mode=mode))


@pytest.mark.parametrize('npdt', [np.float32, np.float64])
def test_fused_kernel_vector_and_scalar_accesses(device, npdt):
    """Both sides of the fused y-then-x kernel's choices of access (correlate1d_yx_kernel through memops.hpp) at
    sigma = 1, on the smallest planes that take each: 2 x 9 x 256 -- aligned rows wider than a wave's strip: 16-byte
    loads and stores (two per lane in float64) in the inner waves, mapped single loads at the row's ends; the same
    tensor without its first column -- the base one element off: single loads and stores throughout (8-byte ones in
    float64); 2 x 9 x 67 -- a ragged strip with a scalar store tail.  Bit-equal to scipy."""
    import scipy.ndimage as ndi
    import torch
    from nd_amd import kernels
    rng = np.random.default_rng(72)
    whole = torch.from_numpy(rng.normal(size=(2, 9, 256)).astype(npdt)).to(device)
    ragged = torch.from_numpy(rng.normal(size=(2, 9, 67)).astype(npdt)).to(device)
    for t in (whole, whole[..., 1:], ragged):
        got = kernels.gaussian_filter(t, (0, 1, 1))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), ndi.gaussian_filter(t.cpu().numpy(), (0, 1, 1)))
