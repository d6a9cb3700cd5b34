"""to_rgb on the GPU: limits == the numpy restatement (tests/rgb_ref.py) and numpy 2.2.6's recorded values
(tests/golden/to_rgb_numpy.npz), composite bytes identical.  Exact equality throughout."""
import numpy as np
import pytest

from tests import rgb_cases, rgb_ref
from tests.test_to_rgb_cpu import GOLDEN, NAMES, golden_planes, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _limits(planes, device, pmin, pmax):
    """device limits of a list of equally shaped planes, one call: (plane, 2) numpy + counts"""
    from nd_amd import kernels
    t = _dev(np.stack(planes), device)
    lim, cnt = kernels.rgb_limits([t], pmin, pmax)
    return lim.cpu().numpy()[:, 0, :], cnt.cpu().numpy()[:, 0]


@pytest.mark.parametrize('dtype', rgb_cases.DTYPES)
@pytest.mark.parametrize('name', NAMES)
def test_limits_and_bytes_of_every_case(golden, device, dtype, name):
    from nd_amd import visualize
    a = golden_planes(golden, dtype)[name]
    rec = golden['%s/%s/pct' % (np.dtype(dtype).name, name)]
    ps = rgb_cases.PERCENTILES
    for j in range(0, len(ps), 2):
        pmin, pmax = ps[j], ps[min(j + 1, len(ps) - 1)]
        lim, cnt = _limits([a], device, pmin, pmax)
        assert lim.dtype == dtype and cnt[0] == np.count_nonzero(~np.isnan(a))
        assert same(lim[0, 0], rgb_ref.nanpercentile(a, pmin)), (name, pmin, lim)
        assert same(lim[0, 1], rgb_ref.nanpercentile(a, pmax)), (name, pmax, lim)
        assert same(lim[0, 0], rec[j]) and same(lim[0, 1], rec[min(j + 1, len(ps) - 1)])
    got = visualize.to_rgb(a)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == a.shape + (3,)
    np.testing.assert_array_equal(got, rgb_ref.composite([a]))
    np.testing.assert_array_equal(got, golden['%s/%s/grey' % (np.dtype(dtype).name, name)])
    dev = visualize.to_rgb(_dev(a, device))
    assert dev.is_cuda
    np.testing.assert_array_equal(dev.cpu().numpy(), got)                # numpy in == device in


@pytest.mark.parametrize('dtype', rgb_cases.DTYPES)
def test_three_channels_limits_given_mask(golden, device, dtype):
    from nd_amd import visualize
    p = golden_planes(golden, dtype)
    tri = [p['exponential'][:32, :32], p['scaled_1e6'], p['one_binade'][:32, :32]]
    np.testing.assert_array_equal(visualize.to_rgb(tri), golden['%s/rgb' % np.dtype(dtype).name])
    mask = np.random.default_rng(2).random(tri[0].shape) < 0.5
    for kw in (dict(), dict(vmin=0.25, vmax=2.5), dict(vmin=[0.1, 3e5, 1.2], vmax=[2, 4e6, 1.7]),
               dict(vmin=0.5), dict(vmax=[1.5, 2e6, 1.9]), dict(vmin=1, vmax=1), dict(vmin=5, vmax=2),
               dict(vmin=1e30), dict(pmin=98, pmax=2), dict(pmin=2.5, pmax=99.9), dict(mask=mask),
               dict(vmin=0.1, mask=mask)):
        np.testing.assert_array_equal(visualize.to_rgb(tri, **kw), rgb_ref.composite(tri, **kw), err_msg=str(kw))
        one = {k: (v[0] if isinstance(v, list) else v) for k, v in kw.items()}
        np.testing.assert_array_equal(visualize.to_rgb(tri[0], **one), rgb_ref.composite(tri[:1], **one),
                                      err_msg=str(kw))
    ints = [(a * 40).astype(np.uint8) for a in tri]
    np.testing.assert_array_equal(visualize.to_rgb(ints), rgb_ref.composite(ints))
    for kw in (dict(vmin=3.0, vmax=200.0), dict(vmin=2.5), dict(vmax=[90.0, 250.0, 60.5])):
        np.testing.assert_array_equal(visualize.to_rgb(ints, **kw), rgb_ref.composite(ints, **kw), err_msg=str(kw))
        np.testing.assert_array_equal(rgb_ref.composite(ints, **kw), rgb_ref.numpy_composite(ints, **kw))
    with pytest.raises(TypeError):
        visualize.to_rgb(tri[0].astype(np.float16))
    with pytest.raises(TypeError, match="astype\\('uint8'\\)"):
        visualize.to_rgb(tri[0] > 1)


@pytest.mark.parametrize('dtype', rgb_cases.DTYPES)
@pytest.mark.parametrize('nx', [1, 2, 3, 4, 5, 6, 7, 8, 9, 4093])
def test_store_tail_widths(device, dtype, nx):
    from nd_amd import visualize
    rng = np.random.default_rng(nx)
    for ny in (1, 3):
        tri = [rng.exponential(size=(ny, nx)).astype(dtype) for _ in range(3)]
        tri[1][rng.random((ny, nx)) < 0.2] = np.nan
        mask = rng.random((ny, nx)) < 0.7
        np.testing.assert_array_equal(visualize.to_rgb(tri), rgb_ref.composite(tri))
        np.testing.assert_array_equal(visualize.to_rgb(tri, mask=mask), rgb_ref.composite(tri, mask=mask))
        np.testing.assert_array_equal(visualize.to_rgb(tri[1]), rgb_ref.composite(tri[1:2]))


def _stack(dtype, k=5, ny=22, nx=35, seed=7, zeros=True):
    rng = np.random.default_rng(seed)
    c11 = rng.exponential(size=(k, ny, nx)).astype(dtype)
    c22 = rng.exponential(size=(k, ny, nx)).astype(dtype)
    if zeros:
        c22[rng.random(c22.shape) < 0.1] = 0                      # x / 0: an infinity, counted
        both = rng.random(c22.shape) < 0.1                        # 0 / 0: NaN, dropped
        c11[both] = 0
        c22[both] = 0
        for t in range(k):                                        # a different NaN count on every date
            c11[t].ravel()[:3 * t] = np.nan
    return c11, c22


def _dataset(c11, c22, dims, to=None):
    from nd_amd import xr_lite
    ds = xr_lite.Dataset()
    for n, a in (('C11', c11), ('C22', c22)):
        a = a if dims[0] == 'time' else np.ascontiguousarray(np.moveaxis(a, 0, -1))
        ds[n] = (dims, a if to is None else to(a))
    return ds


def _frames_ref(c11, c22, **kw):
    with np.errstate(all='ignore'):
        return np.stack([rgb_ref.composite([c11[t], c22[t], c11[t] / c22[t]], **kw) for t in range(len(c11))])


@pytest.mark.parametrize('dtype', rgb_cases.DTYPES)
def test_stack_quotient_layouts_and_per_plane_counts(device, dtype):
    from nd_amd import kernels, visualize
    c11, c22 = _stack(dtype)
    k = len(c11)
    with np.errstate(all='ignore'):
        quo = c11 / c22
    assert np.isinf(quo).any() and np.isnan(quo).any()
    want = _frames_ref(c11, c22)
    planar = _dataset(c11, c22, ('time', 'y', 'x'))
    got = visualize.to_rgb_stack(planar)
    assert isinstance(got, np.ndarray) and got.shape == c11.shape + (3,)
    np.testing.assert_array_equal(got, want)
    # (y, x, time): the same bytes
    np.testing.assert_array_equal(visualize.to_rgb_stack(_dataset(c11, c22, ('y', 'x', 'time'))), got)
    # device data in, device tensor out
    ondev = visualize.to_rgb_stack(_dataset(c11, c22, ('time', 'y', 'x'), to=lambda a: _dev(a, device)))
    assert ondev.is_cuda
    np.testing.assert_array_equal(ondev.cpu().numpy(), got)
    ondev = visualize.to_rgb_stack(_dataset(c11, c22, ('y', 'x', 'time'), to=lambda a: _dev(a, device)))
    np.testing.assert_array_equal(ondev.cpu().numpy(), got)
    # a loop of to_rgb over the dates
    loop = np.stack([visualize.to_rgb([c11[t], c22[t], quo[t]]) for t in range(k)])
    np.testing.assert_array_equal(got, loop)
    # limits and per-plane counts
    lim = visualize.stretch_limits(planar)
    assert lim.shape == (k, 3, 2) and lim.dtype == dtype
    for t in range(k):
        for c, ch in enumerate((c11[t], c22[t], quo[t])):
            assert same(lim[t, c, 0], rgb_ref.nanpercentile(ch, 2)), (t, c)
            assert same(lim[t, c, 1], rgb_ref.nanpercentile(ch, 98)), (t, c)
    d11, d22 = _dev(c11, device), _dev(c22, device)
    _, cnt = kernels.rgb_limits([d11, d22, (d11, d22)])
    want_cnt = np.array([[np.count_nonzero(~np.isnan(ch[t])) for ch in (c11, c22, quo)] for t in range(k)])
    np.testing.assert_array_equal(cnt.cpu().numpy(), want_cnt)
    assert len(set(want_cnt[:, 0])) == k
    # callable rgb, grey DataArray, mask, given limits
    mask = np.random.default_rng(1).random(c11.shape[1:]) < 0.6
    got = visualize.to_rgb_stack(planar, rgb=lambda d: [d['C22'], d['C11'], d['C22']], mask=mask, vmin=0.1)
    want = np.stack([rgb_ref.composite([c22[t], c11[t], c22[t]], mask=mask, vmin=0.1) for t in range(k)])
    np.testing.assert_array_equal(got, want)
    grey = visualize.to_rgb_stack(planar['C11'])
    np.testing.assert_array_equal(grey, np.stack([rgb_ref.composite([c11[t]]) for t in range(k)]))


def test_kernel_ids_are_recorded(device):
    from nd_amd import _lib, visualize
    c11, c22 = _stack(np.float32, zeros=False)
    ds = _dataset(c11, c22, ('time', 'y', 'x'))
    _lib.timing_enable(64)
    try:
        visualize.to_rgb_stack(ds)
        names = [n for n, _ in _lib.timing_collect()]
    finally:
        _lib.timing_enable(0)
    assert names == ['rgb_limits', 'rgb_compose']


def test_bundled_raster(device):
    """the reference's bundled single-date dual-pol raster (tests/golden/slc_c2): 73 % exact zeros, so
    C11 / C22 is NaN on the margin and the 2nd percentile sits in a run of ties"""
    import os
    from nd_amd import visualize
    g = np.load(os.path.join(os.path.dirname(GOLDEN), 'slc_c2', 'slc_c2.npz'))
    c11, c22 = g['C11'], g['C22']
    assert c11.ndim == 2 and (c11 == 0).mean() > 0.7
    with np.errstate(all='ignore'):
        chans = [c11, c22, c11 / c22]
    np.testing.assert_array_equal(visualize.to_rgb(chans), rgb_ref.composite(chans))
    ds = _dataset(c11[None], c22[None], ('time', 'y', 'x'))
    np.testing.assert_array_equal(visualize.to_rgb_stack(ds)[0], rgb_ref.composite(chans))


def test_beyond_2_24_values(device):
    """4100 x 4100 float32: the float32 virtual index is coarse; the device reproduces it"""
    a = np.random.default_rng(5).exponential(size=(4100, 4100)).astype(np.float32)
    a[::1000, ::5] = np.nan
    for pmin, pmax in ((2, 98), (99.9, 100)):
        lim, cnt = _limits([a], device, pmin, pmax)
        assert cnt[0] == np.count_nonzero(~np.isnan(a)) > 2 ** 24
        assert same(lim[0, 0], rgb_ref.nanpercentile(a, pmin)) and same(lim[0, 1], rgb_ref.nanpercentile(a, pmax))


def test_full_size(device):
    """24 x 4096 x 4096 float32 generated on the device: three (date, channel) planes and 64 sampled rows
    of their frames against the restatement; constant and one-binade dates among the 24"""
    import torch
    from nd_amd import _lib, xr_lite, visualize
    k, n = 24, 4096
    gen = torch.Generator(device=device)
    gen.manual_seed(11)
    c11 = torch.empty((k, n, n), dtype=torch.float32, device=device).exponential_(1.0, generator=gen)
    c22 = torch.empty((k, n, n), dtype=torch.float32, device=device).exponential_(2.0, generator=gen)
    c11[3] = 0.75                                                   # a constant plane
    c22[5] = 1 + torch.rand((n, n), device=device, generator=gen)   # one binade
    c22[7, ::9, ::4] = 0
    c11[7, ::18, ::8] = 0
    ds = xr_lite.Dataset()
    ds['C11'] = (('time', 'y', 'x'), c11)
    ds['C22'] = (('time', 'y', 'x'), c22)
    _lib.timing_enable(16)
    try:
        frames = visualize.to_rgb_stack(ds)
        lim = visualize.stretch_limits(ds)
        timed = _lib.timing_collect()
    finally:
        _lib.timing_enable(0)
    assert [nm for nm, _ in timed] == ['rgb_limits', 'rgb_compose', 'rgb_limits']
    print('full size: %s' % ', '.join('%s %.3f ms' % t for t in timed))
    assert frames.shape == (k, n, n, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    lim = lim.cpu().numpy()
    rows = np.random.default_rng(3).choice(n, 64, replace=False)
    rows.sort()
    for t, c in ((3, 0), (5, 1), (7, 2), (23, 2), (0, 0)):
        a, b = c11[t].cpu().numpy(), c22[t].cpu().numpy()
        with np.errstate(all='ignore'):
            ch = (a, b, a / b)[c]
        lo, hi = rgb_ref.limits(ch)
        assert same(lim[t, c, 0], lo) and same(lim[t, c, 1], hi), (t, c, lim[t, c], lo, hi)
        want = rgb_ref.composite([ch[rows]], lims=[(lo, hi)])[:, :, 0]
        np.testing.assert_array_equal(frames[t, :, :, c].cpu().numpy()[rows], want)
