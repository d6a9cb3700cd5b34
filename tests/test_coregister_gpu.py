"""Coregistration on the GPU against scikit-image 0.18's recorded output (tests/golden/coreg_skimage.npz)
and the numpy restatement (tests/coreg_ref.py)."""
import os
import time

import numpy as np
import pytest

from tests import coreg_ref, synth
from tests.test_coregister_cpu import CASES, GOLDEN, load_case

pytestmark = pytest.mark.gpu
_T0 = []


@pytest.fixture(scope='module')
def golden():
    _T0.append(time.time())
    return np.load(GOLDEN)


def _lite(planes, dims=('time', 'y', 'x'), to=None):
    from nd_amd import xr_lite
    ds = xr_lite.Dataset()
    for n, a in planes.items():
        a = a if dims[0] == 'time' else np.ascontiguousarray(np.moveaxis(a, 0, -1))
        ds[n] = (dims, a if to is None else to(a))
    return ds


def _planar(v, dims):
    v = v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)
    return v if dims[0] == 'time' else np.moveaxis(v, -1, 0)


def _check_shifts(got, want, u):
    """Equal, except that a near-tie may move one date by one 1/u step."""
    got, want = np.asarray(got), np.asarray(want)
    off = np.abs(got - want).max(axis=1)
    assert (off <= 1.0 / u + 1e-9).all(), (got, want)
    assert (off > 1e-12).sum() <= 1, (got, want)
    return off


def _check_out(got, want, dtype):
    if dtype == np.float64:
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13 * np.nanmax(np.abs(want)), equal_nan=True)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * np.nanmax(np.abs(want)), equal_nan=True)


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('dims', [('time', 'y', 'x'), ('y', 'x', 'time')])
@pytest.mark.parametrize('where', ['host', 'device'])
def test_apply_matches_skimage(golden, device, name, dims, where):
    import torch
    from nd_amd.warp import Coregistration
    u, ref, ins, outs, want = load_case(golden, name)
    to = None if where == 'host' else (lambda a: torch.from_numpy(a).to(device))
    ds = _lite(ins, dims, to)
    before = {n: _planar(ds[n].values, dims).copy() for n in ins}
    res = Coregistration(reference=ref - len(want) if name == 'f32_u1' else ref, upsampling=u).apply(ds)
    from nd_amd import kernels
    shifts, status = kernels.coregister_shifts(torch.from_numpy(ins['C11']).to(device), ref, u)
    off = _check_shifts(shifts.cpu().numpy(), want, u)
    assert int(status.sum()) == 0
    for n in ins:
        v = res[n].values
        assert (where == 'device') == torch.is_tensor(v)
        got = _planar(v, dims)
        np.testing.assert_array_equal(got[ref], ins[n][ref])          # reference date untouched
        np.testing.assert_array_equal(_planar(ds[n].values, dims), before[n])   # input untouched
        for t in range(len(want)):
            if off[t] < 1e-12:
                _check_out(got[t], outs[n][t], ins[n].dtype)
    if name == 'f32_u10':                                               # the NaN-plane quirk
        plane = _planar(res['C22'].values, dims)[3]
        np.testing.assert_array_equal(np.isnan(plane), np.isnan(outs['C22'][3]))


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('layout', ['planar', 'pixel_major'])
def test_warp_alone(golden, device, name, layout):
    import torch
    from nd_amd import kernels
    u, ref, ins, outs, want = load_case(golden, name)
    sh = torch.from_numpy(want).to(device)
    names = sorted(ins)
    tens = [torch.from_numpy(ins[n] if layout == 'planar' else np.ascontiguousarray(np.moveaxis(ins[n], 0, -1))
                             ).to(device) for n in names]
    res = kernels.warp_translate(tens, sh, ref, layout)
    for n, r in zip(names, res):
        got = r.cpu().numpy()
        got = got if layout == 'planar' else np.moveaxis(got, -1, 0)
        _check_out(got, outs[n], ins[n].dtype)
        # against the restatement: bit-equal in float64, a few ulp in float32
        want_r = coreg_ref.warp_stack(ins[n], want, ref)
        if ins[n].dtype == np.float64:
            np.testing.assert_array_equal(got, want_r)


def test_nan_in_c11_raises(golden, device):
    from nd_amd.warp import Coregistration
    u, ref, ins, outs, want = load_case(golden, 'f32_u10')
    bad = {n: a.copy() for n, a in ins.items()}
    bad['C11'][1, 5, 7] = np.nan
    with pytest.raises(ValueError, match='NaN values found'):
        Coregistration(reference=ref, upsampling=u).apply(_lite(bad))
    bad = {n: a.copy() for n, a in ins.items()}
    bad['C11'][ref, 0, 0] = np.nan
    with pytest.raises(ValueError, match='NaN values found'):
        Coregistration(reference=ref, upsampling=1).apply(_lite(bad))


def test_reference_test_restated(device):
    """nd/tests/test_coregister.py with no skimage: the misaligned set is rebuilt with coreg_ref's
    warp (bit-equal to skimage in float64); after Coregistration(upsampling=50) the residual shifts,
    measured with coreg_ref's phase correlation (u = 30, as the reference test measures), are small."""
    import scipy.ndimage as ndi
    from nd_amd.warp import Coregistration
    from collections import OrderedDict
    np.random.seed(0)
    data = synth.reference_test_dataset(OrderedDict([('y', 200), ('x', 200), ('time', 50)]), 0, 1)
    introduced = np.random.rand(50, 2)
    introduced[0, :] = 0
    planes = {}
    for n, a in data.items():
        d0 = ndi.gaussian_filter(a[:, :, 0], 3)
        a = a / a.max() + (d0 / d0.max())[:, :, None]
        p = np.ascontiguousarray(np.moveaxis(a, -1, 0))
        for t in range(1, 50):
            p[t] = coreg_ref.warp_plane(p[t], introduced[t, 1], introduced[t, 0])
        planes[n] = p
    res = Coregistration(upsampling=50).apply(_lite(planes))
    c11 = res['C11'].values
    shifts = np.array([coreg_ref.phase_shift(c11[t], c11[0], 30) for t in range(1, 50)])
    old = introduced[1:]
    assert (np.abs(shifts) <= 0.2).all()
    assert np.logical_or(np.abs(shifts) <= np.abs(old), np.abs(shifts) <= 0.1).all()


def test_reference_setup_against_skimage(golden, device):
    """skimage's recorded shifts and output sample for the reference's own set-up, from the GPU."""
    import torch
    from nd_amd import kernels
    idx = golden['ref50/sample_tyx'].astype(np.int64)
    names = ('C11', 'C12__im', 'C12__re', 'C22')
    np.random.seed(0)
    from collections import OrderedDict
    import scipy.ndimage as ndi
    data = synth.reference_test_dataset(OrderedDict([('y', 200), ('x', 200), ('time', 50)]), 0, 1)
    introduced = np.random.rand(50, 2)
    introduced[0, :] = 0
    np.testing.assert_array_equal(introduced, golden['ref50/introduced'])
    tens = []
    for n in names:
        a = data[n]
        d0 = ndi.gaussian_filter(a[:, :, 0], 3)
        a = a / a.max() + (d0 / d0.max())[:, :, None]
        p = np.ascontiguousarray(np.moveaxis(a, -1, 0))
        for t in range(1, 50):
            p[t] = coreg_ref.warp_plane(p[t], introduced[t, 1], introduced[t, 0])
        tens.append(torch.from_numpy(p).to(device))
    sh, status = kernels.coregister_shifts(tens[0], 0, 50)
    off = _check_shifts(sh.cpu().numpy(), golden['ref50/shifts'], 50)
    res = kernels.warp_translate(tens, sh, 0)
    for n, r in zip(names, res):
        got = r.cpu().numpy()[idx[:, 0], idx[:, 1], idx[:, 2]]
        keep = off[idx[:, 0]] < 1e-12
        np.testing.assert_allclose(got[keep], golden['ref50/sample/' + n][keep], rtol=1e-13, atol=1e-13)


def test_config_sized_run(device):
    """24 x 4096 x 4096 float32, 4 variables, device-resident, against coreg_ref on sampled dates and
    pixels (shift of 3 dates, warp of 2000 pixels of each variable on those dates)."""
    import torch
    from nd_amd.warp import Coregistration
    from nd_amd import xr_lite
    k, n = 24, 4096
    g = torch.Generator(device=device).manual_seed(5)
    base = torch.rand((n // 64, n // 64), device=device, generator=g)
    base = torch.nn.functional.interpolate(base[None, None], size=(n, n), mode='bilinear')[0, 0]
    ds = xr_lite.Dataset()
    rng = np.random.default_rng(5)
    moves = rng.integers(-6, 7, size=(k, 2))
    for v in ('C11', 'C12__re', 'C12__im', 'C22'):
        noise = torch.rand((k, n, n), device=device, generator=g) * 0.05
        st = torch.stack([torch.roll(base, (int(moves[t, 0]), int(moves[t, 1])), (0, 1)) for t in range(k)])
        ds[v] = (('time', 'y', 'x'), (st + noise + (1.0 if v in ('C11', 'C22') else -0.5)).contiguous())
        del st, noise
    res = Coregistration(reference=0, upsampling=10).apply(ds)
    torch.cuda.synchronize()
    c11 = ds['C11'].values
    from nd_amd import kernels
    sh = kernels.coregister_shifts(c11, 0, 10)[0].cpu().numpy()
    for t in (5, 17):
        np.testing.assert_allclose(sh[t], moves[t] - moves[0], atol=0.11)
    prs = np.random.default_rng(1)
    rows, cols = prs.integers(0, n, 40), prs.integers(0, n, 50)
    for t in (5, 17):
        for v in ('C11', 'C12__im'):
            plane = ds[v].values[t].cpu().numpy()
            want = coreg_ref.warp_pixels(plane, sh[t, 0], sh[t, 1], rows, cols)
            got = res[v].values[t].cpu().numpy()[rows][:, cols]
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * np.abs(plane).max())


def test_budget():
    """the GPU tests of this file stay within 60 s (measured from the first golden load)."""
    if _T0:
        assert time.time() - _T0[0] < 60
