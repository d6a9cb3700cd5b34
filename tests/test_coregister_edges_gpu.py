"""Coregistration on the GPU at the shapes the recorded scikit-image cases leave out: odd and prime
rasters, every width of the upsampled region, the seams of the warp tiles, degenerate axes.  Every
reference comes from the numpy restatement (tests/coreg_ref.py); which shifts must be reproduced
exactly is decided by the near-tie rule of tests/coreg_cases.py."""
import functools

import numpy as np
import pytest

from tests import coreg_cases as cases
from tests import coreg_ref

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHIFT_RUNS = [(c, F32) for c in cases.CASES] + [(c, F64) for c in cases.F64_CASES]
ODD = (31, 37, 7)


def _run_id(run):
    return '%s_%s' % (cases.case_id(run[0]), np.dtype(run[1]).name)


def _dev(a, device):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to(device)


def _shifts(c11, device, reference, u, dims=('time', 'y', 'x')):
    from nd_amd import kernels
    t = c11 if hasattr(c11, 'is_cuda') else _dev(c11, device)
    sh, status = kernels.coregister_shifts(t, reference, u, dims=dims)
    return sh.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------ shifts
@pytest.mark.parametrize('run', SHIFT_RUNS, ids=_run_id)
def test_shifts_of_the_case_table(device, run):
    (ny, nx, u), dtype = run
    want, ok = cases.case_reference(ny, nx, u, dtype)
    got, status = _shifts(cases.c11_stack(ny, nx, u, dtype), device, 0, u)
    print('%s: decided %s\n got  %s\n want %s' % (_run_id(run), ok.astype(int), got.tolist(), want.tolist()))
    assert (status == 0).all()
    assert (got[0] == 0).all()
    cases.check_shifts(got, want, ok, u, (ny, nx))


@pytest.mark.parametrize('case', cases.FOURIER_CASES, ids=cases.case_id)
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_fourier_shifts(device, case, dtype):
    """Band-limited images moved with a phase ramp by multiples of 1 / u: float64 returns exactly the
    shift applied; float32 (the inputs rounded) follows the rule."""
    ny, nx, u = case
    a, applied = cases.fourier_stack(ny, nx, u)
    got, status = _shifts(a.astype(dtype), device, 0, u)
    print('%s %s\n got     %s\n applied %s' % (cases.case_id(case), np.dtype(dtype).name, got.tolist(), applied.tolist()))
    assert (status == 0).all()
    if dtype == F64:
        np.testing.assert_allclose(got, applied, rtol=0, atol=1e-12)
    want, ok = cases.fourier_reference(ny, nx, u, dtype)
    cases.check_shifts(got, want, ok, u, (ny, nx))


def test_input_paths_agree(device):
    """The three ways a C11 stack reaches the staging buffer give the same shifts bit for bit:
    contiguous planar (copy), (y, x, time) (relayout), a planar view with a row pitch (gather)."""
    import torch
    ny, nx, u = ODD
    a = cases.c11_stack(ny, nx, u, F32)
    want, ok = cases.case_reference(ny, nx, u, F32)
    planar, _ = _shifts(a, device, 0, u)
    pm, st_pm = _shifts(np.moveaxis(a, 0, -1), device, 0, u, dims=('y', 'x', 'time'))
    wide = torch.full((cases.K, ny + 2, nx + 5), float('nan'), dtype=torch.float32, device=device)
    view = wide[:, 1:ny + 1, 3:nx + 3]
    view.copy_(_dev(a, device))
    assert not view.is_contiguous() and view.stride(1) == nx + 5
    pitched, st_pitched = _shifts(view, device, 0, u)
    cases.check_shifts(planar, want, ok, u, (ny, nx))
    np.testing.assert_array_equal(pm, planar)
    np.testing.assert_array_equal(pitched, planar)
    assert (st_pm == 0).all() and (st_pitched == 0).all()


def test_reference_last_and_short_series(device):
    ny, nx, u = ODD
    a = cases.c11_stack(ny, nx, u, F32)
    last = cases.K - 1
    want, ok = cases.decided_stack(a, last, u)
    got, status = _shifts(a, device, last, u)
    assert (status == 0).all() and (got[last] == 0).all()
    cases.check_shifts(got, want, ok, u, (ny, nx))
    # one date: nothing to align
    got, status = _shifts(a[:1], device, 0, u)
    assert got.shape == (1, 2) and (got == 0).all() and (status == 0).all()
    # two dates, either as the reference
    for ref in (0, 1):
        want, ok = cases.decided_stack(a[:2], ref, u)
        got, status = _shifts(a[:2], device, ref, u)
        assert (status == 0).all() and (got[ref] == 0).all()
        cases.check_shifts(got, want, ok, u, (ny, nx))


def test_nan_marks_its_date_only(device):
    ny, nx, u = ODD
    a = cases.c11_stack(ny, nx, u, F32)
    clean, _ = _shifts(a, device, 0, u)
    bad = a.copy()
    bad[3, ny - 1, nx - 1] = np.nan
    got, status = _shifts(bad, device, 0, u)
    assert status.tolist() == [0, 0, 0, 1, 0, 0]
    keep = [0, 1, 2, 4, 5]
    np.testing.assert_array_equal(got[keep], clean[keep])
    with pytest.raises(ValueError, match='NaN values found'):
        coreg_ref.phase_shift(bad[3], bad[0], u)


# ------------------------------------------------------------------ warp
def _check_out(got, want, src, what):
    """float64 bit-equal; float32 within 1e-6 max|in|; NaN at the same places."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    if src.dtype == F64:
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * np.nanmax(np.abs(src)), equal_nan=True,
                                   err_msg=what)


@functools.lru_cache(maxsize=None)
def _warp_reference(nr, nc, dtype):
    planes = cases.warp_planes(nr, nc, dtype)
    sh = cases.warp_shifts(nr, nc)
    return planes, sh, {n: coreg_ref.warp_stack(a, sh, cases.WARP_REF) for n, a in planes.items()}


def _warp(planes, sh, reference, layout, device):
    from nd_amd import kernels
    names = sorted(planes)
    tens = [_dev(planes[n] if layout == 'planar' else np.moveaxis(planes[n], 0, -1), device) for n in names]
    res = kernels.warp_translate(tens, _dev(sh, device), reference, layout)
    out = {}
    for n, t, r in zip(names, tens, res):
        got = r.cpu().numpy()
        out[n] = got if layout == 'planar' else np.moveaxis(got, -1, 0)
        kept = t.cpu().numpy()
        np.testing.assert_array_equal(kept if layout == 'planar' else np.moveaxis(kept, -1, 0), planes[n])
    return out


WARP_RUNS = [(s, 'planar') for s in cases.WARP_SHAPES] + [(s, 'pixel_major') for s in cases.WARP_PM_SHAPES]


@pytest.mark.parametrize('run', WARP_RUNS, ids=lambda r: '%dx%d_%s' % (r[0] + (r[1],)))
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_warp_table_of_shifts(device, run, dtype):
    (nr, nc), layout = run
    planes, sh, want = _warp_reference(nr, nc, dtype)
    got = _warp(planes, sh, cases.WARP_REF, layout, device)
    for n in planes:
        np.testing.assert_array_equal(got[n][cases.WARP_REF], planes[n][cases.WARP_REF])    # copied bit for bit
        for t in range(len(sh)):
            _check_out(got[n][t], want[n][t], planes[n], '%s date %d shift %s' % (n, t, sh[t]))
    assert (got['pos'][7] == 0).all() and (got['pos'][8] == 0).all()       # the whole plane outside


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_warp_minmax_partition(device, dtype):
    """129 x 130, one variable, three dates: two partial blocks per plane, the extremes at the ends
    of the plane and on both sides of element 8192.  A lost partial shows where the clip bites."""
    a, sh = cases.minmax_planes(dtype), cases.MINMAX_SHIFTS
    want = coreg_ref.warp_stack(a, sh, -1)
    got = _warp({'v': a}, sh, -1, 'planar', device)['v']
    for t in range(3):
        _check_out(got[t], want[t], a, 'date %d' % t)


def test_warp_pixel_major_257_dates(device):
    """3 x 5 pixels, 257 dates, pixel-major: the second date group of the min / max kernel."""
    k, nr, nc = 257, 3, 5
    rng = np.random.RandomState(257)
    a = (np.round((0.5 + rng.uniform(0, 2, (k, nr, nc))) * 256) / 256).astype(F32)
    a[256] = a[256] * 4 - 5                         # the last date has a range of its own, 0 inside it
    sh = rng.randint(-12, 13, (k, 2)) / 8.0
    sh[256] = (0.375, -0.625)
    want = coreg_ref.warp_stack(a, sh, 255)
    got = _warp({'v': a}, sh, 255, 'pixel_major', device)['v']
    np.testing.assert_array_equal(got[255], a[255])
    _check_out(got[256], want[256], a, 'date 256')
    _check_out(got, want, a, 'all dates')


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize('dims', [('time', 'y', 'x'), ('y', 'x', 'time')], ids=['tyx', 'yxt'])
def test_apply_on_an_odd_raster(device, dims):
    import torch
    from nd_amd import xr_lite
    from nd_amd.warp import Coregistration
    ny, nx, u = 17, 65, 16
    planes = cases.stack(cases.case_seed(ny, nx, u), cases.K, ny, nx, F32, nvars=4)
    np.testing.assert_array_equal(planes['C11'], cases.c11_stack(ny, nx, u, F32))
    want_sh, ok = cases.case_reference(ny, nx, u, F32)
    want = {n: coreg_ref.warp_stack(a, want_sh, 0) for n, a in planes.items()}
    ds = xr_lite.Dataset()
    for n, a in planes.items():
        ds[n] = (dims, _dev(a if dims[0] == 'time' else np.moveaxis(a, 0, -1), device))
    res = Coregistration(reference=0, upsampling=u).apply(ds)
    got_sh, status = _shifts(ds['C11'].values, device, 0, u, dims=dims)
    assert (status == 0).all()
    same = cases.check_shifts(got_sh, want_sh, ok, u, (ny, nx))
    for n, a in planes.items():
        v = res[n].values
        assert torch.is_tensor(v) and tuple(res[n].dims) == dims
        got = v.cpu().numpy()
        got = got if dims[0] == 'time' else np.moveaxis(got, -1, 0)
        np.testing.assert_array_equal(got[0], a[0])
        for t in np.flatnonzero(same):
            _check_out(got[t], want[n][t], a, '%s date %d' % (n, t))
