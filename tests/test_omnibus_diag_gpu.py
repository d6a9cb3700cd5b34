"""The intensity-only omnibus test (pol='diag') on the GPU against tests/golden/omnibus_diag.npz, which is
recorded from the numpy restatement tests/omnibus_diag_ref.py (there is no reference implementation: the
restatement is pinned to the oracle for the 2 x 2 structure in tests/test_omnibus_diag_cpu.py).

The comparison rule (tests/omnibus_diag_cases.py: compare): maps equal at every pixel; z / P within 1e-5
relative (float64: 1e-10) with equal NaN positions; a differing map pixel is tolerated only where the
restatement's deciding test has |P - alpha| <= 2 ulp(T), for at most 1 pixel in 10^5 -- and the file is
recorded with seeds for which no decision comes within 16 ulp, so the expected count is 0."""
import numpy as np
import pytest

from tests import omnibus_diag_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return C.Golden()


def _run(planes, alpha, n, device, layout='tyx'):
    import torch
    from nd_amd import kernels
    ts = [torch.from_numpy(p).to(device) for p in planes]
    dims = ('time', 'y', 'x')
    if layout == 'yxt':
        ts = [t.permute(1, 2, 0).contiguous() for t in ts]
        dims = ('y', 'x', 'time')
    ch, z, P = kernels.change_detection_diag(ts, alpha=alpha, n=n, dims=dims, stats=True)
    ch2 = kernels.change_detection_diag(ts, alpha=alpha, n=n, dims=dims)
    torch.cuda.synchronize()
    assert torch.equal(ch, ch2)
    return ch.cpu().numpy(), z.cpu().numpy(), P.cpu().numpy()


def _check_case(golden, name, device, layout='tyx'):
    case = golden.case(name)
    planes = C.make_input(case)
    changes = 0
    for alpha in case['alphas']:
        want, z0, P0, closest = golden.expected(name, alpha)
        ch, z, P = _run(planes, alpha, case['n'], device, layout=layout)
        C.compare(ch, z, P, want, z0, P0, closest, alpha, case['dtype'])
        changes += int(want.sum())
    return changes


@pytest.mark.parametrize('shape', C.CORE_SHAPES, ids=lambda s: 'k%d_%dx%d' % s)
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('q', [1, 2, 3])
def test_core_grid(golden, device, q, dtype, shape):
    """q x dtype x shape x alpha {0.01, 0.5, 0.9, 0.99} x n {1, 4.4, 9}: widths off the wave and 16-byte grids, a
    row shorter than a wave, rows that straddle block edges, a single date."""
    k, ny, nx = shape
    changes = 0
    for n in C.CORE_LOOKS:
        changes += _check_case(golden, 'core_q%d_%s_k%d_%dx%d_n%g' % (q, dtype, k, ny, nx, n), device)
    assert (changes > 0) == (k >= 2)


def _launched(planes, alpha, n, device):
    """names of the kernels one call launches, from the library's own timing records"""
    import torch
    from nd_amd import _lib, kernels
    ts = [torch.from_numpy(p).to(device) for p in planes]
    _lib.timing_enable(16)
    try:
        kernels.change_detection_diag(ts, alpha=alpha, n=n)
        return {name for name, _ in _lib.timing_collect()}
    finally:
        _lib.timing_enable(0)


@pytest.mark.parametrize('qd', sorted(C.FUSED_MAX_K), ids=lambda qd: 'q%d_%s' % qd)
def test_form_limits(golden, device, qd):
    """Both sides of the one-launch form's limit on k q sizeof(T) at thresholds on both sides of its limit on
    alpha (0.75): the longest series the form serves and the first one that goes through pass A + pass B.  Which
    form served a call is read from the library's timing records, so the cases follow the code's limits."""
    q, dtype = qd
    kmax = C.FUSED_MAX_K[qd]
    for k in (kmax, kmax + 1):
        name = 'limit_q%d_%s_k%d' % (q, dtype, k)
        assert _check_case(golden, name, device) > 0
        planes = C.make_input(golden.case(name))
        for alpha in (0.7, 0.8):
            fused = k == kmax and alpha < 0.75
            assert _launched(planes, alpha, 4.4, device) == \
                ({'omnibus_c2_fused'} if fused else {'omnibus_c2_global', 'omnibus_c2_search'}), (k, alpha)


@pytest.mark.parametrize('name', ['long_q%d_float32_k%d' % (q, k) for q in (2, 3) for k in (33, 97, 200)]
                         + ['long_q2_float64_k97', 'long_q3_float64_k97'])
def test_long_series(golden, device, name):
    """k = 33, 97 (past the table that travels as a kernel argument) and 200 at 4 x 130."""
    assert _check_case(golden, name, device) > 0


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('q', [1, 2])
def test_step_change(golden, device, q, dtype):
    """nd/tests/test_change_omnibus.py for intensities: every pixel has exactly one change, at date 5."""
    name = 'step_q%d_%s' % (q, dtype)
    want = golden.expected(name, 0.9)[0]
    assert (want.sum(axis=-1) == 1).all() and (want[..., 5] == 1).all()
    _check_case(golden, name, device)


@pytest.mark.parametrize('name', ['degenerate_q2_float32', 'degenerate_q3_float64', 'degenerate_q1_float32'])
def test_degenerate_values(golden, device, name):
    """NaN, 0, negative and inf in 5 % of the samples: NaN or infinite statistics, hence no change."""
    _check_case(golden, name, device)


def test_arbitrary_strides(golden, device):
    """A (y, x, time) tensor passed with dims=('y', 'x', 'time') and a sliced view with a row pitch equal the
    contiguous result."""
    import torch
    from nd_amd import kernels
    for name in ('core_q2_float32_k10_5x130_n4.4', 'core_q3_float64_k25_4x257_n9'):
        _check_case(golden, name, device, layout='yxt')
        case = golden.case(name)
        planes = C.make_input(case)
        k, ny, nx = planes[0].shape
        for alpha in (0.01, 0.9):
            want = golden.expected(name, alpha)[0]
            wide = [torch.zeros((k, ny + 2, nx + 7), dtype=torch.from_numpy(p).dtype, device=device) for p in planes]
            views = []
            for w, p in zip(wide, planes):
                w[:, 1:1 + ny, 3:3 + nx] = torch.from_numpy(p).to(device)
                views.append(w[:, 1:1 + ny, 3:3 + nx])
            got = kernels.change_detection_diag(views, alpha=alpha, n=case['n'])
            np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('alpha', [0.01, 0.99])
@pytest.mark.parametrize('shape', [(6, 1, 1), (6, 1, 3), (8, 5, 7)], ids=lambda s: 'k%d_%dx%d' % s)
def test_smallest_rasters_flat_and_cropped(device, shape, alpha):
    """1 x 1 and 1 x 3 pixels: the blocks per shard of pass B sit on their lower bound of one; 5 x 7 pixels; each
    contiguous (one flat row) and as a crop of a wider buffer (row by row).  alpha = 0.01: the one-launch form;
    0.99: pass A and pass B.  Against the restatement computed here, by the file's rule (C.compare)."""
    import torch
    from nd_amd import kernels
    from tests import omnibus_diag_ref as R
    k, ny, nx = shape
    planes = C.gamma_stack(40 + nx, 2, k, ny, nx, 4.4, 'float32')
    S = R.Series(planes, (1, 1), 4.4)
    want, z0, P0 = R.change_detection(planes, (1, 1), alpha, 4.4, series=S)
    ch, z, P = _run(planes, alpha, 4.4, device)
    C.compare(ch, z, P, want, z0, P0, S.closest, alpha, 'float32')
    views = []
    for p in planes:
        wide = torch.zeros((k, ny + 4, nx + 9), dtype=torch.float32, device=device)
        wide[:, 2:2 + ny, 3:3 + nx] = torch.from_numpy(p).to(device)
        views.append(wide[:, 2:2 + ny, 3:3 + nx])
    assert views[0].stride(1) != nx
    ch, z, P = kernels.change_detection_diag(views, alpha=alpha, n=4.4, stats=True)
    C.compare(ch.cpu().numpy(), z.cpu().numpy(), P.cpu().numpy(), want, z0, P0, S.closest, alpha, 'float32')
    assert torch.equal(kernels.change_detection_diag(views, alpha=alpha, n=4.4), ch)


def test_public_interface(golden, device):
    """OmnibusTest(pol='diag') on xr_lite datasets: host and device data, both layouts, named channels and the
    C11 / C22 default with a C12 present and ignored; omnibus_statistics; omnibus()."""
    import torch
    from nd_amd import xr_lite
    from nd_amd.change import OmnibusTest, omnibus, omnibus_statistics
    name, alpha = 'core_q2_float32_k10_5x130_n4.4', 0.9
    case = golden.case(name)
    planes = C.make_input(case)
    want, z0, P0, closest = golden.expected(name, alpha)
    k, ny, nx = planes[0].shape
    coords = {'y': np.linspace(60.0, 50.0, ny), 'x': np.linspace(-10.0, 0.0, nx), 'time': np.arange(k)}
    c12 = (np.ones((k, ny, nx)) + 1j).astype(np.complex64)
    for names, kw in ((('VV', 'VH'), dict(channels=['VV', 'VH'])), (('C11', 'C22'), {})):
        for on_device in (False, True):
            for dims in (('y', 'x', 'time'), ('time', 'y', 'x')):
                ds = xr_lite.Dataset(coords=coords, attrs={'attr1': 1})
                for v, p in zip(names + ('C12',), list(planes) + [c12]):
                    a = np.ascontiguousarray(np.moveaxis(p, 0, -1)) if dims[0] == 'y' else p
                    ds[v] = (dims, torch.from_numpy(a).to(device) if on_device else a)
                got = OmnibusTest(n=case['n'], alpha=alpha, pol='diag', **kw).apply(ds)
                assert got.dims == ('y', 'x', 'time') and got.name == 'change' and got.attrs == ds.attrs
                assert set(got.coords) == set(ds.coords)
                vals = got.values.cpu().numpy() if on_device else got.values
                assert vals.dtype == np.bool_ and isinstance(got.values, torch.Tensor) == on_device
                np.testing.assert_array_equal(vals, want.astype(bool))
                host = (lambda a: a.cpu().numpy()) if on_device else (lambda a: a)
                ch, z, P = omnibus_statistics(ds, n=case['n'], alpha=alpha, pol='diag', channels=kw.get('channels'))
                assert tuple(z.dims) == ('y', 'x') and tuple(P.dims) == ('y', 'x')
                C.compare(host(ch.values).astype(np.uint8), host(z.values), host(P.values), want, z0, P0, closest,
                          alpha, 'float32')
                np.testing.assert_array_equal(host(omnibus(ds, n=case['n'], alpha=alpha, pol='diag', **kw).values),
                                              want.astype(bool))
    with pytest.raises(ValueError, match="'dual'.*'full'.*'diag'"):
        OmnibusTest(pol='quad').apply(ds)


def test_multilook_is_boxcar_then_test(device):
    """ml=3 equals BoxcarFilter(w=3) followed by the test with n = 9, on 6 x 20 x 70."""
    from nd_amd import xr_lite
    from nd_amd.change import OmnibusTest
    from nd_amd.filters import BoxcarFilter
    planes = C.gamma_stack(5, 2, 6, 20, 70, 1, 'float32')
    import torch
    ds, ds_dev = xr_lite.Dataset(), xr_lite.Dataset()
    for v, p in zip(('VV', 'VH'), planes):
        ds[v] = (('y', 'x', 'time'), np.ascontiguousarray(np.moveaxis(p, 0, -1)))
        ds_dev[v] = (('time', 'y', 'x'), torch.from_numpy(p).to(device))       # device data, time-first
    for alpha in (0.01, 0.9):
        got = OmnibusTest(ml=3, alpha=alpha, pol='diag', channels=['VV', 'VH']).apply(ds)
        smooth = BoxcarFilter(dims=('y', 'x'), w=3).apply(ds)
        want = OmnibusTest(n=9, alpha=alpha, pol='diag', channels=['VV', 'VH']).apply(smooth)
        np.testing.assert_array_equal(got.values, want.values)
        assert want.values.any()
        got_dev = OmnibusTest(ml=3, alpha=alpha, pol='diag', channels=['VV', 'VH']).apply(ds_dev)
        np.testing.assert_array_equal(got_dev.values.cpu().numpy(), want.values)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_q2_against_the_dual_pol_test(device, dtype):
    """q = 2 and the 2 x 2 test on the same planes with zero C12 share ln Q: z_diag / T(rho_diag) equals
    z_c2 / T(rho_c2) within 2 ulp (one rounding to T on each side) -- and their maps differ, which shows that
    the block-diagonal constants (f = 2 (j - 1) instead of 4 (j - 1), rho, omega2) are in use."""
    import torch
    from nd_amd import kernels
    from tests import omnibus_diag_ref as R
    k, n = 10, 9
    planes = C.gamma_stack(77, 2, k, 5, 130, n, dtype)
    ts = [torch.from_numpy(p).to(device) for p in planes]
    zero = torch.zeros_like(ts[0])
    T = np.dtype(dtype).type
    rho_d = T(R.constants((1, 1), k, n)[1])
    rho_c = T(R.constants((2,), k, n)[1])
    differ = 0
    for alpha in (0.01, 0.9):
        ch_d, z_d, _ = kernels.change_detection_diag(ts, alpha=alpha, n=n, stats=True)
        ch_c, z_c, _ = kernels.change_detection(ts[0], zero, zero, ts[1], alpha=alpha, n=n, stats=True)
        a = z_d.cpu().numpy().astype(np.float64) / float(rho_d)
        b = z_c.cpu().numpy().astype(np.float64) / float(rho_c)
        assert np.all(np.abs(a - b) <= 2 * np.spacing(np.abs(b).astype(T)).astype(np.float64))
        differ += int((ch_d != ch_c).any(dim=-1).sum())
    assert differ > 0


def _ngpu():
    import torch
    return torch.cuda.device_count()


@pytest.mark.skipif(_ngpu() < 2, reason='needs at least two GPUs')
def test_two_gpus(golden):
    """devices=[0, 1] row sharding equals the one-GPU map: pol and channels reach every shard."""
    from nd_amd import xr_lite
    from nd_amd.change import OmnibusTest
    planes = C.gamma_stack(9, 2, 10, 40, 130, 4.4, 'float32')
    ds = xr_lite.Dataset()
    for v, p in zip(('VV', 'VH'), planes):
        ds[v] = (('y', 'x', 'time'), np.ascontiguousarray(np.moveaxis(p, 0, -1)))
    one = OmnibusTest(n=4.4, alpha=0.9, pol='diag', channels=['VV', 'VH']).apply(ds)
    two = OmnibusTest(n=4.4, alpha=0.9, pol='diag', channels=['VV', 'VH'], devices=[0, 1]).apply(ds)
    np.testing.assert_array_equal(one.values, two.values)
    assert one.values.any()
