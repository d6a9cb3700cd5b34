"""Coregistration without a GPU: the numpy restatement (tests/coreg_ref.py) against scikit-image 0.18's
recorded output (tests/golden/coreg_skimage.npz), the C ABI declarations, and argument errors."""
import ctypes
import os

import numpy as np
import pytest

from tests import coreg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'coreg_skimage.npz')
CASES = ('f32_u10', 'f64_u50', 'f32_u1')


def load_case(g, name):
    u, ref = (int(v) for v in g[name + '/meta'])
    names = sorted({key.split('/')[2] for key in g.files if key.startswith(name + '/in/')})
    return (u, ref, {n: g[name + '/in/' + n] for n in names}, {n: g[name + '/out/' + n] for n in names},
            g[name + '/shifts'])


def ulp_diff(a, b, floor):
    """|a - b| in float32 ulps of max(|a|, |b|, floor): a value formed by cancellation of larger terms
    (C12 near 0) carries their rounding, so the unit is never below that of `floor`."""
    a, b = np.asarray(a), np.asarray(b)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    mag = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(floor))
    return np.where(both_nan, 0.0, d / np.spacing(mag.astype(a.dtype)))


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_skimage(golden, name):
    u, ref, ins, outs, want_shifts = load_case(golden, name)
    got, sh = coreg_ref.coregister(ins, ref, u)
    np.testing.assert_array_equal(sh, want_shifts)
    for n in ins:
        assert got[n].dtype == outs[n].dtype
        if got[n].dtype == np.float64:
            np.testing.assert_array_equal(got[n], outs[n])
        else:
            assert np.isnan(got[n]).sum() == np.isnan(outs[n]).sum()
            floor = np.nanmax(np.abs(ins[n])) / 8
            assert np.nanmax(ulp_diff(got[n], outs[n], floor)) <= 4, n


def test_golden_covers_the_contract(golden):
    """The recorded cases exercise what the issue pins: u in {1, 10, 50}, a non-zero reference, a NaN
    plane outside C11 (NaN except exact zeros) and the cval-preserve rule on a positive plane."""
    us = set()
    for name in CASES:
        u, ref, ins, outs, sh = load_case(golden, name)
        us.add(u)
        assert ref != 0
        assert np.array_equal(sh[ref], [0, 0]) and np.array_equal(outs['C11'][ref], ins['C11'][ref])
        assert np.abs(sh).max() > 0.5
    assert us == {1, 10, 50}
    u, ref, ins, outs, _ = load_case(golden, 'f32_u10')
    plane = outs['C22'][3]
    assert np.isnan(plane).mean() > 0.5 and (plane == 0).any()
    assert ins['C11'].min() > 0 and (outs['C11'] == 0).any()


def test_reference_setup_shifts(golden):
    """The recorded set-up of the reference's own test: 50 shifts on the 1/50 grid, introduced shifts
    in [0, 1), and a sample of every variable's output."""
    sh = golden['ref50/shifts']
    intro = golden['ref50/introduced']
    assert sh.shape == (50, 2) and np.array_equal(sh[0], [0, 0]) and np.abs(sh).max() <= 2
    np.testing.assert_allclose(sh * 50, np.round(sh * 50), atol=1e-9)
    assert intro.shape == (50, 2) and (intro[1:] >= 0).all() and (intro < 1).all()
    for n in ('C11', 'C12__im', 'C12__re', 'C22'):
        assert golden['ref50/sample/' + n].shape == (1000,)


def test_restatement_nan_raises():
    a = np.random.default_rng(0).random((3, 16, 20)).astype(np.float32)
    a[1, 4, 5] = np.nan
    with pytest.raises(ValueError, match='NaN values found'):
        coreg_ref.shifts(a, 0, 10)
    a = np.random.default_rng(0).random((3, 16, 20)).astype(np.float32)
    a[0, 2, 2] = np.nan                               # in the reference: every date raises
    with pytest.raises(ValueError, match='NaN values found'):
        coreg_ref.phase_shift(a[2], a[0], 1)


def test_header_declares_and_library_exports():
    from nd_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    names = ('nd_amd_coregister_shifts_workspace_bytes', 'nd_amd_coregister_shifts',
             'nd_amd_warp_translate_workspace_bytes', 'nd_amd_warp_translate')
    L = ctypes.CDLL(build.build())
    for s in names:
        assert s + '(' in hdr
        assert hasattr(L, s)
        assert s in _lib.SYMBOLS
    assert _lib.lib().nd_amd_abi_version() == 1


def test_abi_argument_validation_without_gpu():
    from nd_amd import _lib
    L = _lib.lib()
    assert L.nd_amd_coregister_shifts_workspace_bytes(7, 4, 16, 16, 10) == 0
    assert L.nd_amd_coregister_shifts_workspace_bytes(0, 4, 16, 16, 129) == 0
    assert L.nd_amd_coregister_shifts_workspace_bytes(0, 24, 4096, 4096, 50) > 24 * 4096 * 4096 * 4 * 3
    rc = L.nd_amd_coregister_shifts(None, 0, 4, 16, 16, 256, 16, 1, 4, 10, None, None, None, 0, None)
    assert rc == _lib.EINVAL and b'reference' in L.nd_amd_last_error()
    rc = L.nd_amd_coregister_shifts(None, 3, 4, 16, 16, 256, 16, 1, 0, 10, None, None, None, 0, None)
    assert rc == _lib.EINVAL and b'dtype' in L.nd_amd_last_error()
    assert L.nd_amd_warp_translate_workspace_bytes(0, 17, 4, 16, 16, 0) == 0
    assert L.nd_amd_warp_translate_workspace_bytes(0, 4, 4, 16, 16, 2) == 0
    assert L.nd_amd_warp_translate_workspace_bytes(1, 4, 4, 16, 16, 1) > 0
    rc = L.nd_amd_warp_translate(None, None, 1, 0, 4, 16, 16, 5, None, -1, None, 0, None)
    assert rc == _lib.EINVAL and b'layout' in L.nd_amd_last_error()


def _lite(values, dims=('time', 'y', 'x')):
    from nd_amd import xr_lite
    ds = xr_lite.Dataset()
    for n, v in values.items():
        ds[n] = (dims, v)
    return ds


def test_apply_argument_errors():
    from nd_amd.warp import Coregistration, coregister
    a = np.ones((3, 8, 9), np.float32)
    with pytest.raises(KeyError):
        Coregistration().apply(_lite({'C22': a}))
    with pytest.raises(IndexError):
        Coregistration(reference=3).apply(_lite({'C11': a}))
    with pytest.raises(IndexError):
        coregister(_lite({'C11': a}), reference=-4)
    with pytest.raises(TypeError):
        Coregistration().apply(_lite({'C11': a, 'C22': np.ones((3, 8, 9), np.int32)}))
    from nd_amd import xr_lite
    ds = _lite({'C11': a})
    ds['extra'] = (('time', 'y', 'x', 'band'), np.ones((3, 8, 9, 2), np.float32))
    with pytest.raises(ValueError):
        Coregistration().apply(ds)
    assert isinstance(ds, xr_lite.Dataset)
