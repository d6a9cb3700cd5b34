"""change_segments without a GPU: the inputs hold every code, the numpy restatement
(tests/change_segments_ref.py) agrees with things that owe nothing to it -- eigenvalues, np.mean over segments
enumerated by hand, the block-diagonal case, step stacks -- and the argument checks of the C entry point and
of the public interface run before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

from tests import change_segments_cases as cases
from tests import change_segments_ref as R

CORE = cases.core_cases()


def _hermitian(d, structure):
    if structure == 'diag':
        return np.diag(np.array(d, np.complex128))
    if structure == 'c2':
        c12 = d[1] + 1j * d[2]
        return np.array([[d[0], c12], [np.conj(c12), d[3]]], np.complex128)
    c12, c13, c23 = d[3] + 1j * d[4], d[5] + 1j * d[6], d[7] + 1j * d[8]
    return np.array([[d[0], c12, c13], [np.conj(c12), d[1], c23], [np.conj(c13), np.conj(c23), d[2]]], np.complex128)


def _segments(row):
    """[(first, last + 1)] of one pixel's segments, enumerated from its map bytes."""
    k = len(row)
    starts = [0] + [t for t in range(1, k) if row[t]]
    return list(zip(starts, starts[1:] + [k]))


@pytest.mark.parametrize('case', CORE, ids=cases.case_id)
def test_inputs_hold_every_code(case):
    """A condition on the inputs, from the restatement alone: each of the codes 1, 2 and 3 makes up at least
    10 % of the flagged positions of every core case (a single date has no position to flag)."""
    planes, change = cases.make(*case)
    direction, _ = R.change_segments(planes, change, case[0])
    flagged = direction[..., 1:][change[..., 1:] != 0]
    assert (direction[..., 0] == 0).all() and (direction[change == 0] == 0).all()
    if case[3] == 1:
        assert flagged.size == 0
        return
    assert flagged.size >= 10 and (flagged > 0).all()
    for c in (1, 2, 3):
        assert (flagged == c).mean() >= 0.10, (c, (flagged == c).mean())


@pytest.mark.parametrize('case', [c for c in CORE if c[3:6] in ((10, 5, 130), (3, 3, 65), (33, 2, 64))],
                         ids=cases.case_id)
def test_codes_are_the_signs_of_the_eigenvalues(case):
    """Wherever the smallest |eigenvalue| of the difference matrix exceeds 1e-9 of the largest, the code is the
    sign pattern np.linalg.eigvalsh gives; the differences are taken from np.mean over segments enumerated
    pixel by pixel, not from the restatement's sums."""
    structure = case[0]
    planes, change = cases.make(*case)
    direction, _ = R.change_segments(planes, change, structure)
    k, ny, nx = planes[0].shape
    mats, got = [], []
    for y in range(ny):
        for x in range(nx):
            for first, end in _segments(change[y, x])[:-1]:
                d = [float(p[end, y, x]) - float(np.mean(p[first:end, y, x].astype(np.float64))) for p in planes]
                mats.append(_hermitian(d, structure))
                got.append(direction[y, x, end])
    ev = np.linalg.eigvalsh(np.array(mats))
    got = np.array(got)
    clear = np.abs(ev).min(axis=1) > 1e-9 * np.abs(ev).max(axis=1)
    want = np.where((ev > 0).all(axis=1), 1, np.where((ev < 0).all(axis=1), 2, 3))
    assert clear.sum() >= 0.6 * len(got)
    np.testing.assert_array_equal(got[clear], want[clear])


@pytest.mark.parametrize('case', [c for c in CORE if c[2] == np.float64 and c[3:6] in ((10, 5, 130), (33, 2, 64))],
                         ids=cases.case_id)
def test_means_are_np_mean_over_hand_enumerated_segments(case):
    planes, change = cases.make(*case)
    _, means = R.change_segments(planes, change, case[0])
    k, ny, nx = planes[0].shape
    for y in range(ny):
        for x in range(nx):
            for first, end in _segments(change[y, x]):
                for p, mp in zip(planes, means):
                    want = np.mean(p[first:end, y, x])
                    assert (mp[first:end, y, x] == mp[first, y, x]).all()
                    assert abs(mp[first, y, x] - want) <= 1e-13 * abs(want)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_c2_with_zero_c12_gives_the_two_intensity_codes(dtype):
    planes, change = cases.make('diag', 2, dtype, 10, 5, 130, 99)
    zero = np.zeros_like(planes[0])
    d2, m2 = R.change_segments(planes, change, 'diag')
    d4, m4 = R.change_segments([planes[0], zero, zero, planes[1]], change, 'c2')
    np.testing.assert_array_equal(d2, d4)
    np.testing.assert_array_equal(m2[0], m4[0])
    np.testing.assert_array_equal(m2[1], m4[3])
    assert all((d2 == c).sum() > 100 for c in (1, 2, 3))


@pytest.mark.parametrize('kind, code', [('up', 1), ('down', 2), ('mixed', 3)])
def test_step_stacks(kind, code):
    planes = cases.step_stack(kind)
    change = np.zeros((5, 5, 10), np.uint8)
    change[..., 5] = 1
    direction, means = R.change_segments(planes, change, 'c2')
    assert (direction[..., 5] == code).all()
    assert (np.delete(direction, 5, axis=-1) == 0).all()
    for m in means:
        assert (m[:5] == m[0]).all() and (m[5:] == m[5]).all()


def test_c_entry_validation():
    """nd_amd_change_segments rejects a bad dtype, structure, plane count, extent, null pointers and a call
    without outputs before any HIP call; an empty raster is served."""
    from nd_amd import _lib
    L = _lib.lib()
    buf = np.ones(64, np.float32)
    cmap = np.zeros(64, np.uint8)
    out = np.zeros(64, np.int8)
    ptrs = (C.c_void_p * 9)(*[buf.ctypes.data] * 9)
    holes = (C.c_void_p * 9)(*([buf.ctypes.data] * 3 + [None] + [buf.ctypes.data] * 5))

    def call(planes=ptrs, nplanes=4, structure=_lib.STRUCT_C2, dtype=_lib.F32, shape=(2, 4, 4), change=cmap,
             direction=out, means=None):
        return L.nd_amd_change_segments(planes, nplanes, structure, dtype, shape[0], shape[1], shape[2], 4, 1, 16,
                                        None if change is None else C.c_void_p(change.ctypes.data),
                                        None if direction is None else C.c_void_p(direction.ctypes.data),
                                        means, None)
    assert call(dtype=7) == _lib.EINVAL and b'dtype' in L.nd_amd_last_error()
    assert call(structure=3) == _lib.EINVAL and b'structure' in L.nd_amd_last_error()
    assert call(structure=-1) == _lib.EINVAL
    for structure, counts, word in ((_lib.STRUCT_DIAG, (0, 4, 9), b'one to three'), (_lib.STRUCT_C2, (3, 9), b'four'),
                                    (_lib.STRUCT_C3, (4, 8, 10), b'nine')):
        for n in counts:
            assert call(nplanes=n, structure=structure) == _lib.EINVAL
            msg = L.nd_amd_last_error()
            assert word in msg and str(n).encode() in msg
    for shape in ((-1, 4, 4), (2, -4, 4), (2, 4, -1)):
        assert call(shape=shape) == _lib.EINVAL and b'negative' in L.nd_amd_last_error()
    assert call(direction=None) == _lib.EINVAL and b'neither' in L.nd_amd_last_error()
    assert call(planes=None) == _lib.EINVAL and b'null' in L.nd_amd_last_error()
    assert call(change=None) == _lib.EINVAL and b'null' in L.nd_amd_last_error()
    assert call(planes=holes) == _lib.EINVAL and b'plane 3' in L.nd_amd_last_error()
    assert call(direction=None, means=holes) == _lib.EINVAL and b'means plane 3' in L.nd_amd_last_error()
    for shape in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert call(shape=shape) == _lib.OK
        assert call(shape=shape, planes=None, change=None) == _lib.OK
    assert _lib.KERNEL_NAMES[26] == 'change_segments'


def test_python_errors():
    """The checks of the public interface name what is wrong and come before any device work."""
    from nd_amd import xr_lite
    from nd_amd.change import change_direction, change_segments, segment_means
    a = np.ones((3, 4, 5), np.float32)
    ds = xr_lite.Dataset()
    for v in ('C11', 'C22', 'VV'):
        ds[v] = (('y', 'x', 'time'), a)
    ds['C12'] = (('y', 'x', 'time'), a.astype(np.complex64))
    good = xr_lite.DataArray(np.zeros((3, 4, 5), bool), dims=('y', 'x', 'time'))
    with pytest.raises(ValueError, match="'dual'.*'full'.*'diag'"):
        change_segments(ds, good, pol='quad')
    with pytest.raises(ValueError, match=r'\(3, 4, 6\).*\(3, 4, 5\)'):
        change_segments(ds, xr_lite.DataArray(np.zeros((3, 4, 6), bool), dims=('y', 'x', 'time')))
    with pytest.raises(ValueError, match=r'\(3, 4, 6\).*\(3, 4, 5\)'):
        change_direction(ds, xr_lite.DataArray(np.zeros((6, 3, 4), np.uint8), dims=('time', 'y', 'x')))
    for dtype in (np.int8, np.float32, np.int64):
        with pytest.raises(TypeError, match='bool or uint8'):
            segment_means(ds, xr_lite.DataArray(np.zeros((3, 4, 5), dtype), dims=('y', 'x', 'time')))
    with pytest.raises(ValueError, match='dimensions y, x, time'):
        change_segments(ds, xr_lite.DataArray(np.zeros((3, 4), bool), dims=('y', 'x')))
    with pytest.raises(TypeError, match='C12'):
        change_segments(ds, good, pol='diag', channels=['VV', 'C12'])
    with pytest.raises(KeyError, match='VH'):
        change_segments(ds, good, pol='diag', channels=['VV', 'VH'])
    with pytest.raises(KeyError, match='C33'):
        change_segments(ds, good, pol='full')
    with pytest.raises(ValueError, match='neither'):
        change_segments(ds, good, direction=False, means=False)
