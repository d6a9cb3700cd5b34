"""Regions of a map without a GPU: the by_value restatement (tests/regions_ref.py) against a flood fill, hand-counted
cases of the definition, the sieve's identities, the header and the entries' argument checks."""
import ctypes
import os
import re
from collections import deque

import numpy as np
import pytest

from tests import regions_cases as cases
from tests import regions_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flood(v, connectivity, background, by_value):
    """breadth-first flood fill in raster order: independent of scipy"""
    v = np.asarray(v)
    ny, nx = v.shape
    bg = v.dtype.type(background)
    labels = np.zeros((ny, nx), np.int32)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]

    def fg(y, x):
        return v[y, x] != bg and v[y, x] == v[y, x]
    n = 0
    for y in range(ny):
        for x in range(nx):
            if labels[y, x] or not fg(y, x):
                continue
            n += 1
            labels[y, x] = n
            todo = deque([(y, x)])
            while todo:
                cy, cx = todo.popleft()
                for dy, dx in steps:
                    py, px = cy + dy, cx + dx
                    if (0 <= py < ny and 0 <= px < nx and not labels[py, px] and fg(py, px)
                            and (not by_value or v[py, px] == v[cy, cx])):
                        labels[py, px] = n
                        todo.append((py, px))
    return labels, n


def test_restatement_equals_flood_fill():
    rng = np.random.default_rng(20261020)
    for i in range(50):
        ny, nx = (int(s) for s in rng.integers(1, 24, size=2))
        dtype = cases.DTYPES[1 + i % 5]
        v = cases.class_map(rng, (ny, nx), int(rng.integers(2, 6)), dtype)
        bg = [0, 3][i % 2]
        for conn in (4, 8):
            for by_value in (True, False):
                got, n = ref.label(v, conn, bg, by_value)
                want, m = flood(v, conn, bg, by_value)
                assert n == m and np.array_equal(got, want), (i, conn, by_value, dtype)
                assert got.dtype == np.int32


def test_diagonal_pair():
    v = np.array([[1, 0], [0, 1]], np.uint8)
    assert ref.label(v, 4)[1] == 2 and ref.label(v, 8)[1] == 1
    assert np.array_equal(ref.label(v, 4)[0], [[1, 0], [0, 2]])


def test_ring_and_hole():
    v = np.ones((5, 5), np.uint8)
    v[1:4, 1:4] = 0
    v[2, 2] = 1
    lab, n = ref.label(v, 8)
    assert n == 2 and lab[0, 0] == 1 and lab[2, 2] == 2
    assert list(ref.sizes(lab, n)) == [16, 1]
    # with background 1 the ring of zeros around the centre is the only region
    lab0, n0 = ref.label(v, 4, background=1)
    assert n0 == 1 and lab0[1, 1] == 1 and lab0[2, 2] == 0 and int(ref.sizes(lab0, n0)[0]) == 8


def test_background_other_than_zero():
    v = np.array([[3, 3, 0], [3, 5, 0]], np.int32)
    lab, n = ref.label(v, 4, background=3)
    assert n == 1 and np.array_equal(lab, [[0, 0, 1], [0, 1, 1]])
    lab, n = ref.label(v, 4, background=3, by_value=True)
    assert n == 2 and np.array_equal(lab, [[0, 0, 1], [0, 2, 1]])
    lab, n = ref.label(v, 4, background=9, by_value=True)
    assert n == 3 and np.array_equal(lab, [[1, 1, 2], [1, 3, 2]])


def test_negative_zero_and_nan():
    v = np.array([[-0.0, 0.0, 2.0]], np.float32)
    assert ref.label(v, 4, background=0)[1] == 1                 # -0.0 is background too
    lab, n = ref.label(v, 4, background=7, by_value=True)
    assert n == 2 and np.array_equal(lab, [[1, 1, 2]])           # -0.0 == 0.0: one region
    v = np.array([[1.0, np.nan, 1.0]], np.float64)
    for by_value in (False, True):
        lab, n = ref.label(v, 8, by_value=by_value)
        assert n == 2 and np.array_equal(lab, [[1, 0, 2]])       # NaN separates, and is background
    assert ref.label(v, 4, background=np.nan)[1] == 2            # even where NaN is named the background


def test_int64_compared_as_int64():
    a, b = 2 ** 53, 2 ** 53 + 1                                      # equal as doubles
    assert float(a) == float(b)
    v = np.array([[a, b]], np.int64)
    assert ref.label(v, 4, by_value=True)[1] == 2
    assert ref.label(v, 4, by_value=False)[1] == 1
    assert ref.label(v, 4, background=a)[1] == 1 and ref.label(v, 4, background=a)[0][0, 0] == 0


def test_single_row_and_column():
    v = np.array([[1, 1, 0, 1, 0, 0, 1, 1, 1]], np.uint8)
    for plane in (v, v.T.copy()):
        for conn in (4, 8):
            lab, n = ref.label(plane, conn)
            assert n == 3 and list(ref.sizes(lab, n)) == [2, 1, 3]
            assert np.array_equal(lab.ravel(), [1, 1, 0, 2, 0, 0, 3, 3, 3])


def test_adversarial_counts():
    assert ref.label(cases.serpentine(), 4)[1] == 1
    assert ref.label(1 - cases.serpentine(), 4)[1] == 65
    assert ref.label(cases.checkerboard(), 4)[1] == 5250 and ref.label(cases.checkerboard(), 8)[1] == 1
    assert ref.label(cases.spiral(), 4)[1] == 1 and ref.label(cases.spiral(), 8)[1] == 1
    assert 0.3 < cases.spiral().mean() < 0.7
    for plane in cases.stripes().values():
        assert ref.label(plane, 4)[1] == 1
    assert ref.label(cases.frames(), 8)[1] == 34
    assert ref.label(cases.antidiagonal(), 4)[1] == 130 and ref.label(cases.antidiagonal(), 8)[1] == 1


def test_sizes_sum_to_the_foreground():
    rng = np.random.default_rng(3)
    for dtype in cases.DTYPES[1:]:
        v = cases.class_map(rng, (40, 50), 4, dtype)
        for by_value in (False, True):
            lab, n = ref.label(v, 8, 0, by_value)
            assert ref.sizes(lab, n).sum() == ref.foreground(v).sum() == (lab > 0).sum()
            assert np.array_equal(ref.area(lab, n) > 0, lab > 0)


def test_sieve_identities():
    rng = np.random.default_rng(4)
    for dtype in ('uint8', 'float32'):
        v = cases.class_map(rng, (40, 50), 4, dtype)
        for by_value in (False, True):
            for m in (0, 1):
                cases.assert_same(ref.sieve(v, m, 4, 0, by_value), v)
            once = ref.sieve(v, 5, 4, 0, by_value)
            cases.assert_same(ref.sieve(once, 5, 4, 0, by_value), once)
            assert not ref.foreground(ref.sieve(v, 10 ** 6, 8, 0, by_value)).any()
            filled = ref.sieve(v, 10 ** 6, 8, 0, by_value, fill=9)
            assert (filled[ref.foreground(v)] == 9).all()
            cases.assert_same(filled[~ref.foreground(v)], v[~ref.foreground(v)])     # NaN bits kept


def test_header_declares_the_entries():
    from nd_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('nd_amd_label_regions', 'nd_amd_region_sizes', 'nd_amd_sieve_regions',
                 'nd_amd_regions_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.SYMBOLS
    assert 'Regions of a map' in hdr
    assert _lib.KERNEL_NAMES[30] == 'regions' and re.search(r'#define\s+ND_AMD_KERNEL_REGIONS\s+30\b', hdr)
    for name, value in (('U8', _lib.U8), ('I32', _lib.I32), ('EINTERNAL', _lib.EINTERNAL)):
        assert re.search(r'#define\s+ND_AMD_%s\s+%d\b' % (name, value), hdr), name


def _label(L, dtype=3, nplanes=1, ny=8, nx=8, conn=4, ptr=None, strides=(64, 8, 1)):
    from nd_amd import _lib
    s = _lib.i64_array(strides)
    bg = ctypes.c_int64(0)
    return L.nd_amd_label_regions(ptr, dtype, nplanes, ny, nx, s, conn, 0, ctypes.byref(bg), ptr, s, None, None, ptr,
                                  None, 0, None)


def _sieve(L, dtype=3, nplanes=1, ny=8, nx=8, conn=4, ptr=None):
    from nd_amd import _lib
    s = _lib.i64_array((64, 8, 1))
    bg = ctypes.c_int64(0)
    return L.nd_amd_sieve_regions(ptr, ptr, dtype, nplanes, ny, nx, s, s, conn, 0, ctypes.byref(bg), ctypes.byref(bg),
                                  4, None, 0, None)


def test_region_argument_validation_without_gpu():
    """every refusal below comes before the first HIP call"""
    from nd_amd import _lib
    L = _lib.lib()
    dummy = ctypes.c_void_p(4096)
    for call in (_label, _sieve):
        assert call(L, dtype=9) == _lib.EINVAL
        assert b'dtype' in L.nd_amd_last_error()
        assert call(L, conn=6) == _lib.EINVAL
        assert b'connectivity' in L.nd_amd_last_error()
        assert call(L, ny=-1) == _lib.EINVAL
        assert call(L, nplanes=-1) == _lib.EINVAL
        assert call(L, ny=1 << 16, nx=1 << 15) == _lib.EUNSUPPORTED          # 2^31 pixels, null pointers
        assert b'2^31' in L.nd_amd_last_error()
        assert call(L, ny=0) == _lib.OK and call(L, nx=0) == _lib.OK and call(L, nplanes=0) == _lib.OK
        assert call(L) == _lib.EINVAL                                        # null pointers
        assert call(L, ptr=dummy) == _lib.EWORKSPACE                         # never dereferenced
    assert _label(L, ptr=dummy, strides=(64, -8, 1)) == _lib.EINVAL
    s = _lib.i64_array((64, 8, 1))
    assert L.nd_amd_region_sizes(None, s, 1, -1, 8, None, None, 0, None) == _lib.EINVAL
    assert L.nd_amd_region_sizes(None, s, 1, 1 << 16, 1 << 15, None, None, 4, None) == _lib.EUNSUPPORTED
    assert L.nd_amd_region_sizes(None, s, 1, 8, 8, None, None, 0, None) == _lib.OK
    assert L.nd_amd_region_sizes(None, s, 1, 8, 8, None, dummy, 4, None) == _lib.EINVAL
    assert L.nd_amd_regions_workspace_bytes(1, 1 << 16, 1 << 15, 0) == 0
    one = L.nd_amd_regions_workspace_bytes(1, 100, 100, 0)
    assert 40000 <= one < 40000 + 2048 and L.nd_amd_regions_workspace_bytes(1, 100, 100, 1) >= one + 40000


def test_background_must_be_representable():
    import torch
    from nd_amd import kernels as K
    assert K.region_element(3, torch.uint8) == 3 and K.region_element(True, torch.bool) == 1
    assert K.region_element(2 ** 53 + 1, torch.int64) == 2 ** 53 + 1
    assert np.isnan(K.region_element(float('nan'), torch.float32))
    assert np.signbit(K.region_element(-0.0, torch.float64))
    for value, dtype in ((256, torch.uint8), (-1, torch.uint8), (2, torch.bool), (0.5, torch.int32),
                         (2 ** 31, torch.int32), (float('nan'), torch.int64), (0.1, torch.float32),
                         (1e40, torch.float32)):
        with pytest.raises(ValueError, match='representable'):
            K.region_element(value, dtype)
    with pytest.raises(TypeError):
        K.region_element(0, torch.int16)


def test_wrappers_refuse_before_the_device():
    import torch
    from nd_amd import kernels as K
    from nd_amd import regions, xr_lite
    t = torch.zeros((4, 5), dtype=torch.uint8)
    with pytest.raises(ValueError, match='ROCm device'):
        K.label_regions(t)
    with pytest.raises(ValueError, match='ROCm device'):
        K.sieve_regions(t, 3)
    da = xr_lite.DataArray(np.zeros((4, 5), np.uint8), ('y', 'x'))
    with pytest.raises(ValueError, match='connectivity'):
        regions.label_regions(da, connectivity=6)
    with pytest.raises(ValueError, match='connectivity'):
        regions.Sieve(3, connectivity=True)
    with pytest.raises(ValueError, match='min_size'):
        regions.Sieve(2.5)
    with pytest.raises(TypeError, match='complex'):
        regions.sieve(xr_lite.DataArray(np.zeros((4, 5), np.complex64), ('y', 'x')), 3)
    with pytest.raises(ValueError, match='y and x'):
        regions.label_regions(xr_lite.DataArray(np.zeros((4, 5), np.uint8), ('time', 'x')))
