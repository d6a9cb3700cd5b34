"""CPU tests of the host side: the C ABI loads and exports what include/nd_amd.h declares, argument
validation that needs no GPU, the footprint builder, the xr_lite container, the Algorithm API
(nd/tests/test_algorithm.py re-stated) and the chunk/halo arithmetic."""
import ctypes
import inspect
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ C ABI
def _declared_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    return sorted(set(re.findall(r'\b(nd_amd_[a-z0-9_]+)\s*\(', hdr)))


def test_library_exports_every_declared_symbol():
    from nd_amd import _lib, build
    lib = build.build()
    L = ctypes.CDLL(lib)
    declared = _declared_symbols()
    assert declared, 'no prototypes found in include/nd_amd.h'
    for s in declared:
        assert hasattr(L, s), 'libnd_amd.so does not export %s' % s
    assert sorted(_lib.SYMBOLS) == declared
    assert _lib.lib().nd_amd_abi_version() == 1


def test_argument_validation_without_gpu():
    from nd_amd import _lib
    L = _lib.lib()
    # bad dtype / negative shape are rejected before any HIP call
    rc = L.nd_amd_omnibus_c2(None, None, None, None, 7, 4, 4, 4, 4, 1, 16, 1, 0.5, None, None, None,
                             None, 0, None)
    assert rc == _lib.EINVAL
    assert b'dtype' in L.nd_amd_last_error()
    rc = L.nd_amd_omnibus_c2(None, None, None, None, 0, -1, 4, 4, 4, 1, 16, 1, 0.5, None, None, None,
                             None, 0, None)
    assert rc == _lib.EINVAL
    # empty raster: nothing to do
    rc = L.nd_amd_omnibus_c2(None, None, None, None, 0, 0, 4, 4, 4, 1, 16, 1, 0.5, None, None, None,
                             None, 0, None)
    assert rc == _lib.OK
    with pytest.raises(_lib.NdAmdError):
        _lib.check(_lib.EINVAL)
    mn = ctypes.c_size_t(0)
    rec = L.nd_amd_omnibus_c2_workspace_bytes(0, 4096, 4096, 24, ctypes.byref(mn))
    assert rec >= mn.value > 4096 * 4096 * 4


def _entry_code_cases():
    """(id, entry, overrides, expected code, message prefix) for the seven change-detection entries.  Every case
    returns before the first HIP call: refused arguments and check_workspace come first, so the non-null addresses
    (DUMMY) are never dereferenced.  The cases with two faults pin the ORDER of the checks."""
    from nd_amd import _lib
    OK, EINVAL, EWS, EUNS = _lib.OK, _lib.EINVAL, _lib.EWORKSPACE, _lib.EUNSUPPORTED
    nan, inf = float('nan'), float('inf')
    big = 65536                                       # 65536 x 65536 pixels: one past the 32-bit pixel index
    cases = []

    def add(entry, name, expect, impl=None, **over):
        # impl: refused one level down, in the family's *_impl, whose name then begins the message -- the workspace
        # always is (check_workspace), the full-pol date limit too
        impl = expect == EWS if impl is None else impl
        prefix = _ENTRY_NAMES[_IMPL_OF.get(entry, entry) if impl else entry]
        cases.append(('%s-%s' % (entry, name), entry, over, expect, prefix))

    def common(entry, nplanes, dims_ok=OK):
        add(entry, 'bad_dtype', EINVAL, dtype=7)
        add(entry, 'bad_dtype_empty', EINVAL, dtype=7, ny=0, null=True)
        for d in ('ny', 'nx', 'k'):
            add(entry, 'negative_' + d, EINVAL, **{d: -1})
            add(entry, 'zero_%s_all_null' % d, dims_ok, **{d: 0, 'null': True})
        add(entry, 'zero_ny_negative_nx', EINVAL, ny=0, nx=-1, null=True)
        for p in range(nplanes):
            add(entry, 'plane%d_null' % p, EINVAL, null_planes=(p,))
        add(entry, 'change_null', EINVAL, change=None)

    for entry in ('c2', 'c2_pm', 'c3', 'c3_pm'):
        common(entry, 4 if entry.startswith('c2') else 9)
        add(entry, 'no_looks', EINVAL, n_looks=0)
        add(entry, 'no_looks_empty', OK, n_looks=0, nx=0, null=True)
        add(entry, 'no_looks_too_many_pixels', EINVAL, n_looks=0, ny=big, nx=big)
        add(entry, 'plane_null_too_many_pixels', EINVAL, null_planes=(1,), ny=big, nx=big)
        add(entry, 'too_many_pixels', EUNS, ny=big, nx=big)
        add(entry, 'most_pixels_no_workspace', EWS, ny=big, nx=big - 1)     # 2^32 - 65536 pixels: admitted
        add(entry, 'no_workspace', EWS)
        add(entry, 'short_workspace', EWS, workspace=DUMMY, workspace_bytes=256)
        add(entry, 'misaligned_workspace', EINVAL, impl=True, workspace=DUMMY + 16, workspace_bytes=1 << 40)
    add('c2', 'too_many_dates', EUNS, k=0x40000000)
    add('c2', 'most_dates_no_workspace', EWS, k=4096)
    add('c2_pm', 'too_many_dates', EUNS, k=193)
    add('c2_pm', 'most_dates_no_workspace', EWS, k=192)
    for entry in ('c3', 'c3_pm'):
        add(entry, 'planes_null', EINVAL, planes=None)
        add(entry, 'too_many_dates', EUNS, impl=True, k=97, workspace=DUMMY, workspace_bytes=1 << 40)
        add(entry, 'too_many_dates_no_workspace', EWS, k=97)
    for entry, n in (('c2_pm', 4), ('c3_pm', 9)):
        add(entry, 'date_stride_null', EINVAL, date_stride=None)
        add(entry, 'date_stride_null_empty', EINVAL, date_stride=None, nx=0, null=True)
        for v in range(n):
            add(entry, 'date_stride%d_3' % v, EINVAL, date_stride=[3 if i == v else 1 for i in range(n)])
        add(entry, 'date_stride_0', EINVAL, date_stride=[0] * n)
        add(entry, 'date_stride_2', EWS, date_stride=[2] * n)
        add(entry, 'date_stride_3_too_many_pixels', EINVAL, date_stride=[3] * n, ny=big, nx=big)
    add('c2_pm', 'date_stride_3_empty', EINVAL, date_stride=[3, 3, 3, 3], nx=0, null=True)
    add('c3_pm', 'date_stride_3_empty', OK, date_stride=[3] * 9, nx=0, null=True)
    add('c2_pm', 'c12_halves_differ', EINVAL, date_stride=[1, 1, 2, 1])
    add('c2_pm', 'c12_halves_differ_empty', EINVAL, date_stride=[1, 2, 1, 1], k=0, null=True)
    add('c2_pm', 'c12_interleaved', EWS, date_stride=[1, 2, 2, 1])

    # the fused-multilook entry: the window where the others have the looks
    common('c2_ml', 4)
    add('c2_ml', 'no_window', EINVAL, ml=0)
    add('c2_ml', 'no_window_empty', EINVAL, ml=0, nx=0, null=True)
    add('c2_ml', 'even_window_empty', OK, ml=4, nx=0, null=True)
    add('c2_ml', 'even_window', EUNS, ml=4)
    add('c2_ml', 'plane_null_even_window', EINVAL, ml=4, null_planes=(2,))
    add('c2_ml', 'float64', EUNS, dtype=_lib.F64)
    add('c2_ml', 'one_date', EUNS, k=1)
    add('c2_ml', 'too_many_dates', EUNS, k=25)
    add('c2_ml', 'most_dates_no_workspace', EWS, k=24, stride_t=64)
    add('c2_ml', 'strided_x', EUNS, stride_x=2)
    add('c2_ml', 'narrower_than_the_window', EUNS, ml=5, nx=4)
    add('c2_ml', 'too_many_pixels', EUNS, ny=big, nx=big)
    add('c2_ml', 'no_workspace', EWS)

    # intensities only: a channel count, and real-valued looks that are checked BEFORE the empty raster
    common('diag', 3)
    for nch in (0, 4):
        add('diag', 'nch_%d' % nch, EINVAL, nch=nch)
        add('diag', 'nch_%d_empty' % nch, EINVAL, nch=nch, ny=0, null=True)
    for nch in (1, 2):
        add('diag', 'nch_%d_plane_behind_null' % nch, EWS, nch=nch, null_planes=(nch,))
        add('diag', 'nch_%d_last_plane_null' % nch, EINVAL, nch=nch, null_planes=(nch - 1,))
    add('diag', 'planes_null', EINVAL, planes=None)
    for name, v in (('0', 0.0), ('minus_1', -1.0), ('inf', inf), ('nan', nan)):
        add('diag', 'looks_' + name, EINVAL, n_looks=v)
        add('diag', 'looks_%s_empty' % name, EINVAL, n_looks=v, nx=0, null=True)
    add('diag', 'looks_fractional', EWS, n_looks=4.4)
    add('diag', 'too_many_pixels', EUNS, ny=big, nx=big)
    add('diag', 'plane_null_too_many_pixels', EINVAL, null_planes=(0,), ny=big, nx=big)
    add('diag', 'too_many_dates', EUNS, k=0x7fffffff // 3 + 1)
    add('diag', 'no_workspace', EWS)
    add('diag', 'misaligned_workspace', EINVAL, impl=True, workspace=DUMMY + 16, workspace_bytes=1 << 40)

    # change_segments has no workspace and no pixel limit: valid arguments would launch, so none are given
    common('cs', 4)
    add('cs', 'bad_structure', EINVAL, structure=3)
    add('cs', 'bad_structure_empty', EINVAL, structure=-1, ny=0, null=True)
    for structure, nplanes in ((_lib.STRUCT_DIAG, 0), (_lib.STRUCT_DIAG, 4), (_lib.STRUCT_C2, 3), (_lib.STRUCT_C2, 9),
                               (_lib.STRUCT_C3, 4)):
        add('cs', 'structure_%d_with_%d_planes' % (structure, nplanes), EINVAL, structure=structure, nplanes=nplanes)
        add('cs', 'structure_%d_with_%d_planes_empty' % (structure, nplanes), EINVAL, structure=structure,
            nplanes=nplanes, k=0, null=True)
    add('cs', 'no_output', EINVAL, direction=None, means=None)
    add('cs', 'no_output_empty', EINVAL, direction=None, means=None, nx=0, null=True, keep_outputs=True)
    add('cs', 'direction_only_empty', OK, means=None, nx=0, null=True, keep_outputs=True)
    add('cs', 'means_only_empty', OK, direction=None, k=0, null=True, keep_outputs=True)
    add('cs', 'planes_null', EINVAL, planes=None)
    for p in range(4):
        add('cs', 'means_plane%d_null' % p, EINVAL, null_means=(p,))
    for p in range(9):
        add('cs', 'c3_plane%d_null' % p, EINVAL, structure=_lib.STRUCT_C3, nplanes=9, null_planes=(p,))
    add('cs', 'diag_last_plane_null', EINVAL, structure=_lib.STRUCT_DIAG, nplanes=2, null_planes=(1,), means=None)
    return cases


DUMMY = 0x10000      # a non-null, 256-byte aligned address that is never dereferenced
_ENTRY_NAMES = {'c2': b'nd_amd_omnibus_c2:', 'c2_ml': b'nd_amd_omnibus_c2_ml:', 'c2_pm': b'nd_amd_omnibus_c2_pixel_major:',
                'c3': b'nd_amd_omnibus_c3:', 'c3_pm': b'nd_amd_omnibus_c3_pixel_major:', 'diag': b'nd_amd_omnibus_diag:',
                'cs': b'nd_amd_change_segments:'}
_IMPL_OF = {'c2_ml': 'c2', 'c2_pm': 'c2', 'c3_pm': 'c3'}      # the entry whose *_impl serves it


def _call_entry(L, entry, over):
    """calls one entry with valid arguments for a tiny raster (null workspace), changed by `over`"""
    from nd_amd import _lib
    vp = ctypes.c_void_p
    a = dict(dtype=_lib.F32, ny=8, nx=8, k=4, stride_y=8, stride_x=1, stride_t=64, n_looks=4, ml=3, alpha=0.5,
             change=DUMMY, z_out=None, p_out=None, workspace=None, workspace_bytes=0, nch=3, structure=_lib.STRUCT_C2,
             nplanes=4, direction=DUMMY)
    nplanes = {'c2': 4, 'c2_ml': 4, 'c2_pm': 4, 'c3': 9, 'c3_pm': 9, 'diag': 3, 'cs': over.get('nplanes', 4)}[entry]
    addr = [None if (p in over.get('null_planes', ()) or over.get('null')) else DUMMY + 4096 * p for p in range(9)]
    a['planes'] = (vp * 9)(*addr)
    a['means'] = (vp * 9)(*[None if p in over.get('null_means', ()) else DUMMY for p in range(9)])
    a['date_stride'] = [1] * nplanes
    if over.get('null'):                              # an empty raster is admitted with every pointer null
        a.update(planes=None, change=None)
        if entry == 'cs' and not over.get('keep_outputs'):
            a.update(means=None)                      # (direction stays: one output must be asked for)
    a.update({k: v for k, v in over.items() if k not in ('null', 'null_planes', 'null_means', 'keep_outputs')})
    ds = None if a['date_stride'] is None else _lib.i64_array(a['date_stride'])
    c2 = [addr[p] if a['planes'] is not None else None for p in range(4)]
    dims = [a['ny'], a['nx'], a['k']]
    strides = [a['stride_y'], a['stride_x'], a['stride_t']]
    tail = [a['alpha'], a['change'], a['z_out'], a['p_out'], a['workspace'], a['workspace_bytes'], None]
    if entry == 'c2':
        return L.nd_amd_omnibus_c2(*c2, a['dtype'], *dims, *strides, a['n_looks'], *tail)
    if entry == 'c2_ml':
        return L.nd_amd_omnibus_c2_ml(*c2, a['dtype'], *dims, *strides, a['ml'], *tail)
    if entry == 'c2_pm':
        return L.nd_amd_omnibus_c2_pixel_major(*c2, a['dtype'], *dims, ds, a['n_looks'], *tail)
    if entry == 'c3':
        return L.nd_amd_omnibus_c3(a['planes'], a['dtype'], *dims, *strides, a['n_looks'], *tail)
    if entry == 'c3_pm':
        return L.nd_amd_omnibus_c3_pixel_major(a['planes'], a['dtype'], *dims, ds, a['n_looks'], *tail)
    if entry == 'diag':
        return L.nd_amd_omnibus_diag(a['planes'], a['nch'], a['dtype'], *dims, *strides, float(a['n_looks']), *tail)
    assert entry == 'cs'
    return L.nd_amd_change_segments(a['planes'], a['nplanes'], a['structure'], a['dtype'], *dims, *strides, a['change'],
                                    a['direction'], a['means'], None)


def test_entry_return_codes_without_gpu():
    """The return code of every refusal of the seven change-detection entries, and of the empty raster, as a table
    (_entry_code_cases); a refusal also leaves a message that begins with the entry's name."""
    from nd_amd import _lib
    L = _lib.lib()
    cases = _entry_code_cases()
    assert len(set(c[0] for c in cases)) == len(cases)
    wrong = []
    for cid, entry, over, expect, prefix in cases:
        rc = _call_entry(L, entry, over)
        msg = L.nd_amd_last_error()
        if rc != expect:
            wrong.append('%s: %d, expected %d (%s)' % (cid, rc, expect, msg.decode()))
        elif rc != _lib.OK and not msg.startswith(prefix):
            wrong.append('%s: message %r does not begin with %r' % (cid, msg, prefix))
        elif 'dtype' in cid and b'dtype' not in msg:
            wrong.append('%s: message %r does not name the dtype' % (cid, msg))
    assert not wrong, '\n'.join(wrong)


def test_ops_refuse_cpu_tensors():
    import torch
    from nd_amd import kernels
    t = torch.zeros((3, 4, 5))
    with pytest.raises(ValueError, match='ROCm device'):
        kernels.change_detection(t, t, t, t, alpha=0.5)
    with pytest.raises(ValueError, match='ROCm device'):
        kernels.convolve(t, np.ones((1, 3, 3)))


# ------------------------------------------------------------------ footprint
def _correlate_numpy(a, offs, w, mode='reflect'):
    """Straightforward evaluation of the footprint with numpy.pad (reflect = scipy 'reflect')."""
    pad = int(np.abs(offs).max()) if len(offs) else 0
    ap = np.pad(a, pad, mode='symmetric')
    out = np.zeros(a.shape, np.float64)
    for o, wt in zip(offs, w):
        sl = tuple(slice(pad + o[d], pad + o[d] + a.shape[d]) for d in range(a.ndim))
        out = out + wt * ap[sl]
    return out


@pytest.mark.parametrize('kshape', [(3, 3), (5, 4), (2, 2), (1, 7), (6, 1)])
def test_footprint_matches_scipy(kshape):
    import scipy.ndimage as ndi
    from nd_amd import kernels
    rng = np.random.default_rng(5)
    a = rng.normal(size=(11, 13))
    k = rng.normal(size=kshape)
    k.flat[1 % k.size] = 0.0
    offs, w = kernels.footprint(k)
    assert len(w) == np.count_nonzero(k)
    np.testing.assert_allclose(_correlate_numpy(a, offs, w), ndi.convolve(a, k), rtol=1e-12, atol=1e-12)
    offs_c, w_c = kernels.footprint(k, convolution=False)
    np.testing.assert_allclose(_correlate_numpy(a, offs_c, w_c), ndi.correlate(a, k), rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match='invalid origin'):
        kernels.footprint(k, origin=9)


# ------------------------------------------------------------------ xr_lite + io
def test_xr_lite_basics():
    from nd_amd import xr_lite
    ds = synth.lite_test_dataset()
    assert list(ds.data_vars) == ['C11', 'C12__im', 'C12__re', 'C22']
    assert ds.dims == OrderedDict([('time', 10), ('x', 20), ('y', 20)])
    sub = ds.isel(time=slice(2, 5))
    assert sub['C11'].shape == (20, 20, 3) and len(sub.coords['time']) == 3
    da = ds[['C11', 'C22']].to_array().transpose('y', 'x', 'time', 'variable')
    assert da.shape == (20, 20, 10, 2)
    back = xr_lite.expand_variables(da)
    assert back['C22'].equals(ds['C22'])
    cat = xr_lite.concat([ds.isel(y=slice(0, 7)), ds.isel(y=slice(7, None))], dim='y')
    assert cat.equals(ds)
    deep = ds.copy(deep=True)
    deep['C11'].values[0, 0, 0] += 1
    assert not deep.equals(ds)


def test_complex_convention():
    """nd/tests/test_convert.py: C12 <-> C12__re / C12__im"""
    from nd_amd.io import assemble_complex, disassemble_complex
    ds = synth.lite_test_dataset()
    c = assemble_complex(ds)
    assert set(c.data_vars) == {'C11', 'C22', 'C12'}
    np.testing.assert_array_equal(c['C12'].values, ds['C12__re'].values + 1j * ds['C12__im'].values)
    d = disassemble_complex(c)
    assert set(d.data_vars) == {'C11', 'C22', 'C12__re', 'C12__im'}
    np.testing.assert_array_equal(d['C12__im'].values, ds['C12__im'].values)
    assert 'C12' in c                       # not modified in place
    disassemble_complex(c, inplace=True)
    assert 'C12' not in c and 'C12__re' in c


# ------------------------------------------------------------------ Algorithm API
def test_wrap_algorithm_and_parallelize():
    """nd/tests/test_algorithm.py:35-88"""
    from nd_amd import xr_lite
    from nd_amd.algorithm import Algorithm, parallelize, wrap_algorithm

    class DummyAlgorithm(Algorithm):
        """test docstring"""

        def __init__(self, value, *args, **kwargs):
            self.value = value

        def apply(self, ds):
            """Apply dummy algorithm."""
            return ds + self.value

    class ParallelDummyAlgorithm(Algorithm):
        """test docstring"""

        def __init__(self, value, *args, **kwargs):
            self.value = value

        @parallelize
        def apply(self, ds):
            """Apply dummy algorithm."""
            return ds + self.value

    da = xr_lite.DataArray(np.random.default_rng(0).normal(size=(20, 20, 10)), ('y', 'x', 'time'), name='v')
    wrapper = wrap_algorithm(DummyAlgorithm, 'wrapper_name')
    assert DummyAlgorithm(0.1).apply(da).equals(wrapper(da, 0.1))
    assert wrapper.__name__ == 'wrapper_name'
    assert wrapper.__doc__ == ('Wrapper for :class:`%s.DummyAlgorithm`.\n\n' % DummyAlgorithm.__module__
                               + DummyAlgorithm.__doc__)
    assert list(inspect.signature(wrapper).parameters) == ['ds', 'value', 'args', 'kwargs']

    class MissingApply(Algorithm):
        def __init__(self):
            pass
    with pytest.raises(TypeError, match='abstract'):
        MissingApply()
    with pytest.raises(ValueError):
        wrap_algorithm(int)

    algo = ParallelDummyAlgorithm(3)
    ref = algo.apply(da)
    for njobs in (-1, 1, 2):
        assert ref.equals(algo.apply(da, njobs=njobs))
    assert 'njobs' in inspect.signature(ParallelDummyAlgorithm.apply).parameters


def test_split_merge_roundtrip():
    """xr_split / xr_merge halo arithmetic (nd/utils.py:288-340, nd/tests/test_utils.py:139-147)."""
    from nd_amd import _adapter
    ds = synth.lite_test_dataset()
    for chunks, buffer in [(2, 0), (3, 2), (4, 1), (7, 2)]:
        parts = list(_adapter.xr_split(ds, 'y', chunks, buffer))
        assert len(parts) == chunks
        merged = _adapter.xr_merge(parts, 'y', buffer)
        assert merged.equals(ds)
    assert _adapter.split_bounds(20, 3, 2) == [(0, 9), (5, 16), (12, 20)]


def test_filter_host_attributes():
    from nd_amd.filters import BoxcarFilter, ConvolutionFilter, GaussianFilter, NLMeansFilter
    b = BoxcarFilter(dims=('y', 'x'), w=5)
    assert b.kernel.shape == (5, 5) and b.kernel.dtype == np.float64 and b.kernel[0, 0] == 1 / 25
    assert b._buffer('y') == 2 and b._buffer('time') == 0
    ds = synth.lite_test_dataset(dims=OrderedDict([('y', 20), ('x', 30), ('time', 10)]))
    assert b._parallel_dimension(ds) == 'time'
    assert ConvolutionFilter(dims=('y', 'x', 'time'))._parallel_dimension(ds) == 'x'
    n = NLMeansFilter(dims=('time', 'y', 'x'), r=(0, 3, 3), f=1)
    assert list(n.r) == [0, 3, 3] and list(n.f) == [0, 1, 1]
    assert n._buffer('y') == 4 and n._buffer('time') == 0
    assert GaussianFilter(sigma=1.5)._buffer('x') == 6
    with pytest.raises(ValueError):
        NLMeansFilter(patch_distances='other')


def test_change_summaries():
    from nd_amd import xr_lite
    from nd_amd.change import change_count, first_change
    ch = np.zeros((2, 3, 5), bool)
    ch[0, 0, 2] = ch[0, 0, 4] = ch[1, 2, 1] = True
    da = xr_lite.DataArray(ch, ('y', 'x', 'time'), name='change')
    np.testing.assert_array_equal(change_count(da).values, ch.sum(axis=2))
    fc = first_change(da).values
    assert fc[0, 0] == 2 and fc[1, 2] == 1 and fc[0, 1] == -1
    assert change_count(da).dims == ('y', 'x')


def test_layout_recognition_helpers():
    """Pure stride logic of the transpose / pixel-major wrappers (no GPU needed)."""
    import torch
    from nd_amd import kernels
    t = torch.zeros((3, 5, 7))
    assert kernels._pixel_major_stride(t) == 1
    c = torch.zeros((3, 5, 7), dtype=torch.complex64)
    assert kernels._pixel_major_stride(c.real) == 2 and kernels._pixel_major_stride(c.imag) == 2
    assert kernels._pixel_major_stride(t.permute(1, 0, 2)) is None
    assert kernels._pixel_major_stride(t[:, ::2]) is None
    assert kernels._pixel_major_stride(torch.zeros((1, 1, 24))) == 1           # length-1 axes
    assert kernels._pixel_major_stride(torch.zeros((1, 4, 1))) == 1
    p = torch.zeros((7, 3, 5))
    assert kernels._planar_ok(p, 3, 5)
    assert kernels._planar_ok(torch.zeros((7, 20))[:, :15].view(7, 3, 5), 3, 5)    # padded planes
    assert not kernels._planar_ok(p.permute(0, 2, 1), 5, 3)
    # CPU tensors are declined by the wrappers themselves
    assert kernels.relayout_planar(t, p) is False
    assert kernels.change_detection_pixel_major(t, t, t, t, alpha=0.9) is None


def test_overlap_test_of_the_filter_wrappers():
    """kernels._may_overlap: conservative address-range test behind `out` aliasing `inp`."""
    import torch
    from nd_amd import kernels
    a = torch.zeros((4, 10, 12))
    assert kernels._may_overlap(a, a)
    assert kernels._may_overlap(a[1:], a[:2])
    assert not kernels._may_overlap(a[:2], a[2:])
    assert not kernels._may_overlap(a, torch.zeros_like(a))
    assert kernels._may_overlap(a[:, :, :6], a[:, :, 6:])        # interleaved columns: ranges intersect
    assert not kernels._may_overlap(a[:0], a)
    z = torch.zeros((5, 7), dtype=torch.complex64)
    assert kernels._may_overlap(z.real, z.imag)
    # the packed-split helpers decline anything that is not a CUDA tensor pair
    assert kernels.split_complex(z.real, z.imag) is None
    assert kernels.merge_complex(torch.zeros((5, 7)), torch.zeros((5, 7)), z) is False


def test_chunk_count_never_drops_rows():
    """xr_split / xr_merge lose rows when the last chunk is empty or shorter than the halo (n = 16,
    chunks = 5, halo = 1 merged to 15 rows: round-2 advisor finding); safe_chunks lowers the count
    until nothing is lost, and `parallel` checks the merged size."""
    from nd_amd import _adapter, xr_lite
    from nd_amd.algorithm import parallel
    assert _adapter.safe_chunks(16, 5, 1) == 4
    assert _adapter.safe_chunks(100, 16, 0) == 15          # ceil(100 / 16) = 7 -> 15 chunks, none empty
    assert _adapter.safe_chunks(10, 4, 3) == 2
    assert _adapter.safe_chunks(5, 1, 2) == 1
    for n in range(1, 60):
        for chunks in (1, 2, 3, 5, 8, 16):
            for halo in (0, 1, 2, 4):
                c = _adapter.safe_chunks(n, chunks, halo)
                assert 1 <= c <= chunks
                ds = xr_lite.Dataset(coords={'y': np.arange(n)})
                ds['a'] = (('y', 'x'), np.arange(n * 3, dtype=np.float32).reshape(n, 3))
                out = parallel(lambda part: part, dim='y', chunks=chunks, buffer=halo)(ds)
                np.testing.assert_array_equal(out['a'].values, ds['a'].values)


def test_integration_doc_quotes_the_example():
    """INTEGRATION.md's binding code IS examples/nd_binding.py: every marked section of the example
    appears verbatim in the document (tests/test_binding_example_gpu.py executes the example)."""
    import re
    ex = open(os.path.join(ROOT, 'examples', 'nd_binding.py')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    sections = dict(re.findall(r"# --8<-- \[(\w+)\]\n(.*?)\n# --8<-- \[end\]", ex, re.S))
    assert set(sections) == {'load', 'omnibus', 'omnibus_ml', 'convolve', 'nlmeans', 'gaussian'}
    for name, code in sections.items():
        assert code.strip('\n') in doc, 'INTEGRATION.md does not quote section [%s] verbatim' % name
    # the header says what the example does with the optional tile arguments
    hdr = open(os.path.join(ROOT, 'include', 'nd_amd.h')).read()
    assert 'NULL for any of the four' in hdr


def test_library_switches_are_the_documented_and_tested_ones():
    """The environment variables libnd_amd.so reads (every ND_AMD_* name handed to getenv / env_int / env_double under
    nd_amd/csrc) are exactly the rows of README.md's "Library switches" table, getenv is called nowhere but in the helper,
    and each switch is set by some test: a switch nothing forces is an experiment that is over and has to go."""
    csrc = os.path.join(ROOT, 'nd_amd', 'csrc')
    read, raw = set(), []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(('.hip', '.hpp')):
            continue
        text = open(os.path.join(csrc, f)).read()
        read |= set(re.findall(r'\b(?:getenv|env_int|env_double)\(\s*"(ND_AMD_[A-Z0-9_]+)"', text))
        raw += [(f, m.group(0)) for m in re.finditer(r'\bgetenv\([^)]*\)', text)]
    assert raw == [('common.hpp', 'getenv(name)')] * 2, raw           # env_int and env_double, nothing else
    readme = open(os.path.join(ROOT, 'README.md')).read()
    section = readme.split('### Library switches', 1)[1].split('\n## ', 1)[0]
    documented = re.findall(r'^\| `(ND_AMD_[A-Z0-9_]+)` \|', section, flags=re.M)
    assert len(documented) == len(set(documented))
    assert read == set(documented), (sorted(read - set(documented)), sorted(set(documented) - read))
    tests_dir = os.path.join(ROOT, 'tests')
    used = ''.join(open(os.path.join(tests_dir, f)).read() for f in sorted(os.listdir(tests_dir))
                   if f.endswith('.py') and f != os.path.basename(__file__))
    untested = sorted(n for n in read if not re.search(r'\b%s\b' % n, used))
    assert not untested, untested
