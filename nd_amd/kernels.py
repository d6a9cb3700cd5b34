"""
nd_amd/kernels.py -- tensor-level entry points: PyTorch-ROCm tensors in, HIP
kernels launched through the ctypes C ABI (include/nd_amd.h) on torch's current
stream.  PyTorch is only the device-memory / stream plumbing here.

Each function names the native call of the reference it stands in for:

  change_detection(...)      nd._change.change_detection          nd/_change.pyx:263-287
  change_detection_diag(...) the same for intensity-only stacks (extension, no reference counterpart)
  correlate_footprint(...)   scipy.ndimage.convolve               nd/filters.py:256-267
  pixelwise_nlmeans_3d(...)  nd._filters._pixelwise_nlmeans_3d    nd/_filters.pyx:320-420
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

_DT = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_cuda(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor, got %r' % (name, type(t)))
    if not t.is_cuda:
        raise ValueError('%s must live on a ROCm device (got %s); nd_amd has no CPU path'
                         % (name, t.device))
    if t.dtype not in _DT:
        raise TypeError('%s must be float32 or float64, got %s' % (name, t.dtype))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ---------------------------------------------------------------------------
# the checks and outputs the omnibus wrappers share
# ---------------------------------------------------------------------------
def _plane_stack(planes, what, names=None):
    """CUDA float tensors, 3-D, of one shape, dtype and device and with the same strides over the axes longer
    than 1 (strides of length-1 axes address nothing: views of one buffer may carry different ones);
    ValueError(what) otherwise.  Returns planes[0]."""
    p0 = planes[0]
    for i, t in enumerate(planes):
        _require_cuda(t, names[i] if names else 'planes[%d]' % i)
        if (t.dim() != 3 or t.shape != p0.shape or t.dtype != p0.dtype or t.device != p0.device
                or any(a != b for a, b, n_ in zip(t.stride(), p0.stride(), t.shape) if n_ > 1)):
            raise ValueError(what)
    return p0


def _yxt(dims, p0):
    """(ny, nx, k, sy, sx, st) of the plane p0 whose axes `dims` names."""
    dims = tuple(dims)
    if sorted(dims) != ['time', 'x', 'y']:
        raise ValueError("dims must be a permutation of ('time', 'y', 'x')")
    ay, ax, at = dims.index('y'), dims.index('x'), dims.index('time')
    return (p0.shape[ay], p0.shape[ax], p0.shape[at], p0.stride(ay), p0.stride(ax), p0.stride(at))


def _omnibus_outputs(ny, nx, k, dtype, dev, stats):
    """change (y, x, time) and, with stats, z and P (y, x) -- else None, None."""
    change = torch.empty((ny, nx, k), dtype=torch.uint8, device=dev)
    z = torch.empty((ny, nx), dtype=dtype, device=dev) if stats else None
    P = torch.empty((ny, nx), dtype=dtype, device=dev) if stats else None
    return change, z, P


def _omnibus_run(shape, dtype, dev, stats, nbytes, entry, *head):
    """The tail the omnibus wrappers share.  On `dev`: the outputs of a (ny, nx, k) raster, a workspace of
    `nbytes` bytes, entry(*head, change, z, P, workspace, nbytes, stream) -- every omnibus entry ends in these six
    arguments -- and the workspace kept alive until the stream has consumed it.  nbytes = None (the wrapper's word for
    an empty raster; a size of 0 is not: that call is made and refused): the empty outputs and no call.  Returns
    the library's code, which the wrapper judges, and change, or (change, z, P) with stats."""
    with torch.cuda.device(dev):
        change, z, P = _omnibus_outputs(*shape, dtype, dev, stats)
        rc = _lib.OK
        if nbytes is not None:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = entry(*head, _ptr(change), _ptr(z), _ptr(P), _ptr(ws), nbytes, _stream_ptr(dev))
            if rc == _lib.OK:
                ws.record_stream(torch.cuda.current_stream(dev))
    return rc, ((change, z, P) if stats else change)


def _pixel_major_ids(planes):
    """_pixel_major_stride of every plane, or None unless all share shape, dtype and device and have one."""
    p0 = planes[0]
    ids = []
    for t in planes:
        if t.shape != p0.shape or t.dtype != p0.dtype or t.device != p0.device:
            return None
        ids.append(_pixel_major_stride(t))
        if ids[-1] is None:
            return None
    return ids


# ---------------------------------------------------------------------------
# OmnibusTest C2
# ---------------------------------------------------------------------------
def change_detection(c11, c12re, c12im, c22, alpha, n=1, dims=('time', 'y', 'x'),
                     stats=False, workspace='recommended'):
    """Omnibus change detection on four covariance planes.

    c11, c12re, c12im, c22 : CUDA tensors of identical shape/strides/dtype whose
        three axes are named by `dims` (any order of 'y', 'x', 'time'); the
        reference's (y, x, time, 4) view (nd/change.py:66-67) is these four
        tensors side by side.
    workspace : 'recommended' (room for the series of 1/8 of the pixels, so the change-point
        search never re-reads the planes) or 'minimal' (candidate list only: less memory, listed
        pixels are gathered from the planes).
    Returns uint8 tensor (y, x, time) [, z (y, x), P (y, x)].
    """
    _plane_stack((c11, c12re, c12im, c22),
                 'the four covariance planes must be 3-D and share shape, strides, dtype and device',
                 names=('c11', 'c12re', 'c12im', 'c22'))
    ny, nx, k, sy, sx, st = _yxt(dims, c11)
    dev = c11.device
    L = _lib.lib()
    nbytes = None
    if ny * nx * k > 0:                     # (an empty raster: empty outputs, no call)
        min_bytes = C.c_size_t(0)
        nbytes = L.nd_amd_omnibus_c2_workspace_bytes(_DT[c11.dtype], ny, nx, k, C.byref(min_bytes))
        if workspace == 'minimal':
            nbytes = min_bytes.value
        elif workspace != 'recommended':
            raise ValueError("workspace must be 'recommended' or 'minimal'")
    rc, out = _omnibus_run((ny, nx, k), c11.dtype, dev, stats, nbytes, L.nd_amd_omnibus_c2,
                           _ptr(c11), _ptr(c12re), _ptr(c12im), _ptr(c22), _DT[c11.dtype], ny, nx, k, sy, sx, st,
                           int(n), float(alpha))
    _lib.check(rc)
    return out


def change_detection_multilooked(c11, c12re, c12im, c22, alpha, ml, stats=False):
    """OmnibusTest(ml=w) in one pass over four planar (time, y, x) device planes: boxcar multilooking
    (scipy's arithmetic, 'reflect' border) fused into the test, n = ml ** 2 looks (nd/change.py:61-69).
    Returns None where the fused kernel does not apply (the caller multilooks the stack and uses
    change_detection); otherwise the uint8 map (y, x, time) [, z, P]."""
    planes = (c11, c12re, c12im, c22)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dim() == 3 for t in planes):
        return None
    if c11.dtype != torch.float32 or int(ml) != ml:
        return None
    for t in planes:
        if t.shape != c11.shape or t.stride() != c11.stride() or t.dtype != c11.dtype or t.device != c11.device:
            return None
    k, ny, nx = c11.shape
    st, sy, sx = c11.stride()
    dev = c11.device
    L = _lib.lib()
    nbytes = L.nd_amd_omnibus_c2_ml_workspace_bytes(_lib.F32, ny, nx, k, int(ml)) if ny * nx * k > 0 else 0
    if nbytes == 0 or sx != 1:
        return None
    with torch.cuda.device(dev):
        change, z, P = _omnibus_outputs(ny, nx, k, c11.dtype, dev, stats)
        # The dump of the fused path has a slot for every pixel of the raster (the multilooked series exists
        # nowhere else), about the size of the input, of which only the listed part is ever touched.  torch's
        # caching allocator hands the same block back from call to call; where the memory is not there the
        # caller takes the two-step path (boxcar kernel, then the plain test), which needs none.
        try:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        except torch.cuda.OutOfMemoryError:
            return None
        rc = L.nd_amd_omnibus_c2_ml(_ptr(c11), _ptr(c12re), _ptr(c12im), _ptr(c22), _lib.F32, ny, nx, k,
                                    sy, sx, st, int(ml), float(alpha), _ptr(change), _ptr(z), _ptr(P),
                                    _ptr(ws), nbytes, _stream_ptr(dev))
        if rc == _lib.EUNSUPPORTED:
            return None
        _lib.check(rc)
        ws.record_stream(torch.cuda.current_stream(dev))
    return (change, z, P) if stats else change


def change_detection_pixel_major(c11, c12re, c12im, c22, alpha, n=1, stats=False):
    """change_detection for four device variables in the reference's own layout, (y, x, time) with
    time fastest; `c12re` / `c12im` may be the `.real` / `.imag` views of one complex tensor (read
    once).  Returns None when the layout or the series length is not one the pixel-major kernel
    takes (the caller then transposes and uses change_detection)."""
    vs = (c11, c12re, c12im, c22)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dim() == 3 for t in vs):
        return None
    ny, nx, k = c11.shape
    dt = c11.dtype
    if dt not in _DT or k > 192 or ny * nx * k == 0:
        return None
    # beyond the register-retaining sizes the kernel takes the sparse regime only (include/nd_amd.h)
    long_series = k > (24 if dt == torch.float32 else 12)
    ids = _pixel_major_ids(vs)
    if ids is None:
        return None
    # The date strides come from the tensors' own strides only.  (Two views one element apart are
    # NOT proof of an interleaved complex tensor: buf[:-1] and buf[1:] of a real buffer look the
    # same.  The library pairs the two C12 reads itself when both strides are 2 and the pointers
    # are adjacent.)
    if ids[1] != ids[2]:
        return None
    dev = c11.device
    L = _lib.lib()
    rc, out = _omnibus_run((ny, nx, k), dt, dev, stats, L.nd_amd_omnibus_c2_workspace_bytes(_DT[dt], ny, nx, k, None),
                           L.nd_amd_omnibus_c2_pixel_major, _ptr(c11), _ptr(c12re), _ptr(c12im), _ptr(c22), _DT[dt],
                           ny, nx, k, _lib.i64_array(ids), int(n), float(alpha))
    if long_series and rc == _lib.EUNSUPPORTED:
        return None                   # the caller transposes and takes the planar path
    _lib.check(rc)
    return out


def change_detection_c3(planes, alpha, n=1, dims=('time', 'y', 'x'), stats=False):
    """Full-pol (3 x 3) omnibus change detection -- an extension, the reference is dual-pol only.
    planes: nine CUDA tensors [C11, C22, C33, C12re, C12im, C13re, C13im, C23re, C23im] of
    identical shape/strides/dtype, axes named by `dims`.  Returns uint8 (y, x, time) [, z, P]."""
    planes = list(planes)
    if len(planes) != 9:
        raise ValueError('full-pol covariance needs nine real planes')
    p0 = _plane_stack(planes, 'the nine covariance planes must be 3-D and share shape, strides, dtype and device')
    ny, nx, k, sy, sx, st = _yxt(dims, p0)
    dev = p0.device
    L = _lib.lib()
    # (an empty raster: empty outputs, no call)
    nbytes = L.nd_amd_omnibus_c3_workspace_bytes(ny, nx, k) if ny * nx * k > 0 else None
    ptrs = (C.c_void_p * 9)(*[t.data_ptr() for t in planes])
    rc, out = _omnibus_run((ny, nx, k), p0.dtype, dev, stats, nbytes, L.nd_amd_omnibus_c3,
                           ptrs, _DT[p0.dtype], ny, nx, k, sy, sx, st, int(n), float(alpha))
    _lib.check(rc)
    return out


def change_detection_diag(planes, alpha, n=1, dims=('time', 'y', 'x'), stats=False):
    """Omnibus change detection on intensity-only stacks -- an extension: the block-diagonal case of the
    test, q independent 1 x 1 blocks.  planes: one to three real CUDA tensors (e.g. [VV, VH]) of identical
    shape/strides/dtype, axes named by `dims`; n: the (equivalent) number of looks, any positive real.
    Returns uint8 (y, x, time) [, z, P]."""
    planes = list(planes)
    if not 1 <= len(planes) <= 3:
        raise ValueError('the intensity-only test takes one to three channels, got %d' % len(planes))
    p0 = _plane_stack(planes, 'the intensity planes must be 3-D and share shape, strides, dtype and device')
    ny, nx, k, sy, sx, st = _yxt(dims, p0)
    dev = p0.device
    L = _lib.lib()
    # (an empty raster: empty outputs, no call)
    nbytes = L.nd_amd_omnibus_diag_workspace_bytes(_DT[p0.dtype], len(planes), ny, nx, k) if ny * nx * k > 0 else None
    ptrs = (C.c_void_p * len(planes))(*[t.data_ptr() for t in planes])
    rc, out = _omnibus_run((ny, nx, k), p0.dtype, dev, stats, nbytes, L.nd_amd_omnibus_diag,
                           ptrs, len(planes), _DT[p0.dtype], ny, nx, k, sy, sx, st, float(n), float(alpha))
    _lib.check(rc)
    return out


_STRUCTURES = {'diag': (_lib.STRUCT_DIAG, (1, 2, 3)), 'c2': (_lib.STRUCT_C2, (4,)), 'c3': (_lib.STRUCT_C3, (9,))}


def change_segments(planes, change, structure, dims=('time', 'y', 'x'), direction=True, means=True):
    """Direction of every declared change and the segment means -- an extension (include/nd_amd.h has the
    definition).  planes: the real CUDA tensors an omnibus entry reads, in its order -- structure 'diag': one
    to three intensities, 'c2': [C11, C12re, C12im, C22], 'c3': the nine planes of change_detection_c3 -- of
    identical shape/strides/dtype, axes named by `dims`.  change: the contiguous uint8 or bool CUDA tensor
    (y, x, time) an omnibus entry returns.
    Returns direction, int8 (y, x, time): 0 no change declared, 1 / 2 / 3 the difference between the new date
    and the mean of the segment before it is positive definite / negative definite / neither; and / or means:
    a list of planes shaped and strided like `planes`, every date replaced by the mean of its segment."""
    planes = list(planes)
    if structure not in _STRUCTURES:
        raise ValueError("structure must be 'diag', 'c2' or 'c3', got %r" % (structure,))
    code, counts = _STRUCTURES[structure]
    if len(planes) not in counts:
        raise ValueError("structure '%s' takes %s planes, got %d"
                         % (structure, {'diag': 'one to three', 'c2': 'four', 'c3': 'nine'}[structure], len(planes)))
    if not (direction or means):
        raise ValueError('change_segments: neither direction nor means is asked for')
    p0 = _plane_stack(planes, 'the planes must be 3-D and share shape, strides, dtype and device')
    if any(st_ == 0 and n_ > 1 for st_, n_ in zip(p0.stride(), p0.shape)):
        raise ValueError('expanded planes (stride 0) are not served: the means would overlap')
    ny, nx, k, sy, sx, st = _yxt(dims, p0)
    if not isinstance(change, torch.Tensor):
        raise TypeError('change must be a torch.Tensor, got %r' % type(change))
    if change.dtype not in (torch.uint8, torch.bool):
        raise TypeError('change must be uint8 or bool, got %s' % change.dtype)
    if tuple(change.shape) != (ny, nx, k):
        raise ValueError('change has shape %s, the planes are (y, x, time) = %s'
                         % (tuple(change.shape), (ny, nx, k)))
    if change.device != p0.device:
        raise ValueError('change lives on %s, the planes on %s' % (change.device, p0.device))
    if not change.is_contiguous():
        raise ValueError('change must be contiguous (y, x, time)')
    dev = p0.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        out_d = torch.empty((ny, nx, k), dtype=torch.int8, device=dev) if direction else None
        # one allocation per plane with the planes' own strides (empty_strided: nothing is initialised)
        out_m = [torch.empty_strided(tuple(p0.shape), p0.stride(), dtype=p0.dtype, device=dev)
                 for _ in planes] if means else None
        if ny * nx * k > 0:
            ptrs = (C.c_void_p * len(planes))(*[t.data_ptr() for t in planes])
            mptrs = (C.c_void_p * len(planes))(*[t.data_ptr() for t in out_m]) if means else None
            cbytes = change.view(torch.uint8) if change.dtype == torch.bool else change
            _lib.check(L.nd_amd_change_segments(
                ptrs, len(planes), code, _DT[p0.dtype], ny, nx, k, sy, sx, st,
                _ptr(cbytes), _ptr(out_d), mptrs, _stream_ptr(dev)))
    if direction and means:
        return out_d, out_m
    return out_d if direction else out_m


def change_detection_c3_pixel_major(planes, alpha, n=1, stats=False):
    """change_detection_c3 for nine device variables in the reference's own layout, (y, x, time) with time
    fastest -- [C11, C22, C33, C12re, C12im, C13re, C13im, C23re, C23im], the off-diagonal pairs either real
    arrays or the `.real` / `.imag` views of complex tensors (read once).  Returns None where the kernel
    does not apply (other layouts, series lengths, thresholds below the sparse regime): the caller then
    transposes and uses change_detection_c3."""
    planes = list(planes)
    if len(planes) != 9 or not all(torch.is_tensor(t) and t.is_cuda and t.dim() == 3 for t in planes):
        return None
    p0 = planes[0]
    ny, nx, k = p0.shape
    dt = p0.dtype
    if dt not in _DT or ny * nx * k == 0:
        return None
    ids = _pixel_major_ids(planes)
    if ids is None:
        return None
    # the entry point's documented conditions (include/nd_amd.h), checked before anything is allocated: with the
    # reference's default alpha = 0.01 every full-pol (y, x, time) call would otherwise allocate the map and the
    # workspace only to learn that it is declined.  (0.75 is the entry point's fixed switch-over to the fused search,
    # `fused_alpha` in omnibus_c3.hip: no environment variable moves it.)
    ve = 16 // p0.element_size()
    if (not (alpha >= 0.75) or k % ve != 0 or 16 * 9 * k * p0.element_size() > 56 * 1024
            or any(t.data_ptr() % 16 != 0 for t, i in zip(planes, ids) if i == 1)):
        return None
    dev = p0.device
    L = _lib.lib()
    ptrs = (C.c_void_p * 9)(*[t.data_ptr() for t in planes])
    rc, out = _omnibus_run((ny, nx, k), dt, dev, stats, L.nd_amd_omnibus_c3_workspace_bytes(ny, nx, k),
                           L.nd_amd_omnibus_c3_pixel_major, ptrs, _DT[dt], ny, nx, k, _lib.i64_array(ids), int(n),
                           float(alpha))
    if rc == _lib.EUNSUPPORTED:
        return None
    _lib.check(rc)
    return out


# ---------------------------------------------------------------------------
# layout change in front of the hot path
# ---------------------------------------------------------------------------
def _pixel_major_stride(t):
    """1 if the 3-D tensor `t` (y, x, time) is C-contiguous, 2 if it is one half of an interleaved
    complex tensor of that layout, else None.  Strides of length-1 axes carry no information."""
    ny, nx, k = t.shape
    for ids in (1, 2):
        want = (nx * k * ids, k * ids, ids)
        if all(n == 1 or s == w for n, s, w in zip(t.shape, t.stride(), want)):
            return ids
    return None


def _planar_ok(t, ny, nx):
    """(time, y, x) tensor with x contiguous, rows adjacent, any plane pitch >= ny * nx."""
    k = t.shape[0]
    return ((nx == 1 or t.stride(2) == 1) and (ny == 1 or t.stride(1) == nx)
            and (k == 1 or t.stride(0) >= ny * nx))


_RELAYOUT_LDS = 48 * 1024      # bytes of LDS one pixel's series may take in the transpose kernels


def relayout_planar(src, dst):
    """Copy a device variable laid out (y, x, time) with time fastest -- the reference's own
    layout -- into the planar (time, y, x) view `dst` (x fastest, any plane pitch).  `src` may be
    a real tensor, or the `.real` / `.imag` view of an interleaved complex tensor.  Returns False
    (nothing done) when the layouts are not of that form; the caller then copies through torch."""
    if not (torch.is_tensor(src) and src.is_cuda and src.dim() == 3 and dst.dim() == 3):
        return False
    ny, nx, k = src.shape
    if tuple(dst.shape) != (k, ny, nx) or src.dtype != dst.dtype or src.dtype not in _DT:
        return False
    if ny * nx * k == 0:
        return True
    ids = _pixel_major_stride(src)
    if ids is None or not _planar_ok(dst, ny, nx):
        return False
    if (k | 1) * src.element_size() > _RELAYOUT_LDS:        # series too long for the staging buffer
        return False
    dev = src.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nd_amd_relayout_planar(
            _ptr(src), _ptr(dst), _DT[src.dtype], ny * nx, k, ids, max(dst.stride(0), ny * nx),
            _stream_ptr(dev)))
    return True


def relayout_planar_complex(src_re, src_im, dst_re, dst_im):
    """relayout_planar for both halves of one interleaved complex (y, x, time) tensor at once
    (`src_re`, `src_im` = its `.real` / `.imag` views): the source is read once.  False when the two
    views are not the halves of one such tensor."""
    if not (torch.is_tensor(src_re) and torch.is_tensor(src_im) and src_re.is_cuda and src_re.dim() == 3):
        return False
    ny, nx, k = src_re.shape
    es = src_re.element_size()
    if (src_im.shape != src_re.shape or src_re.dtype not in _DT
            or src_im.dtype != src_re.dtype or src_im.data_ptr() != src_re.data_ptr() + es
            or _pixel_major_stride(src_re) is None or _pixel_major_stride(src_im) is None
            or (ny * nx * k > 1 and (_pixel_major_stride(src_re) != 2 or _pixel_major_stride(src_im) != 2))):
        return False
    if ((2 * k) | 1) * es > _RELAYOUT_LDS:
        return False
    for d in (dst_re, dst_im):
        if (tuple(d.shape) != (k, ny, nx) or d.dtype != src_re.dtype or not _planar_ok(d, ny, nx)
                or (k > 1 and d.stride(0) != dst_re.stride(0))):
            return False
    if ny * nx * k == 0:
        return True
    dev = src_re.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nd_amd_relayout_planar_complex(
            _ptr(src_re), _ptr(dst_re), _ptr(dst_im), _DT[src_re.dtype], ny * nx, k,
            max(dst_re.stride(0), ny * nx),
            _stream_ptr(dev)))
    return True


def split_complex(src_re, src_im):
    """The `.real` / `.imag` views of ONE contiguous complex CUDA tensor as two packed real tensors
    of the same shape, in one pass over its memory (nd_amd_split_complex).  None when the views
    are anything else (the caller then packs them one by one)."""
    if not (torch.is_tensor(src_re) and torch.is_tensor(src_im) and src_re.is_cuda
            and src_re.dtype in _DT and src_im.dtype == src_re.dtype and src_re.shape == src_im.shape
            and src_re.device == src_im.device and src_re.numel() > 0):
        return None
    es = src_re.element_size()
    if src_im.data_ptr() != src_re.data_ptr() + es or src_re.stride() != src_im.stride():
        return None
    # a contiguous complex tensor seen through a real view: every stride doubled, innermost 2
    want = []
    acc = 2
    for n_ in reversed(src_re.shape):
        want.append(acc)
        acc *= n_
    want = tuple(reversed(want))
    if any(s_ != w_ for s_, w_, n_ in zip(src_re.stride(), want, src_re.shape) if n_ > 1):
        return None
    if src_re.data_ptr() % 16:
        return None
    dev = src_re.device
    with torch.cuda.device(dev):
        re = torch.empty(src_re.shape, dtype=src_re.dtype, device=dev)
        im = torch.empty(src_re.shape, dtype=src_re.dtype, device=dev)
        _lib.check(_lib.lib().nd_amd_split_complex(_ptr(src_re), _ptr(re), _ptr(im), _DT[src_re.dtype],
                                                   src_re.numel(), _stream_ptr(dev)))
    return re, im


def merge_complex(re, im, out):
    """Two packed real CUDA tensors -> the contiguous complex tensor `out` of the same shape, one
    pass (nd_amd_merge_complex).  False when the tensors are not of that form."""
    if not (torch.is_tensor(out) and out.is_complex() and out.is_cuda and out.is_contiguous()
            and torch.is_tensor(re) and torch.is_tensor(im) and re.is_contiguous() and im.is_contiguous()
            and re.shape == out.shape and im.shape == out.shape and re.dtype in _DT and im.dtype == re.dtype
            and torch.view_as_real(out).dtype == re.dtype and re.device == out.device == im.device
            and out.numel() > 0):
        return False
    if (re.data_ptr() | im.data_ptr() | out.data_ptr()) % 16:
        return False
    dev = out.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nd_amd_merge_complex(_ptr(re), _ptr(im), _ptr(out), _DT[re.dtype],
                                                   re.numel(), _stream_ptr(dev)))
    return True


def relayout_pixel_major(src, dst):
    """Inverse of relayout_planar: planar (time, y, x) `src` (x fastest, any plane pitch) into
    `dst` laid out (y, x, time) with time fastest (a real tensor or one half of a complex one).
    Returns False when the layouts are not of that form."""
    if not (torch.is_tensor(dst) and dst.is_cuda and src.is_cuda and src.dim() == 3 and dst.dim() == 3):
        return False
    ny, nx, k = dst.shape
    if tuple(src.shape) != (k, ny, nx) or src.dtype != dst.dtype or src.dtype not in _DT:
        return False
    if ny * nx * k == 0:
        return True
    ods = _pixel_major_stride(dst)
    if ods is None or not _planar_ok(src, ny, nx):
        return False
    if (k | 1) * src.element_size() > _RELAYOUT_LDS:
        return False
    dev = src.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nd_amd_relayout_pixel_major(
            _ptr(src), _ptr(dst), _DT[src.dtype], ny * nx, k, max(src.stride(0), ny * nx), ods,
            _stream_ptr(dev)))
    return True


# ---------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------
def footprint(weights, origin=0, convolution=True):
    """scipy.ndimage `_correlate_or_convolve` footprint of a kernel: offsets
    (ntaps, ndim) int64 and weights (ntaps,) float64 of the taps NI_Correlate
    visits, in its order (|w| <= DBL_EPSILON dropped)."""
    weights = np.asarray(weights, dtype=np.float64)
    ndim = weights.ndim
    origins = [int(origin)] * ndim if np.isscalar(origin) else [int(o) for o in origin]
    if len(origins) != ndim:
        raise ValueError('origin must have one entry per kernel axis')
    if convolution:
        weights = weights[tuple([slice(None, None, -1)] * ndim)]
        for ii in range(ndim):
            origins[ii] = -origins[ii]
            if not weights.shape[ii] & 1:
                origins[ii] -= 1
    for o, lenw in zip(origins, weights.shape):
        if (lenw // 2 + o < 0) or (lenw // 2 + o >= lenw):
            raise ValueError('invalid origin')
    keep = np.abs(weights) > np.finfo(np.float64).eps
    idx = np.argwhere(keep)                                  # C order
    centre = np.array([weights.shape[d] // 2 + origins[d] for d in range(ndim)])
    offs = (idx - centre).astype(np.int64).reshape(-1, ndim)
    return offs, np.ascontiguousarray(weights[keep], np.float64)


def _may_overlap(a, b):
    """Conservative test: the address ranges the two tensors span intersect."""
    if a.device != b.device or a.numel() == 0 or b.numel() == 0:
        return False

    def span(t):
        lo = t.data_ptr()
        hi = lo + (sum((n - 1) * abs(st) for n, st in zip(t.shape, t.stride())) + 1) * t.element_size()
        return lo, hi
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def correlate_footprint(inp, out, offsets, weights, mode='reflect', cval=0.0):
    """out[i] = (T) sum_t weights[t] * inp[extend(i + offsets[t])], double
    accumulation in tap order.  inp/out: CUDA tensors, same shape, ndim <= 4."""
    _require_cuda(inp, 'inp')
    _require_cuda(out, 'out')
    if inp.shape != out.shape or inp.dtype != out.dtype or inp.device != out.device:
        raise ValueError('inp and out must share shape, dtype and device')
    if inp.dim() > 4:
        raise NotImplementedError('nd_amd_correlate handles up to 4 dimensions')
    if mode not in _lib.MODES:
        raise RuntimeError('boundary mode not supported')
    offsets = np.asarray(offsets, np.int64).reshape(-1, inp.dim())
    weights = np.ascontiguousarray(weights, np.float64)
    ntaps = len(weights)
    pad = 4 - inp.dim()
    dims = (1,) * pad + tuple(inp.shape)
    si = (0,) * pad + tuple(inp.stride())
    so = (0,) * pad + tuple(out.stride())
    offs4 = np.zeros((ntaps, 4), np.int64)
    offs4[:, pad:] = offsets
    dev = inp.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        taps_dev = None
        if ntaps > 128:
            taps_dev = torch.empty(24 * ntaps, dtype=torch.uint8, device=dev)
        _lib.check(L.nd_amd_correlate(
            _ptr(inp), _ptr(out), _DT[inp.dtype], _lib.i64_array(dims), _lib.i64_array(si),
            _lib.i64_array(so), ntaps,
            offs4.ctypes.data_as(C.POINTER(C.c_int64)),
            weights.ctypes.data_as(C.POINTER(C.c_double)),
            _lib.MODES[mode], float(cval), _ptr(taps_dev),
            0 if taps_dev is None else taps_dev.numel(), _stream_ptr(dev)))
    return out


def convolve(inp, kernel, out=None, mode='reflect', cval=0.0, origin=0):
    """scipy.ndimage.convolve(inp, kernel, output=out, mode, cval, origin) on a
    real CUDA tensor; kernel.ndim must equal inp.dim().

    A window over the last three axes of an x-contiguous array runs in the LDS-tiled kernel where the
    array lies.  When the array is laid out differently -- the reference's datasets are (y, x, time)
    with time fastest -- it is transposed on the device first and the result transposed back; the tap
    order over the window axes, hence the result, is unchanged.
    """
    kernel = np.asarray(kernel, np.float64)
    if kernel.ndim != inp.dim():
        raise RuntimeError('filter weights array has incorrect shape.')
    if out is None:
        out = torch.empty_like(inp)
    elif _may_overlap(inp, out):
        # scipy filters into a temporary when input and output share memory; the kernels read
        # neighbours of what they write
        out.copy_(convolve(inp, kernel, None, mode, cval, origin))
        return out
    nd = inp.dim()
    span = [d for d in range(nd) if kernel.shape[d] > 1]
    tail = list(range(nd - len(span), nd))
    # (round 5) the tiled kernel walks windows over the last THREE axes of x-contiguous arrays where they
    # lie -- (time, y, x) kernels, and windows along time or y alone, which used to be transposed to the
    # back first (a 3 x 1 x 1 window on 8 x 2048^2: 0.95 ms of transposes around 0.08 ms of filtering).  The
    # reference's (y, x, time) layout with a (y, x) window keeps its transpose kernels: its last axis is the
    # short one.
    # (only where the LAST axis is long -- it is the tiles' x axis; on time-fastest data, (y, x, time)
    # or (var, y, x, time) with a window over y and / or x, wide tiles would idle over a short time axis)
    in_place = (inp.stride(-1) == 1 and out.stride(-1) == 1 and all(d >= nd - 3 for d in span)
                and not (nd == 3 and span == [0, 1]) and inp.shape[-1] >= 64)
    if (0 < len(span) <= 2 and nd <= 4 and not in_place
            and (span != tail or inp.stride(-1) != 1 or out.stride(-1) != 1)
            and inp.numel() >= (1 << 16)):
        perm = [d for d in range(nd) if d not in span] + span
        origins = [int(origin)] * nd if np.isscalar(origin) else [int(o) for o in origin]
        k = np.transpose(kernel, perm)
        offs, w = footprint(k, [origins[d] for d in perm], convolution=True)
        # the reference's (y, x, time) layout with a (y, x) window: dedicated transpose kernels
        t = None
        if nd == 3 and span == [0, 1]:
            t = torch.empty((inp.shape[2], inp.shape[0], inp.shape[1]), dtype=inp.dtype, device=inp.device)
            if not relayout_planar(inp, t):
                t = None
        if t is None:
            t = inp.permute(*perm).contiguous()
        o = torch.empty_like(t)
        correlate_footprint(t, o, offs, w, mode, cval)
        if not (nd == 3 and span == [0, 1] and relayout_pixel_major(o, out)):
            inv = [perm.index(d) for d in range(nd)]
            out.copy_(o.permute(*inv))
        return out
    offs, w = footprint(kernel, origin, convolution=True)
    return correlate_footprint(inp, out, offs, w, mode, cval)


def correlate1d(inp, weights, axis, out, mode='reflect', cval=0.0):
    """scipy.ndimage.correlate1d(inp, weights, axis, out, mode, cval, origin=0) on a real CUDA
    tensor (ndim <= 4); `out` must not alias `inp`."""
    _require_cuda(inp, 'inp')
    _require_cuda(out, 'out')
    if inp.shape != out.shape or inp.dtype != out.dtype or inp.device != out.device:
        raise ValueError('inp and out must share shape, dtype and device')
    if inp.dim() > 4:
        raise NotImplementedError('nd_amd_correlate1d handles up to 4 dimensions')
    if mode not in _lib.MODES:
        raise RuntimeError('boundary mode not supported')
    weights = np.ascontiguousarray(weights, np.float64)
    pad = 4 - inp.dim()
    axis = axis % inp.dim()
    dev = inp.device
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nd_amd_correlate1d(
            _ptr(inp), _ptr(out), _DT[inp.dtype], _lib.i64_array((1,) * pad + tuple(inp.shape)),
            _lib.i64_array((0,) * pad + tuple(inp.stride())),
            _lib.i64_array((0,) * pad + tuple(out.stride())), axis + pad, len(weights),
            weights.ctypes.data_as(C.POINTER(C.c_double)), _lib.MODES[mode], float(cval),
            _stream_ptr(dev)))
    return out


def _gaussian_kernel1d(sigma, radius):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, order=0, radius)."""
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


def _gaussian_yx_fused(inp, out, axes, nd, mode, truncate):
    """The common GaussianFilter(dims=('y', 'x')) case on x-contiguous float32 / float64 planes: both
    passes in one kernel (nd_amd_correlate1d_yx), the intermediate in the array dtype like scipy's.
    Returns False when the request is not one the fused kernel takes."""
    if (len(axes) != 2 or [ax for ax, _ in axes] != [nd - 2, nd - 1] or nd > 4
            or inp.dtype not in (torch.float32, torch.float64) or mode not in _lib.MODES or mode == 'constant'
            or inp.stride(-1) != 1 or out.stride(-1) != 1 or inp.data_ptr() == out.data_ptr()
            or inp.shape != out.shape or inp.device != out.device):
        return False
    lws = [int(truncate * sd + 0.5) for _, sd in axes]
    if lws[0] != lws[1] or lws[0] < 1:
        return False
    wy, wx = (np.ascontiguousarray(_gaussian_kernel1d(sd, lw)[::-1], np.float64)
              for (_, sd), lw in zip(axes, lws))
    pad = 4 - nd
    dev = inp.device
    with torch.cuda.device(dev):
        rc = _lib.lib().nd_amd_correlate1d_yx(
            _ptr(inp), _ptr(out), _DT[inp.dtype], _lib.i64_array((1,) * pad + tuple(inp.shape)),
            _lib.i64_array((0,) * pad + tuple(inp.stride())),
            _lib.i64_array((0,) * pad + tuple(out.stride())), len(wy),
            wy.ctypes.data_as(C.POINTER(C.c_double)), wx.ctypes.data_as(C.POINTER(C.c_double)),
            _lib.MODES[mode], _stream_ptr(dev))
    if rc == _lib.EUNSUPPORTED:
        return False
    _lib.check(rc)
    return True


def gaussian_filter(inp, sigma, out=None, mode='reflect', cval=0.0, truncate=4.0):
    """scipy.ndimage.gaussian_filter(inp, sigma, output=out, mode, cval, truncate): one
    correlate1d pass per axis with sigma > 1e-15, each pass reading the previous pass's result
    in the array dtype (scipy filters `output` in place from the second axis on)."""
    if out is None:
        out = torch.empty_like(inp)
    elif _may_overlap(inp, out):
        out.copy_(gaussian_filter(inp, sigma, None, mode, cval, truncate))
        return out
    nd = inp.dim()
    sigmas = [float(sigma)] * nd if np.isscalar(sigma) else [float(s) for s in sigma]
    if len(sigmas) != nd:
        raise RuntimeError('sequence argument must have length equal to input rank')
    axes = [(ax, sd) for ax, sd in enumerate(sigmas) if sd > 1e-15]
    if not axes:
        out.copy_(inp)
        return out
    # The real / imaginary halves of a complex variable (and other views whose last axis is not
    # contiguous) would run in the per-element kernel: one packed copy in, one strided copy out
    # is cheaper by far (GaussianFilter on a (time, y, x) dataset with a complex64 C12: 6.8 -> 3.9 ms).
    if nd >= 1 and inp.numel() >= (1 << 16) and (inp.stride(-1) != 1 or out.stride(-1) != 1):
        packed = gaussian_filter(inp.contiguous(), sigma, None, mode, cval, truncate)
        out.copy_(packed)
        return out
    src = inp
    bufs = [out, None]
    if _gaussian_yx_fused(inp, out, axes, nd, mode, truncate):
        return out
    for n_done, (ax, sd) in enumerate(axes):
        lw = int(truncate * sd + 0.5)
        weights = _gaussian_kernel1d(sd, lw)[::-1]
        # the last pass must land in `out`; alternate between `out` and one scratch tensor
        remaining = len(axes) - n_done
        dst = out if remaining % 2 == 1 else None
        if dst is None:
            if bufs[1] is None:
                bufs[1] = torch.empty_like(out)
            dst = bufs[1]
        correlate1d(src, weights, ax, dst, mode, cval)
        src = dst
    return out


# ---------------------------------------------------------------------------
# non-local means
# ---------------------------------------------------------------------------
def raise_if_no_solution(status):
    """The deferred half of pixelwise_nlmeans_3d(..., status=t): reads the device flag (this is the
    host synchronisation) and raises the reference's ValueError('No solution') if it is set."""
    if status is not None and int(status.item()) != 0:
        raise ValueError('No solution')


def pixelwise_nlmeans_3d(arr, output, r, f, sigma, h, n_eff=-1, patch_mode=0,
                         neff_policy=1, global_shape=None, tile_offset=None,
                         core=None, status=None):
    """In-place into `output` like the reference.  arr/output: CUDA tensors
    (N0, N1, N2, nvars), any strides.

    patch_mode 0 = bit-compatible with the compiled reference (LP64: patch
    loops empty when any f > 0); 1 = true patch distances.
    neff_policy 1 raises ValueError('No solution') like a current build of the
    reference, 0 gives the self weight 0 of the shipped C.
    global_shape/tile_offset/core describe a halo-carrying tile (multi-GPU).
    status: an int32 device tensor of one element.  Without it (the reference's behaviour) a call
    with n_eff >= 0 reads the find_weight flag back and raises at once -- one host
    synchronisation per call.  With it the library writes the flag there (zeroing it first) and
    the call stays asynchronous: a pipeline step then has no host stall, and the caller checks
    with raise_if_no_solution(status) when it next needs the host anyway.
    """
    _require_cuda(arr, 'arr')
    _require_cuda(output, 'output')
    if arr.dim() != 4 or output.shape != arr.shape or output.dtype != arr.dtype:
        raise ValueError('arr and output must be 4-D (N0, N1, N2, nvars) and alike')
    r = [int(v) for v in r]
    f = [int(v) for v in f]
    if len(r) != 3 or len(f) != 3:
        raise ValueError('r and f must have three entries')
    N = tuple(arr.shape[:3])
    G = tuple(global_shape) if global_shape is not None else N
    toff = tuple(tile_offset) if tile_offset is not None else (0, 0, 0)
    clo = tuple(c[0] for c in core) if core is not None else (0, 0, 0)
    chi = tuple(c[1] for c in core) if core is not None else N
    dev = arr.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        deferred = status is not None
        if deferred and (status.dtype != torch.int32 or status.numel() != 1 or status.device != dev):
            raise ValueError('status must be one int32 element on the device of arr')
        if not deferred and n_eff >= 0 and neff_policy == 1:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.nd_amd_nlmeans3d(
            _ptr(arr), _ptr(output), _DT[arr.dtype], _lib.i64_array(N), arr.shape[3],
            _lib.i64_array(arr.stride()), _lib.i64_array(output.stride()),
            _lib.u32_array(r), _lib.u32_array(f), float(sigma), float(h), float(n_eff),
            int(patch_mode), int(neff_policy), _ptr(status),
            _lib.i64_array(G), _lib.i64_array(toff), _lib.i64_array(clo),
            _lib.i64_array(chi), _stream_ptr(dev)))
        if not deferred:
            raise_if_no_solution(status)
    return output


# ---------------------------------------------------------------------------
# Coregistration (nd/warp.py:1104-1163)
# ---------------------------------------------------------------------------
def coregister_shifts(c11, reference=0, upsampling=10, dims=('time', 'y', 'x')):
    """Shift of every date of the C11 stack against date `reference`, as
    skimage.registration.phase_cross_correlation(C11[t], C11[reference], upsample_factor=upsampling)
    (scikit-image 0.18) computes it: (row, col) in the order the two spatial axes of `dims` are stored.
    Returns device tensors (shifts float64 (k, 2), status int32 (k,)); status[t] = 1 where skimage
    raises ValueError (a NaN reached the correlation).  Nothing is synchronised."""
    _require_cuda(c11, 'c11')
    dims = tuple(dims)
    if c11.dim() != 3 or sorted(dims) != ['time', 'x', 'y']:
        raise ValueError("c11 must be 3-D with dims a permutation of ('time', 'y', 'x')")
    at = dims.index('time')
    ar, ac = [i for i in range(3) if i != at]
    k, nr, nc = c11.shape[at], c11.shape[ar], c11.shape[ac]
    ref = int(reference)
    if not 0 <= ref < k:
        raise IndexError('reference %d is out of bounds for %d dates' % (ref, k))
    dev = c11.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        shifts = torch.zeros((k, 2), dtype=torch.float64, device=dev)
        status = torch.zeros(k, dtype=torch.int32, device=dev)
        if k * nr * nc == 0:
            return shifts, status
        nbytes = L.nd_amd_coregister_shifts_workspace_bytes(_DT[c11.dtype], k, nr, nc, int(upsampling))
        if nbytes == 0:
            raise ValueError('coregister_shifts: unsupported shape %s or upsampling %r (1 .. 128)'
                             % (tuple(c11.shape), upsampling))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(L.nd_amd_coregister_shifts(
            _ptr(c11), _DT[c11.dtype], k, nr, nc, c11.stride(at), c11.stride(ar), c11.stride(ac), ref,
            int(upsampling), _ptr(shifts), _ptr(status), _ptr(ws), nbytes, _stream_ptr(dev)))
        ws.record_stream(torch.cuda.current_stream(dev))
    return shifts, status


def warp_translate(planes, shifts, reference=-1, layout='planar'):
    """Translate every date of each variable by its row of `shifts` (device float64 (k, 2)), as
    skimage.transform.warp(v[t], AffineTransform(translation=(s[t, 1], s[t, 0])), order=3) does
    (constant 0 outside, clipped to the plane's input range).  planes: device tensors of one dtype
    and shape, (k, rows, cols) for layout 'planar', (rows, cols, k) for 'pixel_major'; the date
    `reference` (-1: none) is copied.  Returns new tensors; the inputs are never written."""
    planes = list(planes)
    if not planes:
        return []
    p0 = planes[0]
    for i, t in enumerate(planes):
        _require_cuda(t, 'planes[%d]' % i)
        if t.shape != p0.shape or t.dtype != p0.dtype or t.device != p0.device or t.dim() != 3:
            raise ValueError('the planes must be 3-D and share shape, dtype and device')
    if layout == 'planar':
        k, nr, nc = p0.shape
        lay = _lib.LAYOUT_PLANAR
    elif layout == 'pixel_major':
        nr, nc, k = p0.shape
        lay = _lib.LAYOUT_PIXEL_MAJOR
    else:
        raise ValueError("layout must be 'planar' or 'pixel_major'")
    if not (torch.is_tensor(shifts) and shifts.is_cuda and shifts.dtype == torch.float64
            and tuple(shifts.shape) == (k, 2)):
        raise ValueError('shifts must be a float64 device tensor of shape (%d, 2)' % k)
    dev = p0.device
    L = _lib.lib()
    outs = []
    with torch.cuda.device(dev):
        shifts = shifts.to(dev).contiguous()
        ins = [t.contiguous() for t in planes]
        outs = [torch.empty_like(t) for t in ins]
        if k * nr * nc == 0:
            return outs
        maxv = 16
        for g in range(0, len(ins), maxv):
            gi, go = ins[g:g + maxv], outs[g:g + maxv]
            nbytes = L.nd_amd_warp_translate_workspace_bytes(_DT[p0.dtype], len(gi), k, nr, nc, lay)
            if nbytes == 0:
                raise ValueError('warp_translate: unsupported shape %s' % (tuple(p0.shape),))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            pin = (C.c_void_p * len(gi))(*[t.data_ptr() for t in gi])
            pout = (C.c_void_p * len(go))(*[t.data_ptr() for t in go])
            _lib.check(L.nd_amd_warp_translate(pin, pout, len(gi), _DT[p0.dtype], k, nr, nc, lay,
                                               _ptr(shifts), int(reference), _ptr(ws), nbytes,
                                               _stream_ptr(dev)))
            ws.record_stream(torch.cuda.current_stream(dev))
        for t in ins:
            t.record_stream(torch.cuda.current_stream(dev))
    return outs


# ---------------------------------------------------------------------------
# RGB composites (nd/visualize.py:176-193)
# ---------------------------------------------------------------------------
def _rgb_strides(t):
    """element strides (frame, y, x) of a (frames, y, x) view; the stride of a dimension of size 1 is
    arbitrary in torch and is replaced by the contiguous one, which keeps single planes on the fast path"""
    (k, ny, nx), (st, sy, sx) = t.shape, t.stride()
    if nx == 1:
        sx = 1
    if ny == 1:
        sy = nx * sx
    if k == 1:
        st = ny * sy
    return st, sy, sx


def _rgb_planes(channels, name):
    """channels: one or three entries, each a (frames, y, x) device view or a (numerator, denominator)
    pair of such views (the channel is their quotient, never stored).  All views share shape, dtype,
    device and strides (any non-negative strides: a (y, x, time) variable is passed as
    v.permute(2, 0, 1)).  -> (num tensors, den tensors or None, ctypes pointer arrays)."""
    channels = list(channels)
    if len(channels) not in (1, 3):
        raise ValueError('%s: a frame has 1 or 3 channels, got %d' % (name, len(channels)))
    num, den = [], []
    for ch in channels:
        n, d = ch if isinstance(ch, (tuple, list)) else (ch, None)
        num.append(n)
        den.append(d)
    first = num[0]
    for i, t in enumerate(num + [d for d in den if d is not None]):
        _require_cuda(t, '%s: channel %d' % (name, i % len(num)))
        if (t.dim() != 3 or t.shape != first.shape or t.dtype != first.dtype or t.device != first.device
                or _rgb_strides(t) != _rgb_strides(first)):
            raise ValueError('%s: the planes must be (frames, y, x) views that share shape, dtype, device '
                             'and strides' % name)
    pn = (C.c_void_p * len(num))(*[t.data_ptr() for t in num])
    pd = (C.c_void_p * len(num))(*[(d.data_ptr() if d is not None else None) for d in den])
    return num, den, pn, pd


def rgb_limits(channels, pmin=2, pmax=98):
    """np.nanpercentile(channel, pmin) and (channel, pmax) of every channel plane of every frame, as numpy
    2.2.6 computes them in the data type (exact selection, include/nd_amd.h).  `channels` as in
    _rgb_planes.  Returns device tensors: limits (frames, channels, 2) of the data type and the number of
    non-NaN values per plane, int64 (frames, channels).  Nothing is synchronised."""
    num, den, pn, pd = _rgb_planes(channels, 'rgb_limits')
    t0 = num[0]
    k, ny, nx = t0.shape
    nch = len(num)
    if not (0 <= float(pmin) <= 100 and 0 <= float(pmax) <= 100):
        raise ValueError('Percentiles must be in the range [0, 100]')
    dev = t0.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        limits = torch.empty((k, nch, 2), dtype=t0.dtype, device=dev)
        counts = torch.zeros((k, nch), dtype=torch.int64, device=dev)
        if k == 0:
            return limits, counts
        nbytes = L.nd_amd_rgb_limits_workspace_bytes(_DT[t0.dtype], k * nch)
        if nbytes == 0:
            raise ValueError('rgb_limits: unsupported batch of %d planes' % (k * nch))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        st, sy, sx = _rgb_strides(t0)
        _lib.check(L.nd_amd_rgb_limits(pn, pd, nch, _DT[t0.dtype], k, ny, nx, st, sy, sx, float(pmin),
                                       float(pmax), _ptr(limits), _ptr(counts), _ptr(ws), nbytes,
                                       _stream_ptr(dev)))
        stream = torch.cuda.current_stream(dev)
        for t in [ws] + num + [d for d in den if d is not None]:
            t.record_stream(stream)
    return limits, counts


def rgb_compose(channels, limits=None, vmin=None, vmax=None, mask=None):
    """The 8-bit composite of every frame: (frames, y, x, 3) uint8 on the device.  Per channel
    minval / maxval are vmin[c] / vmax[c] (sequences of Python numbers, one per channel) where given,
    else limits[frame, c] (rgb_limits' output); channels with maxval > minval are stretched to 0 .. 255 in
    the data type, NaN gives 0.  mask: bool or uint8 (y, x) device tensor, pixels where it is 0 are
    black.  One channel is replicated into the three bytes."""
    num, den, pn, pd = _rgb_planes(channels, 'rgb_compose')
    t0 = num[0]
    k, ny, nx = t0.shape
    nch = len(num)
    dev = t0.device
    for v, nm in ((vmin, 'vmin'), (vmax, 'vmax')):
        if v is not None and len(v) != nch:
            raise ValueError('rgb_compose: %s needs one value per channel' % nm)
    if limits is None and (vmin is None or vmax is None):
        raise ValueError('rgb_compose: without limits both vmin and vmax must be given')
    if limits is not None:
        if not (torch.is_tensor(limits) and limits.device == dev and limits.dtype == t0.dtype
                and tuple(limits.shape) == (k, nch, 2)):
            raise ValueError('rgb_compose: limits must be a %s device tensor of shape (%d, %d, 2)'
                             % (t0.dtype, k, nch))
        limits = limits.contiguous()
    if mask is not None:
        if not (torch.is_tensor(mask) and mask.device == dev and tuple(mask.shape) == (ny, nx)
                and mask.dtype in (torch.bool, torch.uint8)):
            raise ValueError('rgb_compose: mask must be a bool or uint8 device tensor of shape (%d, %d)'
                             % (ny, nx))
        mask = mask.contiguous()
    dbl = C.c_double * nch
    pmin_ = dbl(*[float(v) for v in vmin]) if vmin is not None else None
    pmax_ = dbl(*[float(v) for v in vmax]) if vmax is not None else None
    L = _lib.lib()
    with torch.cuda.device(dev):
        out = torch.empty((k, ny, nx, 3), dtype=torch.uint8, device=dev)
        st, sy, sx = _rgb_strides(t0)
        _lib.check(L.nd_amd_rgb_compose(pn, pd, nch, _DT[t0.dtype], k, ny, nx, st, sy, sx, _ptr(limits),
                                        pmin_, pmax_, _ptr(mask), _ptr(out), _stream_ptr(dev)))
        stream = torch.cuda.current_stream(dev)
        for t in num + [d for d in den if d is not None] + [x for x in (limits, mask) if x is not None]:
            t.record_stream(stream)
    return out


# ---------------------------------------------------------------------------
# Pixel classification (nd/classify.py)
# ---------------------------------------------------------------------------
def _dims4(values, name):
    values = [int(v) for v in values]
    if len(values) > 4:
        raise ValueError('%s: at most four row dimensions, got %d' % (name, len(values)))
    return values


def _feature_table(features, sizes, strides, name):
    """features: device tensors of one dtype and device, one per feature; element (0, .., 0) of feature f is
    features[f]'s first element and row (i0, .., i3) lies at i . strides from it (the caller passes views whose
    data_ptr() is that element).  -> (ctypes pointer array, sizes[4], strides[4], workspace tensor)."""
    features = list(features)
    if not features:
        raise ValueError('%s: no features' % name)
    if len(features) > _lib.CLASSIFY_MAX_FEATURES:
        raise ValueError('%s: at most %d features, got %d' % (name, _lib.CLASSIFY_MAX_FEATURES, len(features)))
    first = features[0]
    for i, t in enumerate(features):
        _require_cuda(t, '%s: feature %d' % (name, i))
        if t.dtype != first.dtype or t.device != first.device:
            raise ValueError('%s: the features must share dtype and device' % name)
    sizes, strides = _dims4(sizes, name), _dims4(strides, name)
    if len(sizes) != len(strides) or any(s < 0 for s in strides) or any(n < 0 for n in sizes):
        raise ValueError('%s: sizes and strides must pair up and not be negative' % name)
    pad = 4 - len(sizes)
    sizes, strides = [1] * pad + sizes, [0] * pad + strides
    ptrs = (C.c_void_p * len(features))(*[t.data_ptr() for t in features])
    nbytes = _lib.lib().nd_amd_classify_workspace_bytes(len(features))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=first.device)
    return ptrs, _lib.i64_array(sizes), _lib.i64_array(strides), ws


def _scaler_args(mean, scale, nfeat, dev, name):
    if (mean is None) != (scale is None):
        raise ValueError('%s: scaler needs both mean and scale' % name)
    if mean is None:
        return None, None
    out = []
    for v in (mean, scale):
        v = torch.as_tensor(v, dtype=torch.float64).to(dev).contiguous()
        if v.numel() != nfeat:
            raise ValueError('%s: the scaler has %d entries for %d features' % (name, v.numel(), nfeat))
        out.append(v)
    return out


def _record(tensors, dev):
    stream = torch.cuda.current_stream(dev)
    for t in tensors:
        if t is not None:
            t.record_stream(stream)


def classify_forest(features, sizes, strides, nodes, values, roots, classes, mean=None, scale=None,
                    want_labels=True, want_proba=False):
    """clf.predict / clf.predict_proba of a decision forest over rows that are never stacked
    (nd/classify.py:222-241; include/nd_amd.h nd_amd_classify_forest).  nodes: uint8 device tensor of
    16-byte packed nodes (classify.ForestModel.packed), values float64 (n, classes), roots int32, classes
    float64, all on the features' device.  -> (labels float64 sizes | None, proba float64 sizes + (classes,)
    | None); NaN for rows with a NaN feature."""
    name = 'classify_forest'
    ptrs, sz, st, ws = _feature_table(features, sizes, strides, name)
    dev = features[0].device
    ncls, ntrees, nnodes = int(classes.numel()), int(roots.numel()), int(nodes.numel()) // 16
    for t, dt, nm in ((nodes, torch.uint8, 'nodes'), (values, torch.float64, 'values'),
                      (roots, torch.int32, 'roots'), (classes, torch.float64, 'classes')):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == dt and t.is_contiguous()):
            raise ValueError('%s: %s must be a contiguous %s tensor on %s' % (name, nm, dt, dev))
    if values.dim() != 2 or values.shape[1] != ncls or nodes.numel() % 16 or nodes.data_ptr() % 16:
        raise ValueError('%s: values must be (leaves, %d) and nodes 16-byte records' % (name, ncls))
    if not (want_labels or want_proba):
        raise ValueError('%s: nothing to compute' % name)
    shape = tuple(int(n) for n in sizes)
    with torch.cuda.device(dev):
        mean, scale = _scaler_args(mean, scale, len(features), dev, name)
        labels = torch.empty(shape, dtype=torch.float64, device=dev) if want_labels else None
        proba = torch.empty(shape + (ncls,), dtype=torch.float64, device=dev) if want_proba else None
        _lib.check(_lib.lib().nd_amd_classify_forest(
            ptrs, len(features), _DT[features[0].dtype], sz, st, _ptr(nodes), nnodes, _ptr(values), _ptr(roots),
            ntrees, _ptr(classes), ncls, _ptr(mean), _ptr(scale), _ptr(labels), _ptr(proba), _ptr(ws), ws.numel(),
            _stream_ptr(dev)))
        _record(list(features) + [nodes, values, roots, classes, mean, scale, ws], dev)
    return labels, proba


def classify_kmeans(features, sizes, strides, centers, mean=None, scale=None):
    """KMeans.predict over unstacked rows: the first nearest centre in float64 (nd_amd_classify_kmeans).
    centers: float64 (k, features) device tensor.  -> float64 labels of shape sizes, NaN for masked rows."""
    name = 'classify_kmeans'
    ptrs, sz, st, ws = _feature_table(features, sizes, strides, name)
    dev = features[0].device
    if not (torch.is_tensor(centers) and centers.device == dev and centers.dtype == torch.float64
            and centers.dim() == 2 and centers.shape[1] == len(features) and centers.shape[0] >= 1):
        raise ValueError('%s: centers must be a float64 (k, %d) tensor on %s' % (name, len(features), dev))
    centers = centers.contiguous()
    with torch.cuda.device(dev):
        mean, scale = _scaler_args(mean, scale, len(features), dev, name)
        labels = torch.empty(tuple(int(n) for n in sizes), dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().nd_amd_classify_kmeans(
            ptrs, len(features), _DT[features[0].dtype], sz, st, _ptr(centers), int(centers.shape[0]), _ptr(mean),
            _ptr(scale), _ptr(labels), _ptr(ws), ws.numel(), _stream_ptr(dev)))
        _record(list(features) + [centers, mean, scale, ws], dev)
    return labels


def classify_knn(features, sizes, strides, train, target, classes, k, mean=None, scale=None,
                 want_labels=True, want_proba=False):
    """KNeighborsClassifier.predict / predict_proba (uniform weights, Euclidean) over unstacked rows: the k
    training samples smallest by (float64 squared distance, index) vote (nd_amd_classify_knn).  train: float64
    (n_train, features), target: int32 (n_train,) indices into classes, classes: float64, all on the features'
    device.  -> (labels float64 sizes | None, proba float64 sizes + (classes,) | None); NaN for masked rows."""
    name = 'classify_knn'
    ptrs, sz, st, ws = _feature_table(features, sizes, strides, name)
    dev = features[0].device
    for t, dt, nm in ((train, torch.float64, 'train'), (target, torch.int32, 'target'),
                      (classes, torch.float64, 'classes')):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == dt and t.is_contiguous()):
            raise ValueError('%s: %s must be a contiguous %s tensor on %s' % (name, nm, dt, dev))
    if train.dim() != 2 or train.shape[1] != len(features) or train.shape[0] < 1 \
            or target.shape != (train.shape[0],) or classes.dim() != 1 or classes.numel() < 1:
        raise ValueError('%s: train must be (n_train, %d), target (n_train,) and classes (n_classes,)'
                         % (name, len(features)))
    k, ntrain, ncls = int(k), int(train.shape[0]), int(classes.numel())
    if not 1 <= k <= ntrain:
        raise ValueError('%s: k = %d neighbours of %d training samples' % (name, k, ntrain))
    if k > _lib.CLASSIFY_KNN_MAX_K or len(features) > _lib.CLASSIFY_KNN_MAX_FEATURES:
        raise NotImplementedError('%s: serves k <= %d and up to %d features, got k = %d and %d features'
                                  % (name, _lib.CLASSIFY_KNN_MAX_K, _lib.CLASSIFY_KNN_MAX_FEATURES, k,
                                     len(features)))
    if ntrain >= 2 ** 31:
        raise ValueError('%s: too many training samples' % name)
    if not (want_labels or want_proba):
        raise ValueError('%s: nothing to compute' % name)
    shape = tuple(int(n) for n in sizes)
    with torch.cuda.device(dev):
        mean, scale = _scaler_args(mean, scale, len(features), dev, name)
        labels = torch.empty(shape, dtype=torch.float64, device=dev) if want_labels else None
        proba = torch.empty(shape + (ncls,), dtype=torch.float64, device=dev) if want_proba else None
        _lib.check(_lib.lib().nd_amd_classify_knn(
            ptrs, len(features), _DT[features[0].dtype], sz, st, _ptr(train), _ptr(target), ntrain, k, _ptr(classes),
            ncls, _ptr(mean), _ptr(scale), _ptr(labels), _ptr(proba), _ptr(ws), ws.numel(), _stream_ptr(dev)))
        _record(list(features) + [train, target, classes, mean, scale, ws], dev)
    return labels, proba


def classify_linear(features, sizes, strides, coef, intercept, classes, link='none', func='predict', mean=None,
                    scale=None):
    """decision_function / predict / predict_proba of a linear classifier over unstacked rows
    (nd_amd_classify_linear).  coef: float64 (n_rows, features), intercept: float64 (n_rows,), classes:
    float64 (2 for one row of coefficients, else n_rows), on the features' device.  link: 'none', 'softmax'
    or 'ovr'.  -> float64 of shape sizes ('predict'), sizes + (n_rows,) ('decision_function') or sizes +
    (classes,) ('predict_proba'); NaN for masked rows."""
    name = 'classify_linear'
    ptrs, sz, st, ws = _feature_table(features, sizes, strides, name)
    dev = features[0].device
    for t, nm in ((coef, 'coef'), (intercept, 'intercept'), (classes, 'classes')):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError('%s: %s must be a contiguous float64 tensor on %s' % (name, nm, dev))
    if coef.dim() != 2 or coef.shape[1] != len(features) or coef.shape[0] < 1 \
            or intercept.shape != (coef.shape[0],):
        raise ValueError('%s: coef must be (n_rows, %d) and intercept (n_rows,)' % (name, len(features)))
    ncoef = int(coef.shape[0])
    ncls = 2 if ncoef == 1 else ncoef
    if classes.shape != (ncls,):
        raise ValueError('%s: %d rows of coefficients need %d classes' % (name, ncoef, ncls))
    if link not in _lib.LINKS or func not in _lib.LINEAR_OUTPUTS:
        raise ValueError('%s: link %r / func %r' % (name, link, func))
    if func == 'predict_proba' and link == 'none':
        raise ValueError('%s: predict_proba needs a link' % name)
    shape = tuple(int(n) for n in sizes)
    width = {'predict': (), 'decision_function': (ncoef,), 'predict_proba': (ncls,)}[func]
    with torch.cuda.device(dev):
        mean, scale = _scaler_args(mean, scale, len(features), dev, name)
        out = torch.empty(shape + width, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().nd_amd_classify_linear(
            ptrs, len(features), _DT[features[0].dtype], sz, st, _ptr(coef), _ptr(intercept), ncoef, _ptr(classes),
            _lib.LINKS[link], _lib.LINEAR_OUTPUTS[func], _ptr(mean), _ptr(scale), _ptr(out), _ptr(ws), ws.numel(),
            _stream_ptr(dev)))
        _record(list(features) + [coef, intercept, classes, mean, scale, ws], dev)
    return out


def _label_args(labels, label_strides, sizes, dev, name):
    nd = len(sizes)
    if labels is None:
        return None, None
    if not (torch.is_tensor(labels) and labels.device == dev and labels.dtype == torch.float64):
        raise ValueError('%s: labels must be a float64 tensor on %s' % (name, dev))
    ls = _dims4(label_strides, name)
    if len(ls) != nd or any(s < 0 for s in ls):
        raise ValueError('%s: one non-negative label stride per row dimension' % name)
    reach = sum((int(n) - 1) * s for n, s in zip(sizes, ls)) if all(int(n) > 0 for n in sizes) else -1
    if reach >= labels.numel():
        raise ValueError('%s: the label strides reach element %d of %d labels' % (name, reach, labels.numel()))
    return labels, _lib.i64_array([0] * (4 - nd) + ls)


def classify_gather(features, sizes, strides, labels=None, label_strides=None):
    """The training rows of make_Xy (nd/classify.py:164-178): rows whose label is > 0 and not NaN (all rows
    without labels) and whose features hold no NaN, compacted in row order.  labels: float64 device tensor
    read at i . label_strides.  -> (X (n, features) of the data type, y float64 (n,) | None, mask uint8
    (rows,)).  Synchronises once, to learn n."""
    name = 'classify_gather'
    ptrs, sz, st, ws = _feature_table(features, sizes, strides, name)
    dev = features[0].device
    lab, ls = _label_args(labels, label_strides, list(sizes), dev, name)
    rows = 1
    for n in sizes:
        rows *= int(n)
    nblocks = -(-rows // _lib.CLASSIFY_BLOCK_ROWS)
    L = _lib.lib()
    with torch.cuda.device(dev):
        mask = torch.empty(rows, dtype=torch.uint8, device=dev)
        offsets = torch.empty(max(nblocks, 1), dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        args = (ptrs, len(features), _DT[features[0].dtype], sz, st, _ptr(lab), ls)
        _lib.check(L.nd_amd_classify_select(*args, _ptr(mask), _ptr(offsets), _ptr(count), _ptr(ws), ws.numel(),
                                            _stream_ptr(dev)))
        n = int(count.item())
        X = torch.empty((n, len(features)), dtype=features[0].dtype, device=dev)
        y = torch.empty(n, dtype=torch.float64, device=dev) if lab is not None else None
        if n:
            _lib.check(L.nd_amd_classify_gather(*args, _ptr(mask), _ptr(offsets), _ptr(X), _ptr(y), _ptr(ws),
                                                ws.numel(), _stream_ptr(dev)))
        _record(list(features) + [lab, ws, offsets], dev)
    return X, y, mask


def _class_args(var, labels, label_strides, name):
    _require_cuda(var, name + ': var')
    order = sorted(range(var.dim()), key=lambda d: -var.stride(d))
    if var.dim() > 4:
        raise ValueError('%s: at most four dimensions' % name)
    lab, _ = _label_args(labels, label_strides, list(var.shape), var.device, name)
    pad = 4 - var.dim()
    sizes = [1] * pad + [var.shape[d] for d in order]
    strides = [0] * pad + [var.stride(d) for d in order]
    ls = [0] * pad + [int(label_strides[d]) for d in order]
    return lab, _lib.i64_array(sizes), _lib.i64_array(strides), _lib.i64_array(ls)


def class_stats(var, labels, label_strides, nclasses):
    """Per class l in 0 .. nclasses-1 of `var` under labels read at i . label_strides (one stride per dimension
    of var, 0 = broadcast): float64 sum and int64 count of the non-NaN values, int64 count of the NaN values
    (nd_amd_class_stats; the statistics class_mean needs, nd/classify.py:36-44).  Device tensors."""
    name = 'class_stats'
    lab, sz, st, ls = _class_args(var, labels, label_strides, name)
    dev = var.device
    with torch.cuda.device(dev):
        out = [torch.empty(int(nclasses), dtype=dt, device=dev) for dt in (torch.float64, torch.int64, torch.int64)]
        _lib.check(_lib.lib().nd_amd_class_stats(_ptr(var), _DT[var.dtype], sz, st, _ptr(lab), ls, int(nclasses),
                                                 _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream_ptr(dev)))
        _record([var, lab], dev)
    return tuple(out)


def class_fill(var, labels, label_strides, fill):
    """A new tensor like var: fill[l] where the label is l in 0 .. len(fill)-2, elsewhere var's value, or
    fill[-1] where that is NaN (nd_amd_class_fill).  var must be dense; fill: device tensor of var's dtype."""
    name = 'class_fill'
    lab, sz, st, ls = _class_args(var, labels, label_strides, name)
    dev = var.device
    if not (torch.is_tensor(fill) and fill.device == dev and fill.dtype == var.dtype and fill.dim() == 1
            and fill.numel() >= 2):
        raise ValueError('%s: fill must be a 1-D %s tensor on %s' % (name, var.dtype, dev))
    fill = fill.contiguous()
    with torch.cuda.device(dev):
        out = torch.empty_like(var)
        if out.stride() != var.stride():
            raise ValueError('%s: var must be a dense tensor (call .contiguous())' % name)
        _lib.check(_lib.lib().nd_amd_class_fill(_ptr(var), _ptr(out), _DT[var.dtype], sz, st, _ptr(lab), ls,
                                                int(fill.numel()) - 1, _ptr(fill), _stream_ptr(dev)))
        _record([var, lab, fill], dev)
    return out


# ---------------------------------------------------------------------------
# Training k-means on the device (include/nd_amd.h, nd_amd_kmeans_step and its neighbours)
# ---------------------------------------------------------------------------
def _rows_of(sizes):
    rows = 1
    for n in sizes:
        rows *= int(n)
    return rows


def _fit_workspace(nfeat, k, rows, dev, name):
    """the pointer table and the per-block partial sums of the reducing passes"""
    if k < 1:
        raise ValueError('%s: needs k >= 1 centres, got %d' % (name, k))
    if k * (nfeat + 1) > _lib.KMEANS_FIT_MAX_ACC:
        raise NotImplementedError('%s: serves k * (features + 1) <= %d, got k = %d and %d features'
                                  % (name, _lib.KMEANS_FIT_MAX_ACC, k, nfeat))
    nbytes = _lib.lib().nd_amd_kmeans_fit_workspace_bytes(nfeat, k, rows)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def kmeans_step(features, sizes, strides, centers, labels, mean=None, scale=None):
    """One Lloyd iteration over unstacked rows (nd_amd_kmeans_step): every row without a NaN feature goes to its
    first nearest centre in float64.  centers: float64 (k, features) device tensor.  labels: int32 device tensor of
    `sizes`, read and overwritten (-1 for rows with a NaN feature; fill it with -1 before the first iteration).
    -> (sums float64 (k, features), counts int64 (k,), inertia float64 (), changed int64 ()), device tensors;
    changed counts the rows whose label differs from the one found in `labels`.  The sums are formed in a fixed
    order: the same inputs give the same bits."""
    name = 'kmeans_step'
    ptrs, sz, st, _ = _feature_table(features, sizes, strides, name)
    dev = features[0].device
    nfeat, rows = len(features), _rows_of(sizes)
    if not (torch.is_tensor(centers) and centers.device == dev and centers.dtype == torch.float64
            and centers.dim() == 2 and centers.shape[1] == nfeat and centers.shape[0] >= 1):
        raise ValueError('%s: centers must be a float64 (k, %d) tensor on %s' % (name, nfeat, dev))
    if not (torch.is_tensor(labels) and labels.device == dev and labels.dtype == torch.int32
            and labels.is_contiguous() and labels.numel() == rows):
        raise ValueError('%s: labels must be a contiguous int32 tensor of %d rows on %s' % (name, rows, dev))
    centers = centers.contiguous()
    k = int(centers.shape[0])
    with torch.cuda.device(dev):
        ws = _fit_workspace(nfeat, k, rows, dev, name)
        mean, scale = _scaler_args(mean, scale, nfeat, dev, name)
        fbuf = torch.empty(k * nfeat + 1, dtype=torch.float64, device=dev)
        ibuf = torch.empty(k + 1, dtype=torch.int64, device=dev)
        sums, inertia, counts, changed = fbuf[:k * nfeat].view(k, nfeat), fbuf[k * nfeat], ibuf[:k], ibuf[k]
        _lib.check(_lib.lib().nd_amd_kmeans_step(
            ptrs, nfeat, _DT[features[0].dtype], sz, st, _ptr(centers), k, _ptr(mean), _ptr(scale), _ptr(labels),
            _ptr(sums), _ptr(counts), _ptr(inertia), _ptr(changed), _ptr(ws), ws.numel(), _stream_ptr(dev)))
        _record(list(features) + [centers, labels, mean, scale, ws], dev)
    return sums, counts, inertia, changed


def feature_moments(features, sizes, strides, mean=None, scale=None):
    """Over the rows without a NaN feature (nd_amd_feature_moments): -> (count int64 (), mean float64 (features,),
    var float64 (features,)), device tensors; var is the population variance, sum (x - mean)^2 / count in a
    second pass.  With mean / scale given the moments are those of the scaled values.  Deterministic."""
    name = 'feature_moments'
    ptrs, sz, st, _ = _feature_table(features, sizes, strides, name)
    dev = features[0].device
    nfeat, rows = len(features), _rows_of(sizes)
    with torch.cuda.device(dev):
        ws = _fit_workspace(nfeat, 1, rows, dev, name)
        mean, scale = _scaler_args(mean, scale, nfeat, dev, name)
        count = torch.empty((), dtype=torch.int64, device=dev)
        fmean = torch.empty(nfeat, dtype=torch.float64, device=dev)
        fvar = torch.empty(nfeat, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().nd_amd_feature_moments(
            ptrs, nfeat, _DT[features[0].dtype], sz, st, _ptr(mean), _ptr(scale), _ptr(count), _ptr(fmean), _ptr(fvar),
            _ptr(ws), ws.numel(), _stream_ptr(dev)))
        _record(list(features) + [mean, scale, ws], dev)
    return count, fmean, fvar


def gather_rows(features, sizes, strides, index, mean=None, scale=None):
    """The rows at `index` (int64 device tensor of row numbers, row-major over `sizes`, repeats allowed) as a dense
    matrix (nd_amd_gather_rows): -> (X (m, features) of the data type, scaled where mean / scale are given, valid
    uint8 (m,): 1 where the row has no NaN feature).  An index outside the rows gives a NaN row and valid 0."""
    name = 'gather_rows'
    ptrs, sz, st, ws = _feature_table(features, sizes, strides, name)
    dev = features[0].device
    if not (torch.is_tensor(index) and index.device == dev and index.dtype == torch.int64 and index.dim() == 1):
        raise ValueError('%s: index must be a 1-D int64 tensor on %s' % (name, dev))
    index = index.contiguous()
    m, nfeat = int(index.numel()), len(features)
    with torch.cuda.device(dev):
        mean, scale = _scaler_args(mean, scale, nfeat, dev, name)
        X = torch.empty((m, nfeat), dtype=features[0].dtype, device=dev)
        valid = torch.empty(m, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().nd_amd_gather_rows(
            ptrs, nfeat, _DT[features[0].dtype], sz, st, _ptr(index), m, _ptr(mean), _ptr(scale), _ptr(X), _ptr(valid),
            _ptr(ws), ws.numel(), _stream_ptr(dev)))
        _record(list(features) + [index, mean, scale, ws], dev)
    return X, valid


# ---------------------------------------------------------------------------
# polygons burned into a label raster (nd/vector.py:48-187; include/nd_amd.h nd_amd_rasterize_polygons)
# ---------------------------------------------------------------------------
RASTERIZE_MAX_CROSSINGS = _lib.RASTERIZE_MAX_CROSSINGS
# |pixel coordinate| the table accepts.  xc = x1 + ((v - y1) * (x2 - x1)) / (y2 - y1) with (v - y1) / (y2 - y1) in
# [0, 1) lies within a few roundings of [x1, x2]: at most 4 * 2^-53 * 2^41 = 2^-10 pixel beyond it below this cap.  The
# column box (the extent and one pixel beyond) may stand for the row only while that excess stays under a pixel.
RASTERIZE_MAX_COORD = float(2 ** 40)
_VALUE_DT = {torch.int64: _lib.I64, torch.float64: _lib.F64}


def _offsets(a, name, last):
    a = np.ascontiguousarray(np.asarray(a.cpu() if torch.is_tensor(a) else a), dtype=np.int64)
    if a.ndim != 1 or a.size < 1 or a[0] != 0 or a[-1] != last or np.any(np.diff(a) < 0):
        raise ValueError('%s must be non-decreasing int64 offsets from 0 to %d' % (name, last))
    return a


class PolygonTable:
    """The polygons of one raster on the device -- pixel-coordinate vertices, ring and polygon offsets, and the
    row / column boxes with the prefix sums of their rows -- uploaded once and shared by every
    rasterize_polygons call (the columns and dates of one nd_amd.vector.rasterize)."""

    def __init__(self, verts, ring_offsets, poly_offsets, ny, nx, device=None):
        if torch.is_tensor(verts):
            if not verts.is_cuda:
                raise ValueError('verts must be a numpy array or live on a ROCm device (got %s); nd_amd has no '
                                 'CPU path' % verts.device)
            device = verts.device if device is None else device
            host = verts.detach().cpu().numpy()
        else:
            host = np.asarray(verts)
        host = np.ascontiguousarray(host, dtype=np.float64)
        if host.size == 0:
            host = host.reshape(0, 2)
        if host.ndim != 2 or host.shape[1] != 2:
            raise ValueError('verts must be (nverts, 2) pixel coordinates, got shape %s' % (host.shape,))
        if not np.all(np.isfinite(host)):
            raise ValueError('non-finite vertex coordinates')
        if host.size and np.max(np.abs(host)) > RASTERIZE_MAX_COORD:
            raise ValueError('pixel coordinates beyond 2^40 are not served (the crossing abscissa would no longer '
                             'stay within a pixel of the polygon\'s extent)')
        ny, nx = int(ny), int(nx)
        if ny < 0 or nx < 0:
            raise ValueError('negative raster size (%d, %d)' % (ny, nx))
        if ny >= 2 ** 31 or nx >= 2 ** 31:
            raise ValueError('raster sides of 2^31 pixels or more are not served')
        ring_offsets = _offsets(ring_offsets, 'ring_offsets', host.shape[0])
        poly_offsets = _offsets(poly_offsets, 'poly_offsets', ring_offsets.size - 1)
        self.npolys = poly_offsets.size - 1
        if self.npolys >= 2 ** 32 - 1:
            raise ValueError('fewer than 2^32 - 1 polygons are served')
        self.ny, self.nx = ny, nx
        boxes, row_work = polygon_boxes(host, ring_offsets, poly_offsets, ny, nx)
        self.items = int(row_work[-1])
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError('nd_amd needs a ROCm GPU: the compute path is HIP only')
            device = torch.device('cuda', torch.cuda.current_device())
        up = lambda a: torch.from_numpy(a).to(torch.device(device))
        # one spare vertex keeps the table non-empty (and its pointer non-null) for polygons without vertices
        self.verts = up(np.concatenate([host, np.zeros((1, 2))]))
        self.ring_offsets, self.poly_offsets = up(ring_offsets), up(poly_offsets)
        self.boxes, self.row_work = up(np.concatenate([boxes, np.zeros((1, 4), np.int32)])), up(row_work)
        self.device = self.verts.device         # with its index, whatever form `device` had ('cuda', 'cuda:0')


def polygon_boxes(verts, ring_offsets, poly_offsets, ny, nx):
    """-> boxes int32 (npolys, 4) r0, r1, c0, c1 clipped to the raster, row_work int64 (npolys + 1) prefix sums of
    r1 - r0.  A box holds every row i with ymin <= i + 0.5 <= ymax over the polygon's vertices (columns
    likewise), and a pixel beyond.  A superset is all the kernel needs while the crossing abscissae stay within
    a pixel of the extent, which RASTERIZE_MAX_COORD sees to: inside the box the rule decides."""
    npolys = poly_offsets.size - 1
    boxes = np.zeros((npolys, 4), np.int32)
    v0 = ring_offsets[poly_offsets[:-1]]
    v1 = ring_offsets[poly_offsets[1:]]
    some = np.nonzero(v1 > v0)[0]
    if some.size:
        # reduceat over the non-empty polygons: their vertex ranges are consecutive and cover what lies between
        starts = v0[some]
        for col, (n, lo, hi) in enumerate(((nx, 2, 3), (ny, 0, 1))):
            cmin = np.minimum.reduceat(verts[:, col], starts)
            cmax = np.maximum.reduceat(verts[:, col], starts)
            first = np.clip(np.floor(cmin - 0.5), 0, n)
            end = np.clip(np.floor(cmax - 0.5) + 2, 0, n)
            boxes[some, lo] = first.astype(np.int32)
            boxes[some, hi] = np.maximum(first, end).astype(np.int32)
    empty = (boxes[:, 1] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 2])
    boxes[empty] = 0
    row_work = np.zeros(npolys + 1, np.int64)
    np.cumsum(boxes[:, 1].astype(np.int64) - boxes[:, 0], out=row_work[1:])
    return boxes, row_work


def rasterize_polygons(verts, ring_offsets, poly_offsets, values, ny, nx, layer=None, nlayers=1, fill=0, out=None):
    """Burn polygons into a raster (include/nd_amd.h has the rule).  verts: (nverts, 2) float64 pixel coordinates
    (px, py) as a numpy array or a ROCm tensor, with ring_offsets (nrings + 1) and poly_offsets (npolys + 1, into
    the rings) -- or a PolygonTable built from them once, ring_offsets and poly_offsets then None.  The boxes and
    the prefix sums of their rows are computed here on the host from those coordinates.  values: one per polygon,
    integers (burned as int64) or floats (float64), a sequence, numpy array or ROCm tensor.  layer: npolys layer
    numbers in [0, nlayers), None = all 0.  out: a ROCm tensor shaped (nlayers, ny, nx) of the values' type, any
    non-negative strides (a permuted (ny, nx, nlayers) buffer gives the reference's (y, x, time) result without a
    transpose); allocated contiguous when None.  -> out.  The value of a pixel is that of the highest-index polygon
    of its layer that contains its centre, `fill` where there is none."""
    for t, nm in ((verts, 'verts'), (values, 'values'), (layer, 'layer'), (out, 'out')):
        if torch.is_tensor(t) and not t.is_cuda:
            raise ValueError('%s must live on a ROCm device (got %s); nd_amd has no CPU path' % (nm, t.device))
    ny, nx, nlayers = int(ny), int(nx), int(nlayers)
    if nlayers < 0:
        raise ValueError('nlayers must not be negative, got %d' % nlayers)
    dev = next((t.device for t in (out, values, verts) if torch.is_tensor(t)), None)
    if isinstance(verts, PolygonTable):
        if ring_offsets is not None or poly_offsets is not None:
            raise ValueError('a PolygonTable carries its offsets: pass ring_offsets=None, poly_offsets=None')
        table = verts
        if (table.ny, table.nx) != (ny, nx):
            raise ValueError('the PolygonTable was built for a (%d, %d) raster, not (%d, %d)'
                             % (table.ny, table.nx, ny, nx))
    else:
        table = PolygonTable(verts, ring_offsets, poly_offsets, ny, nx, device=dev)
    dev = table.device
    npolys = table.npolys
    if ny * nx * nlayers >= 2 ** 32:
        raise ValueError('rasters of 2^32 pixels x layers or more are not served (%d x %d x %d)' % (ny, nx, nlayers))

    if torch.is_tensor(values):
        vals = values
        if vals.dtype not in _VALUE_DT:
            vals = vals.to(torch.float64 if vals.is_floating_point() else torch.int64)
    else:
        host = np.asarray(values)
        if host.dtype.kind in 'biu':
            if host.dtype.kind == 'u' and host.size and host.max() > np.iinfo(np.int64).max:
                raise ValueError('values beyond int64')
            host = host.astype(np.int64)
        elif host.dtype.kind == 'f':
            host = host.astype(np.float64)
        else:
            raise TypeError('values must be integers or floats, got %s' % host.dtype)
        vals = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    if vals.dim() != 1 or vals.numel() != npolys or vals.device != dev:
        raise ValueError('values must be one per polygon (%d) on %s, got shape %s on %s'
                         % (npolys, dev, tuple(vals.shape), vals.device))
    vals = vals.contiguous()

    lay = None
    if layer is not None:
        host = np.asarray(layer.cpu() if torch.is_tensor(layer) else layer)
        if host.shape != (npolys,) or (host.size and host.dtype.kind not in 'iu'):
            raise ValueError('layer must be %d integers, one per polygon' % npolys)
        if host.size and (host.min() < 0 or host.max() >= nlayers):
            raise ValueError('layer numbers must lie in [0, %d)' % nlayers)
        lay = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(dev) if host.size else None
    elif npolys and nlayers < 1:
        raise ValueError('polygons without a layer to burn them into')

    shape = (nlayers, ny, nx)
    if out is None:
        with torch.cuda.device(dev):
            out = torch.empty(shape, dtype=vals.dtype, device=dev)
    else:
        if tuple(out.shape) != shape or out.dtype != vals.dtype or out.device != dev:
            raise ValueError('out must be %s of %s on %s, got %s of %s on %s'
                             % (shape, vals.dtype, dev, tuple(out.shape), out.dtype, out.device))
        if any(s == 0 and n > 1 for s, n in zip(out.stride(), shape)):
            raise ValueError('an expanded out (stride 0) is not served')
    fill_host = (C.c_int64(int(fill)) if vals.dtype == torch.int64 else C.c_double(float(fill)))
    L = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = L.nd_amd_rasterize_workspace_bytes(nlayers, ny, nx)
        ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
        _lib.check(L.nd_amd_rasterize_polygons(
            _ptr(table.verts), _ptr(table.ring_offsets), _ptr(table.poly_offsets), _ptr(lay), _ptr(table.row_work),
            _ptr(table.boxes), _ptr(vals), _VALUE_DT[vals.dtype], C.cast(C.pointer(fill_host), C.c_void_p), npolys,
            nlayers, ny, nx, _ptr(out), out.stride(0), out.stride(1), out.stride(2), _ptr(ws), int(nbytes),
            _stream_ptr(dev)))
        _record([table.verts, table.ring_offsets, table.poly_offsets, table.row_work, table.boxes, lay, vals, ws,
                 out], dev)
    return out


# ---------------------------------------------------------------------------
# stacks brought onto another rotation-free grid (nd/warp.py:872-1097; include/nd_amd.h nd_amd_resample)
# ---------------------------------------------------------------------------
RESAMPLE_MAX_TAPS = _lib.RESAMPLE_MAX_TAPS
RESAMPLE_METHODS = ('nearest', 'bilinear', 'cubic', 'average')
# raw runs the table builder is willing to lay out before it gives up (the entry serves RESAMPLE_MAX_TAPS)
_RESAMPLE_TABLE_CAP = 16 * RESAMPLE_MAX_TAPS


class AxisTable:
    """The taps of one axis: start and count int32 (m), count 0 = outside; weights float64 (taps, m), tap-major.
    numpy arrays as resample_axis returns them, ROCm tensors after .to(device)."""

    def __init__(self, n, m, method, start, count, weights):
        self.n, self.m, self.method = int(n), int(m), method
        self.start, self.count, self.weights = start, count, weights
        self.taps = int(weights.shape[0])

    @property
    def device(self):
        return self.start.device if torch.is_tensor(self.start) else None

    def to(self, device):
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self.device == device:
            return self
        up = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device)   # noqa: E731
        return AxisTable(self.n, self.m, self.method, up(self.start), up(self.count), up(self.weights))


def _resample_phi(method, d):
    d = np.abs(d)
    if method == 'bilinear':
        return np.where(d < 1.0, 1.0 - d, 0.0)
    a = -0.5
    near = ((a + 2.0) * d - (a + 3.0)) * (d * d) + 1.0
    far = (((d - 5.0) * d + 8.0) * d - 4.0) * a
    return np.where(d < 1.0, near, np.where(d < 2.0, far, 0.0))


def resample_axis(n, m, src, dst, method):
    """The tap table of one axis (README.md "Resampling and reprojection" has the definition): n source samples on
    src = (a_s, c_s), m output samples on dst = (a_d, c_d), the (a, c) / (e, f) terms of the two transforms.
    method: 'nearest', 'bilinear', 'cubic' or 'average'.  -> AxisTable of numpy arrays; float64 throughout, every
    operation bracketed as the definition writes it, so that the table equals a scalar evaluation bit for bit."""
    if method not in RESAMPLE_METHODS:
        raise ValueError('method must be one of %s, got %r' % (RESAMPLE_METHODS, method))
    n, m = int(n), int(m)
    if n < 0 or m < 0 or n >= 2 ** 31 or m >= 2 ** 31:
        raise ValueError('axis lengths must lie in [0, 2^31), got n=%d m=%d' % (n, m))
    a_s, c_s, a_d, c_d = float(src[0]), float(src[1]), float(dst[0]), float(dst[1])
    if not (np.isfinite(a_s) and np.isfinite(a_d)) or a_s == 0.0 or a_d == 0.0:
        raise ValueError('a grid needs a finite pixel size other than 0, got source %r destination %r'
                         % ((a_s, c_s), (a_d, c_d)))
    rho = abs(a_d / a_s)
    with np.errstate(all='ignore'):
        u = ((c_d + a_d * (np.arange(m, dtype=np.float64) + 0.5)) - c_s) / a_s
        inside = (u >= 0.0) & (u < n)
        u = np.where(inside, u, 0.0)
        if method == 'nearest':
            return AxisTable(n, m, method, np.floor(u).astype(np.int32), inside.astype(np.int32),
                             inside.astype(np.float64)[None, :])
        if method == 'average':
            lo, hi = u - rho / 2.0, u + rho / 2.0
            x0 = np.maximum(0.0, np.floor(lo))
            x1 = np.minimum(float(n), np.ceil(hi))
        else:
            R = 1.0 if method == 'bilinear' else 2.0
            s = max(rho, 1.0)
            x0 = np.maximum(0.0, np.floor(u - R * s + 0.5))
            x1 = np.minimum(float(n), np.floor(u + R * s + 0.5))
        x1 = np.where(inside, x1, x0)
        K = int(np.max(x1 - x0)) if m else 0
        if K > _RESAMPLE_TABLE_CAP:
            raise ValueError('%d taps on an axis: at most %d are served' % (K, RESAMPLE_MAX_TAPS))
        raw = np.zeros((max(K, 1), m), np.float64)
        for t in range(K):
            x = x0 + t
            if method == 'average':
                w = np.minimum(x + 1.0, hi) - np.maximum(x, lo)
            else:
                w = _resample_phi(method, (x + 0.5 - u) / s)
            raw[t] = np.where(x < x1, w, 0.0)
        # zeros trimmed from both ends of the run, zeros inside kept
        some = raw != 0.0
        first = np.argmax(some, axis=0)
        last = raw.shape[0] - 1 - np.argmax(some[::-1], axis=0)
        count = np.where(some.any(axis=0), last - first + 1, 0).astype(np.int32)
        T = max(int(count.max()) if m else 0, 1)
        cols = np.arange(m)
        run = np.zeros((T, m), np.float64)
        total = np.zeros(m, np.float64)
        for t in range(T):
            run[t] = raw[np.minimum(first + t, raw.shape[0] - 1), cols]
            total = np.where(t < count, total + run[t], total)
        weights = np.where(np.arange(T)[:, None] < count[None, :], run / total[None, :], 0.0)
    start = np.where(count > 0, x0 + first, 0.0).astype(np.int32)
    return AxisTable(n, m, method, start, count, weights)


def _resample_axes(dims, ndim):
    dims = tuple(dims)
    if len(dims) != ndim or len(set(dims)) != ndim or 'y' not in dims or 'x' not in dims:
        raise ValueError("dims must name the tensor's %d axes, 'y' and 'x' among them, got %r" % (ndim, dims))
    if ndim > 4:
        raise ValueError('at most two axes besides y and x are served, got dims %r' % (dims,))
    return dims.index('y'), dims.index('x'), [d for d in range(ndim) if dims[d] not in ('y', 'x')]


def _empty_like_strides(t, shape):
    """an uninitialised tensor of `shape` whose axes are ordered in memory as t's are"""
    order = sorted(range(t.dim()), key=lambda d: (-t.stride(d), d))
    inv = [order.index(d) for d in range(t.dim())]
    return torch.empty([shape[d] for d in order], dtype=t.dtype, device=t.device).permute(*inv)


def resample(planes, table_y, table_x, dims=('time', 'y', 'x'), fill=None, out=None):
    """Bring images onto another grid (include/nd_amd.h has the definition).  planes: one ROCm tensor or a list of
    same-shaped ones of one dtype, with the axes `dims` names: y, x and up to two more in any order and with any
    non-negative strides (crops of larger tensors included).  (time, y, x) and (y, x, time) data are read where
    they lie and the result has the same memory order.  table_y / table_x: the AxisTables of resample_axis; numpy
    tables are uploaded once for all planes of the call, tables already on the device are used as they are.  Where
    both tables are 'nearest' the elements are copied bit for bit (1, 2, 4 or 8 bytes: bool, integers and floats
    keep their type); otherwise float32 and float64 are served and integers are computed and returned as float64.
    fill: the value outside the source, NaN by default for floating data and 0 for integers.  out: a tensor (or
    list) of the result's shape and type, any strides.  -> a tensor, or a list where a list was given."""
    single = torch.is_tensor(planes)
    planes = [planes] if single else list(planes)
    if not planes:
        return []
    p0 = planes[0]
    for t in planes:
        if not torch.is_tensor(t):
            raise TypeError('planes must be torch tensors, got %r' % type(t))
        if not t.is_cuda:
            raise ValueError('planes must live on a ROCm device (got %s); nd_amd has no CPU path' % t.device)
        if t.shape != p0.shape or t.dtype != p0.dtype or t.device != p0.device:
            raise ValueError('the planes of one call share shape, dtype and device')
    for tb in (table_y, table_x):
        if not isinstance(tb, AxisTable):
            raise TypeError('table_y and table_x are the AxisTables resample_axis returns')
    dev = p0.device
    ay, ax, extra = _resample_axes(dims, p0.dim())
    if (table_y.n, table_x.n) != (p0.shape[ay], p0.shape[ax]):
        raise ValueError('the tables were built for a (%d, %d) source, the planes are (%d, %d)'
                         % (table_y.n, table_x.n, p0.shape[ay], p0.shape[ax]))
    nearest = table_y.method == 'nearest' and table_x.method == 'nearest'
    if nearest:
        if p0.element_size() not in (1, 2, 4, 8):
            raise TypeError('nearest serves elements of 1, 2, 4 and 8 bytes, got %s' % p0.dtype)
    elif p0.dtype not in _DT:
        if p0.is_floating_point() or p0.is_complex():
            raise TypeError('the weighted methods serve float32, float64 and integers, got %s' % p0.dtype)
        planes = [t.to(torch.float64) for t in planes]
        p0 = planes[0]
    shape = list(p0.shape)
    shape[ay], shape[ax] = table_y.m, table_x.m
    if out is None:
        outs = [_empty_like_strides(p0, shape) for _ in planes]
    else:
        outs = [out] if torch.is_tensor(out) else list(out)
        if len(outs) != len(planes):
            raise ValueError('out must hold one tensor per plane')
        for o, t in zip(outs, planes):
            if (not torch.is_tensor(o) or list(o.shape) != shape or o.dtype != p0.dtype or o.device != dev):
                raise ValueError('out must be %s of %s on %s' % (tuple(shape), p0.dtype, dev))
            if any(s == 0 and n > 1 for s, n in zip(o.stride(), shape)):
                raise ValueError('an expanded out (stride 0) is not served')
            if _may_overlap(o, t):
                raise ValueError('out must not overlap its source')
    if fill is None:
        fill = float('nan') if (p0.is_floating_point() or p0.is_complex()) else 0
    if p0.numel() == 0 and outs[0].numel() > 0:
        raise ValueError('an empty source has nothing to resample')
    # the inner axis is the extra one closer in the destination; a second one is the batch
    o0 = outs[0]
    extra = sorted(extra, key=lambda d: -o0.stride(d))
    plane_ax = extra[0] if len(extra) == 2 else None
    inner_ax = extra[-1] if extra else None
    nplanes = p0.shape[plane_ax] if plane_ax is not None else 1
    inner = p0.shape[inner_ax] if inner_ax is not None else 1

    def strides(t):
        return _lib.i64_array([t.stride(plane_ax) if plane_ax is not None else 0, t.stride(ay), t.stride(ax),
                               t.stride(inner_ax) if inner_ax is not None else 0])

    L = _lib.lib()
    with torch.cuda.device(dev):
        ty, tx = table_y.to(dev), table_x.to(dev)
        if nearest:
            from ._device import _TORCH2NP
            if p0.dtype in _TORCH2NP:
                fill_bytes = np.array(fill).astype(_TORCH2NP[p0.dtype]).tobytes()
            elif fill == 0:
                fill_bytes = bytes(p0.element_size())
            else:
                raise TypeError('a fill other than 0 for %s elements is not served' % p0.dtype)
            fill_buf = C.create_string_buffer(fill_bytes, len(fill_bytes))
        for t, o in zip(planes, outs):
            args = [nplanes, inner, p0.shape[ay], p0.shape[ax], strides(t), table_y.m, table_x.m, strides(o)]
            if nearest:
                _lib.check(L.nd_amd_resample_nearest(
                    _ptr(t), _ptr(o), p0.element_size(), *args, _ptr(ty.start), _ptr(ty.count), _ptr(tx.start),
                    _ptr(tx.count), C.cast(fill_buf, C.c_void_p), _stream_ptr(dev)))
            else:
                _lib.check(L.nd_amd_resample(
                    _ptr(t), _ptr(o), _DT[p0.dtype], *args, _ptr(ty.start), _ptr(ty.count), _ptr(ty.weights), ty.taps,
                    _ptr(tx.start), _ptr(tx.count), _ptr(tx.weights), tx.taps, float(fill), _stream_ptr(dev)))
        _record(planes + outs + [ty.start, ty.count, ty.weights, tx.start, tx.count, tx.weights], dev)
    return outs[0] if single else outs


def resample_check_table(table, device=None):
    """Raise NdAmdError unless every run of the table lies inside its axis (nd_amd_resample_check_table;
    synchronises).  resample_axis builds tables that pass; this is for tables made elsewhere."""
    dev = table.device or _lib_device(device)
    with torch.cuda.device(dev):
        t = table.to(dev)
        _lib.check(_lib.lib().nd_amd_resample_check_table(_ptr(t.start), _ptr(t.count), t.m, t.n, t.taps,
                                                          _stream_ptr(dev)))


# ---------------------------------------------------------------------------
# speckle filters (include/nd_amd.h "Speckle filters"; tests/speckle_ref.py restates them)
# ---------------------------------------------------------------------------
SPECKLE_MAX_W = _lib.SPECKLE_MAX_W
SPECKLE_MAX_VARIABLES = _lib.SPECKLE_MAX_VARIABLES
SPECKLE_HOT_MAX_PLANES = _lib.SPECKLE_HOT_MAX_PLANES
SPECKLE_TILE = (_lib.SPECKLE_TILE_Y, _lib.SPECKLE_TILE_X)          # outputs a block owns: rows, columns
SPECKLE_HOT_TILE = (_lib.SPECKLE_HOT_TILE_Y, _lib.SPECKLE_TILE_X)  # the same in the one-launch multitemporal form


def speckle_window(w):
    """w as an int if it is an odd window of 1 ... SPECKLE_MAX_W samples, ValueError otherwise."""
    if isinstance(w, bool) or int(w) != w:
        raise ValueError('w must be an odd integer from 1 to %d, got %r' % (SPECKLE_MAX_W, w))
    w = int(w)
    if w < 1 or w % 2 == 0 or w > SPECKLE_MAX_W:
        raise ValueError('w must be an odd integer from 1 to %d, got %d' % (SPECKLE_MAX_W, w))
    return w


def multitemporal_looks(looks, k, w, variables=1):
    """Equivalent number of looks of MultitemporalFilter's output in homogeneous speckle of `looks` looks
    (Quegan & Yu 2001): M N L / (M + N - 1) with M = k * variables planes and N = w * w window samples."""
    m, n = float(k * variables), float(w * w)
    return m * n * float(looks) / (m + n - 1.0)


def _speckle_data(t, name):
    if not torch.is_tensor(t):
        raise TypeError('%s must be a torch.Tensor, got %r' % (name, type(t)))
    if not t.is_cuda:
        raise ValueError('%s must live on a ROCm device (got %s); nd_amd has no CPU path' % (name, t.device))
    if t.is_complex():
        raise TypeError('%s is complex: the speckle filters work on intensities' % name)
    if t.dtype not in _DT:
        if t.is_floating_point():
            raise TypeError('%s must be float32, float64 or an integer type, got %s' % (name, t.dtype))
        t = t.to(torch.float64)                       # integers are computed and returned as float64
    return t


def _speckle_out(out, like, name='out'):
    if out is None:
        return _empty_like_strides(like, list(like.shape))
    if (not torch.is_tensor(out) or out.shape != like.shape or out.dtype != like.dtype
            or out.device != like.device):
        raise ValueError('%s must be %s of %s on %s' % (name, tuple(like.shape), like.dtype, like.device))
    if any(s == 0 and n > 1 for s, n in zip(out.stride(), out.shape)):
        raise ValueError('an expanded %s (stride 0) is not served' % name)
    if _may_overlap(out, like):
        raise ValueError('%s must not overlap its source' % name)
    return out


def _speckle_plane_limit(ny, nx):
    if ny * nx >= 2 ** 31:
        raise NotImplementedError('planes of 2^31 pixels or more are not served (%d x %d)' % (ny, nx))


def speckle_lee(inp, w, looks, method='lee', out=None, dims=None):
    """The local-statistics speckle filter of Lee / Kuan over a w x w window of every (y, x) plane of `inp`
    (include/nd_amd.h has the definition).  inp: a ROCm tensor of float32 or float64 (integers are computed and
    returned as float64) whose axes `dims` names, 'y' and 'x' among them -- by default ('y', 'x') for two axes
    and ('time', 'y', 'x') for three; any strides, crops of larger tensors included.  looks: the ENL of the
    intensities, any positive real.  method: 'lee' or 'kuan'.  out: a tensor of the input's shape and type, any
    strides, not overlapping it.  -> out"""
    w = speckle_window(w)
    if method not in _lib.SPECKLE_METHODS:
        raise ValueError("method must be 'lee' or 'kuan', got %r" % (method,))
    if not float(looks) > 0 or not np.isfinite(1.0 / float(looks)):
        raise ValueError('looks must be positive, got %r' % (looks,))
    cu2 = 1.0 / float(looks)
    inp = _speckle_data(inp, 'inp')
    if dims is None:
        dims = {2: ('y', 'x'), 3: ('time', 'y', 'x')}.get(inp.dim())
        if dims is None:
            raise ValueError('dims must name the %d axes of inp' % inp.dim())
    dims = tuple(dims)
    if len(dims) != inp.dim() or len(set(dims)) != len(dims) or 'y' not in dims or 'x' not in dims:
        raise ValueError("dims must name the tensor's %d axes, 'y' and 'x' among them, got %r" % (inp.dim(), dims))
    ay, ax = dims.index('y'), dims.index('x')
    ny, nx = inp.shape[ay], inp.shape[ax]
    _speckle_plane_limit(ny, nx)
    out = _speckle_out(out, inp)
    dev = inp.device
    # the batch axis of a call is the last axis besides y and x; axes before it are walked on the host
    rest = [d for d in range(inp.dim()) if d not in (ay, ax)]
    order = rest + [ay, ax]
    src, dst = inp.permute(*order), out.permute(*order)
    if not rest:
        src, dst = src[None], dst[None]
    lead = src.shape[:-3]
    L = _lib.lib()
    with torch.cuda.device(dev):
        for idx in np.ndindex(*lead):
            s, d = src[idx], dst[idx]
            _lib.check(L.nd_amd_speckle_lee(_ptr(s), _ptr(d), _DT[inp.dtype], s.shape[0], ny, nx,
                                            _lib.i64_array(s.stride()), _lib.i64_array(d.stride()), w, cu2,
                                            _lib.SPECKLE_METHODS[method], _stream_ptr(dev)))
        _record([inp, out], dev)
    return out


def speckle_multitemporal(planes, w, dims=('time', 'y', 'x'), out=None):
    """The multitemporal speckle filter of Quegan & Yu 2001 over a w x w window and all dates (include/nd_amd.h
    has the definition).  planes: one ROCm tensor with the three axes `dims` names, or a list of up to
    SPECKLE_MAX_VARIABLES of them, which are filtered jointly, in the list's order within a date; float32 or
    float64 (integers are computed and returned as float64), any strides.  Up to SPECKLE_HOT_MAX_PLANES
    planes (dates x variables) are filtered in one launch, more in two passes with the same result.
    out: a tensor (or list) of the inputs' shape and type.  -> a tensor, or a list where a list was given."""
    w = speckle_window(w)
    single = torch.is_tensor(planes)
    planes = [planes] if single else list(planes)
    if not planes:
        return []
    planes = [_speckle_data(t, 'planes[%d]' % i) for i, t in enumerate(planes)]
    p0 = planes[0]
    dims = tuple(dims)
    if sorted(dims) != ['time', 'x', 'y'] or p0.dim() != 3:
        raise ValueError("dims must be a permutation of ('time', 'y', 'x') naming the three axes of the data")
    if len(planes) > SPECKLE_MAX_VARIABLES:
        raise NotImplementedError('%d variables: at most %d are filtered jointly'
                                  % (len(planes), SPECKLE_MAX_VARIABLES))
    for t in planes:
        if t.shape != p0.shape or t.dtype != p0.dtype or t.device != p0.device:
            raise NotImplementedError('variables filtered jointly share shape, type and device')
    at, ay, ax = dims.index('time'), dims.index('y'), dims.index('x')
    k, ny, nx = p0.shape[at], p0.shape[ay], p0.shape[ax]
    _speckle_plane_limit(ny, nx)
    if out is None:
        outs = [None] * len(planes)
    else:
        outs = [out] if torch.is_tensor(out) else list(out)
        if len(outs) != len(planes):
            raise ValueError('out must hold one tensor per variable')

    def same_strides(ts):
        return all(a == b for t in ts for a, b, n in zip(t.stride(), ts[0].stride(), t.shape) if n > 1)

    # one set of strides per call: variables that lie differently in memory are packed first
    if not same_strides(planes):
        planes = [t.contiguous() for t in planes]
        p0 = planes[0]
    outs = [_speckle_out(o, t, 'out[%d]' % i) for i, (o, t) in enumerate(zip(outs, planes))]
    given = outs
    if not same_strides(outs):
        outs = [torch.empty_like(p0, memory_format=torch.contiguous_format) for _ in planes]
    for o in outs:
        for t in planes:
            if _may_overlap(o, t):
                raise ValueError('out must not overlap a source')
    dev = p0.device
    nvar = len(planes)
    L = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(L.nd_amd_speckle_multitemporal_workspace_bytes(ny, nx, k, nvar))
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev) if nbytes else None
        src = (C.c_void_p * nvar)(*[t.data_ptr() for t in planes])
        dst = (C.c_void_p * nvar)(*[o.data_ptr() for o in outs])

        def strides(t):
            return _lib.i64_array([t.stride(at), t.stride(ay), t.stride(ax)])

        _lib.check(L.nd_amd_speckle_multitemporal(src, dst, nvar, _DT[p0.dtype], k, ny, nx, strides(p0),
                                                  strides(outs[0]), w, _ptr(work), nbytes, _stream_ptr(dev)))
        _record(planes + outs + [work], dev)
        for g, o in zip(given, outs):
            if g is not o:
                g.copy_(o)
    return given[0] if single else given


# ---------------------------------------------------------------------------
# regions of a map (include/nd_amd.h "Regions of a map"; scipy.ndimage.label pins the result,
# tests/regions_ref.py restates the by_value form)
# ---------------------------------------------------------------------------
_REGION_DT = {torch.bool: _lib.U8, torch.uint8: _lib.U8, torch.int32: _lib.I32, torch.int64: _lib.I64,
              torch.float32: _lib.F32, torch.float64: _lib.F64}
_REGION_NP = {torch.bool: np.uint8, torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64,
              torch.float32: np.float32, torch.float64: np.float64}
# The labelling's workspace (4 bytes per pixel and plane, 8 with area and for the sieve) is capped at this many
# bytes: a larger batch is walked in chunks of planes.  One plane is always served, whatever it takes.
REGIONS_WORKSPACE_CAP = 1 << 30


def region_element(value, dtype, name='background'):
    """`value` as one numpy element of the map's torch `dtype` (bool as uint8); ValueError if the type cannot hold it
    exactly.  NaN is held by the floating types."""
    if dtype not in _REGION_DT:
        raise TypeError('maps of bool, uint8, int32, int64, float32 and float64 are served, got %s' % (dtype,))
    npt = np.dtype(_REGION_NP[dtype])
    if isinstance(value, (bool, np.bool_)):
        value = int(value)
    bad = ValueError('%s = %r is not representable in %s' % (name, value, dtype))
    if npt.kind == 'f':
        with np.errstate(over='ignore', invalid='ignore'):
            e = npt.type(value)
        v = float(value)
        if not (v != v and e != e) and not (np.isfinite(e) == np.isfinite(v) and float(e) == v):
            raise bad
        return e
    if isinstance(value, (float, np.floating)):
        if value != value or value != int(value):
            raise bad
        value = int(value)
    value = int(value)
    info = np.iinfo(npt)
    if not info.min <= value <= (1 if dtype == torch.bool else info.max):
        raise bad
    return npt.type(value)


def _region_input(inp, dims, name='inp'):
    """-> (dims, ay, ax, ny, nx): the checks label_regions and sieve_regions share"""
    if not torch.is_tensor(inp):
        raise TypeError('%s must be a torch.Tensor, got %r' % (name, type(inp)))
    if not inp.is_cuda:
        raise ValueError('%s must live on a ROCm device (got %s); nd_amd has no CPU path' % (name, inp.device))
    if inp.is_complex():
        raise TypeError('%s is complex: regions are defined on real maps' % name)
    if inp.dtype not in _REGION_DT:
        raise TypeError('%s must be bool, uint8, int32, int64, float32 or float64, got %s' % (name, inp.dtype))
    if dims is None:
        dims = {2: ('y', 'x'), 3: ('time', 'y', 'x')}.get(inp.dim())
        if dims is None:
            raise ValueError('dims must name the %d axes of %s' % (inp.dim(), name))
    dims = tuple(dims)
    if len(dims) != inp.dim() or len(set(dims)) != len(dims) or 'y' not in dims or 'x' not in dims:
        raise ValueError("dims must name the tensor's %d axes, 'y' and 'x' among them, got %r" % (inp.dim(), dims))
    ay, ax = dims.index('y'), dims.index('x')
    ny, nx = inp.shape[ay], inp.shape[ax]
    if ny * nx >= 2 ** 31:
        raise NotImplementedError('planes of 2^31 pixels or more are not served (%d x %d)' % (ny, nx))
    return dims, ay, ax, ny, nx


def _region_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError('connectivity must be 4 or 8, got %r' % (connectivity,))
    return int(connectivity)


def _region_out(out, like, dtype, name, sources):
    if out is None:
        # the input's memory order, packed
        order = sorted(range(like.dim()), key=lambda d: (-like.stride(d), d))
        inv = [order.index(d) for d in range(like.dim())]
        return torch.empty([like.shape[d] for d in order], dtype=dtype, device=like.device).permute(*inv)
    if (not torch.is_tensor(out) or out.shape != like.shape or out.dtype != dtype or out.device != like.device):
        raise ValueError('%s must be %s of %s on %s' % (name, tuple(like.shape), dtype, like.device))
    if any(s == 0 and n > 1 for s, n in zip(out.stride(), out.shape)):
        raise ValueError('an expanded %s (stride 0) is not served' % name)
    if any(s < 0 for s in out.stride()):
        raise ValueError('%s has a negative stride' % name)
    for s in sources:
        if s is not None and _may_overlap(out, s):
            raise ValueError('%s must not overlap the input or another output' % name)
    return out


def _plane_batches(tensors, ay, ax):
    """every tensor (all of one shape) as (lead..., plane, y, x) views, and the index tuples of the leading axes: the
    batch axis of a call is the last axis besides y and x, axes before it are walked on the host"""
    t0 = tensors[0]
    rest = [d for d in range(t0.dim()) if d not in (ay, ax)]
    order = rest + [ay, ax]
    views = [None if t is None else t.permute(*order) for t in tensors]
    if not rest:
        views = [None if v is None else v[None] for v in views]
    return views, list(np.ndindex(*views[0].shape[:-3]))


def _region_chunks(nplanes, ny, nx, sizes):
    """plane ranges of a batch so that the workspace of each stays under REGIONS_WORKSPACE_CAP"""
    per_plane = ny * nx * (8 if sizes else 4) + 4 * (-(-ny * nx // 1024)) + 512
    step = max(1, min(nplanes, REGIONS_WORKSPACE_CAP // max(per_plane, 1)))
    return [(p, min(nplanes, p + step)) for p in range(0, nplanes, step)]


def _byte_view(t):
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def label_regions(inp, connectivity=4, background=0, by_value=False, dims=None, labels=None, area=None):
    """The connected regions of every (y, x) plane of `inp`, numbered from 1 in raster order of their first pixel
    (include/nd_amd.h "Regions of a map"; with by_value=False it is scipy.ndimage.label(inp != background)).
    inp: a ROCm tensor of bool, uint8, int32, int64, float32 or float64 whose axes `dims` names, 'y' and 'x' among
    them -- by default ('y', 'x') for two axes and ('time', 'y', 'x') for three; any non-negative strides.
    connectivity: 4 or 8.  background: the value that is no region (NaN never is one).  by_value: neighbours are
    joined only where their values are equal.  labels: an int32 tensor of the input's shape, any strides, not
    overlapping it.  area: True, or such a tensor, for the pixel count of every pixel's region as well.
    -> (labels, counts) or (labels, counts, area); counts is int64 with the input's shape without y and x: the
    number of regions of every plane.  Waits for the device."""
    dims, ay, ax, ny, nx = _region_input(inp, dims)
    conn = _region_connectivity(connectivity)
    bg = region_element(background, inp.dtype)
    dev = inp.device
    labels = _region_out(labels, inp, torch.int32, 'labels', [inp])
    want_area = area is not None and area is not False
    area = _region_out(None if area is True else area, inp, torch.int32, 'area', [inp, labels]) if want_area else None
    lead_shape = [n for d, n in enumerate(inp.shape) if d not in (ay, ax)]
    counts = torch.zeros(lead_shape, dtype=torch.int64, device=dev)
    if inp.numel() == 0:
        return (labels, counts, area) if want_area else (labels, counts)
    (src, lab, ar), lead = _plane_batches([_byte_view(inp), labels, area], ay, ax)
    cnt = counts.reshape(src.shape[:-2]) if lead_shape else counts.reshape(1)
    L = _lib.lib()
    bg_buf = np.array([bg])
    bgp = C.c_void_p(bg_buf.ctypes.data)
    with torch.cuda.device(dev):
        nplanes = src.shape[-3]
        chunks = _region_chunks(nplanes, ny, nx, want_area)
        nbytes = int(L.nd_amd_regions_workspace_bytes(chunks[0][1] - chunks[0][0], ny, nx, int(want_area)))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for idx in lead:
            s, l, c = src[idx], lab[idx], cnt[idx]
            a = ar[idx] if want_area else None
            for p0, p1 in chunks:
                _lib.check(L.nd_amd_label_regions(
                    _ptr(s[p0:p1]), _REGION_DT[inp.dtype], p1 - p0, ny, nx, _lib.i64_array(s.stride()), conn,
                    int(bool(by_value)), bgp, _ptr(l[p0:p1]), _lib.i64_array(l.stride()),
                    _ptr(a[p0:p1]) if want_area else None, _lib.i64_array(a.stride()) if want_area else None,
                    _ptr(c[p0:p1]), _ptr(work), nbytes, _stream_ptr(dev)))
        _record([inp, labels, area, counts, work], dev)
    return (labels, counts, area) if want_area else (labels, counts)


def region_sizes(labels, counts, dims=None):
    """The pixel count of every region of a labelling: `labels` and `counts` as label_regions returned them.
    -> (sizes, offsets): sizes is int32 with counts.sum() entries, the regions of plane p (in the order of counts'
    elements) at offsets[p] : offsets[p] + counts[p]; offsets is an int64 host array with one entry more than planes.
    It counts the labels; it does not label again."""
    dims, ay, ax, ny, nx = _region_input(labels, dims, 'labels')
    if labels.dtype != torch.int32:
        raise TypeError('labels must be int32, got %s' % labels.dtype)
    lead_shape = [n for d, n in enumerate(labels.shape) if d not in (ay, ax)]
    if not torch.is_tensor(counts) or list(counts.shape) != lead_shape:
        raise ValueError('counts must be the tensor label_regions returned: shape %s' % (tuple(lead_shape),))
    dev = labels.device
    host = counts.reshape(-1).to('cpu', torch.int64).numpy()
    if (host < 0).any():
        raise ValueError('counts must not be negative')
    offsets = np.concatenate(([0], np.cumsum(host))).astype(np.int64)
    total = int(offsets[-1])
    sizes = torch.zeros(total, dtype=torch.int32, device=dev)
    if total == 0 or labels.numel() == 0:
        return sizes, offsets
    (lab,), lead = _plane_batches([labels], ay, ax)
    nplanes = lab.shape[-3]
    off_dev = torch.from_numpy(offsets[:-1].copy()).to(dev).reshape(lab.shape[:-2])
    L = _lib.lib()
    with torch.cuda.device(dev):
        for n, idx in enumerate(lead):
            l = lab[idx]
            lo, hi = int(offsets[n * nplanes]), int(offsets[(n + 1) * nplanes])
            if hi == lo:
                continue
            # this batch's planes count into their own slice of sizes: offsets relative to its start
            rel = (off_dev[idx] - lo).contiguous()
            _lib.check(L.nd_amd_region_sizes(_ptr(l), _lib.i64_array(l.stride()), nplanes, ny, nx, _ptr(rel),
                                             _ptr(sizes[lo:hi]), hi - lo, _stream_ptr(dev)))
            _record([rel], dev)
        _record([labels, sizes], dev)
    return sizes, offsets


def sieve_regions(inp, min_size, connectivity=4, background=0, by_value=False, fill=None, dims=None, out=None):
    """`inp` with every region of fewer than `min_size` pixels replaced by `fill` (default: `background`); background
    pixels, NaN among them, keep their bits, and min_size <= 1 is a copy (include/nd_amd.h "Regions of a map").
    Arguments as for label_regions; out: a tensor of the input's shape and type, any strides, not overlapping it.
    -> out.  Waits for the device."""
    dims, ay, ax, ny, nx = _region_input(inp, dims)
    conn = _region_connectivity(connectivity)
    if isinstance(min_size, bool) or int(min_size) != min_size:
        raise ValueError('min_size must be an integer, got %r' % (min_size,))
    min_size = max(-1, min(int(min_size), 2 ** 62))
    bg = region_element(background, inp.dtype)
    fl = bg if fill is None else region_element(fill, inp.dtype, 'fill')
    out = _region_out(out, inp, inp.dtype, 'out', [inp])
    if inp.numel() == 0:
        return out
    dev = inp.device
    (src, dst), lead = _plane_batches([_byte_view(inp), _byte_view(out)], ay, ax)
    bg_buf, fill_buf = np.array([bg]), np.array([fl])
    L = _lib.lib()
    with torch.cuda.device(dev):
        nplanes = src.shape[-3]
        chunks = _region_chunks(nplanes, ny, nx, True)
        nbytes = int(L.nd_amd_regions_workspace_bytes(chunks[0][1] - chunks[0][0], ny, nx, 1)) if min_size > 1 else 0
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        for idx in lead:
            s, d = src[idx], dst[idx]
            for p0, p1 in chunks:
                _lib.check(L.nd_amd_sieve_regions(
                    _ptr(s[p0:p1]), _ptr(d[p0:p1]), _REGION_DT[inp.dtype], p1 - p0, ny, nx,
                    _lib.i64_array(s.stride()), _lib.i64_array(d.stride()), conn, int(bool(by_value)),
                    C.c_void_p(bg_buf.ctypes.data), C.c_void_p(fill_buf.ctypes.data), min_size, _ptr(work), nbytes,
                    _stream_ptr(dev)))
        _record([inp, out, work], dev)
    return out


# ---------------------------------------------------------------------------
# statistics of zones (include/nd_amd.h "Statistics of zones"; tests/zonal_ref.py restates it bit for bit)
# ---------------------------------------------------------------------------
ZONAL_STATS = ('count', 'nan_count', 'sum', 'min', 'max', 'm2', 'mean')
_ZONAL_OUT = ('count', 'nan_count', 'sum', 'min', 'max', 'm2')      # the order of nd_amd_zonal_stats' outputs


def zonal_ids(ids):
    """`ids` as a strictly increasing int64 numpy array; ValueError otherwise"""
    a = np.asarray(ids)
    if a.ndim == 1 and a.size == 0:
        return np.zeros(0, np.int64)
    if a.ndim != 1 or a.dtype.kind not in 'iu':
        raise ValueError('ids must be a one-dimensional list of integers, got %s %s' % (a.dtype, a.shape))
    if a.dtype.kind == 'u' and a.size and int(a.max()) >= 2 ** 63:
        raise ValueError('ids must fit an int64')
    a = a.astype(np.int64)
    if a.size > 1 and not (a[1:] > a[:-1]).all():
        raise ValueError('ids must be strictly increasing')
    return a


class ZonalIndex(object):
    """A label plane's zones as the statistics read them: keys (int32, (ny, nx): the zone's rank, n for no zone), perm
    (int32: the stable argsort of the keys), offsets (int64, n + 1: the keys below z), n, and ids (int64 numpy)."""

    def __init__(self, keys, perm, offsets, n, ids):
        self.keys, self.perm, self.offsets, self.n, self.ids = keys, perm, offsets, n, ids

    @property
    def shape(self):
        return tuple(self.keys.shape)


def _zonal_default_n(labels):
    """the largest label that is a positive whole number, 0 if there is none: one number read back"""
    if labels.numel() == 0:
        return 0
    if labels.dtype == torch.bool:
        return int(labels.any())
    if labels.is_floating_point():
        whole = (labels == labels.trunc()) & (labels.abs() < 2.0 ** 63)
        top = float(labels.masked_fill(~whole, 0).max())
        if top >= 2 ** 31 - 1:
            raise NotImplementedError('2^31 - 1 zones or more are not served (largest label %r)' % top)
        return max(int(top), 0)
    return max(int(labels.max()), 0)


def zonal_index(labels, ids=None, dims=None, n=None):
    """The zones of one label plane: a ROCm tensor of bool, uint8, int32, int64, float32 or float64 with the axes
    ('y', 'x') (dims: their order), any non-negative strides.  ids: a strictly increasing list of integer zone ids;
    by default 1 .. the largest label.  A pixel belongs to the zone whose id its label equals, every other pixel
    (0, NaN, 2.5, a label not listed) to none.  -> ZonalIndex.  The keys come from nd_amd_zonal_keys; the stable sort
    and the search between the two entries are torch's, on the device.  n: with ids=None, the zones are 1 .. n (a
    caller that labels several planes alike); without it the call reads the largest label back and waits for the
    device."""
    dims = ('y', 'x') if dims is None else tuple(dims)
    if torch.is_tensor(labels) and labels.dim() != 2:
        raise ValueError('labels must be one plane with the axes y and x, got %d axes' % labels.dim())
    dims, ay, ax, ny, nx = _region_input(labels, dims, 'labels')
    dev = labels.device
    lab = _byte_view(labels).permute(ay, ax)
    if ids is None:
        if n is not None and (isinstance(n, bool) or int(n) != n or n < 0):
            raise ValueError('n must be a non-negative integer, got %r' % (n,))
        n = _zonal_default_n(lab) if n is None else int(n)
        host_ids = np.arange(1, n + 1, dtype=np.int64)
        ids_dev = None
    else:
        host_ids = zonal_ids(ids)
        n = len(host_ids)
        ids_dev = torch.from_numpy(host_ids).to(dev) if n else None
    if n >= 2 ** 31 - 1:
        raise NotImplementedError('2^31 - 1 zones or more are not served (%d)' % n)
    with torch.cuda.device(dev):
        keys = torch.empty((ny, nx), dtype=torch.int32, device=dev)
        if keys.numel():
            _lib.check(_lib.lib().nd_amd_zonal_keys(_ptr(lab), _REGION_DT[labels.dtype], ny, nx,
                                                    _lib.i64_array(lab.stride()), _ptr(ids_dev), n, _ptr(keys),
                                                    _stream_ptr(dev)))
            _record([labels, ids_dev, keys], dev)
        ordered, perm = torch.sort(keys.reshape(-1), stable=True)
        offsets = torch.searchsorted(ordered, torch.arange(n + 1, dtype=torch.int32, device=dev)).to(torch.int64)
        return ZonalIndex(keys, perm.to(torch.int32), offsets, n, host_ids)


def _zonal_values(values, index, dims, name='values'):
    if not isinstance(index, ZonalIndex):
        raise TypeError('index must come from zonal_index, got %r' % type(index))
    dims, ay, ax, ny, nx = _region_input(values, dims, name)
    if (ny, nx) != index.shape:
        raise ValueError('%s has planes of %d x %d, the zones of %d x %d' % ((name, ny, nx) + index.shape))
    if values.device != index.keys.device:
        raise ValueError('%s and the index live on different devices' % name)
    return dims, ay, ax, ny, nx


def zonal_stats(values, index, dims=None, stats=('count', 'mean', 'min', 'max', 'm2')):
    """Statistics of every (y, x) plane of `values` inside every zone of `index` (zonal_index): a ROCm tensor whose
    axes `dims` names as for label_regions, float32 or float64 (other types are computed as float64), any non-negative
    strides.  stats: names among ZONAL_STATS.  -> a dict of tensors shaped (the axes besides y and x..., n): int64
    counts, float64 for the rest.  NaN values are skipped and counted; every sum is formed in the zone's fixed tree, so
    the bytes do not depend on the layout, the other zones or the number of planes."""
    stats = tuple(stats)
    for s in stats:
        if s not in ZONAL_STATS:
            raise ValueError('stats must be among %s, got %r' % (ZONAL_STATS, s))
    dims, ay, ax, ny, nx = _zonal_values(values, index, dims)
    if not values.is_floating_point():
        values = values.to(torch.float64)
    dev, n = values.device, index.n
    want = set(stats) | ({'sum', 'count'} if 'mean' in stats else set())
    (src,), lead = _plane_batches([values], ay, ax)
    shape = tuple(src.shape[:-2]) + (n,)
    with torch.cuda.device(dev):
        out = {s: torch.empty(shape, dtype=torch.int64 if s in ('count', 'nan_count') else torch.float64, device=dev)
               for s in _ZONAL_OUT if s in want}
        nplanes = src.shape[-3]
        if n and src.numel():
            L = _lib.lib()
            nbytes = int(L.nd_amd_zonal_workspace_bytes(nplanes, ny, nx, n))
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            for idx in lead:
                s = src[idx]
                _lib.check(L.nd_amd_zonal_stats(
                    _ptr(s), _DT[values.dtype], nplanes, ny, nx, _lib.i64_array(s.stride()), _ptr(index.perm),
                    _ptr(index.offsets), n, *[_ptr(out[k][idx]) if k in out else None for k in _ZONAL_OUT],
                    _ptr(work), nbytes, _stream_ptr(dev)))
            _record([values, work, index.perm, index.offsets] + list(out.values()), dev)
        elif n:                                         # zones, and no pixel: what a zone without a participant gets
            for k, t in out.items():
                t.fill_(float('nan') if k in ('min', 'max') else 0)
        if 'mean' in stats:
            out['mean'] = out['sum'] / out['count'].to(torch.float64)
    res = {s: out[s] for s in stats}
    if values.dim() == 2:
        res = {s: t[0] for s, t in res.items()}
    return res


def zonal_paint(table, index, like=None, out=None, keep=False, fill=None, dims=None):
    """Every pixel of zone z gets table[..., z]: table is a float64 ROCm tensor shaped (the axes besides y and x..., n),
    as zonal_stats returns.  like: a float32 or float64 tensor whose shape, type and memory order the result takes, and
    with keep=True the values of the pixels of no zone; out: the result's tensor, any strides.  Pixels of no zone get
    `fill` (default NaN) unless keep.  -> out."""
    ref = out if like is None else like
    if ref is None:
        raise ValueError('like or out must be given')
    dims, ay, ax, ny, nx = _zonal_values(ref, index, dims, 'like' if like is not None else 'out')
    if ref.dtype not in _DT:
        raise TypeError('painted planes are float32 or float64, got %s' % ref.dtype)
    if keep and like is None:
        raise ValueError('keep=True needs `like`: the values of the pixels of no zone')
    dev, n = ref.device, index.n
    out = _region_out(out, ref, ref.dtype, 'out', [like if keep else None])
    fillv = float('nan') if fill is None else float(fill)
    (dst, src), lead = _plane_batches([out, like if keep else None], ay, ax)
    shape = tuple(dst.shape[:-2]) + (n,)
    if not torch.is_tensor(table) or table.dtype != torch.float64 or table.device != dev:
        raise ValueError('table must be a float64 tensor on %s' % dev)
    if out.dim() == 2:
        table = table[None]
    if tuple(table.shape) != shape:
        raise ValueError('table must be shaped %s, got %s' % (shape, tuple(table.shape)))
    if out.numel() == 0:
        return out
    table = table.contiguous()
    L = _lib.lib()
    with torch.cuda.device(dev):
        nplanes = dst.shape[-3]
        for idx in lead:
            d = dst[idx]
            s = src[idx] if keep else None
            _lib.check(L.nd_amd_zonal_paint(
                _ptr(index.keys), _ptr(table[idx]) if n else None, nplanes, ny, nx, n, _ptr(s) if keep else None,
                _lib.i64_array(s.stride()) if keep else None, _ptr(d), _lib.i64_array(d.stride()), _DT[out.dtype],
                fillv, _stream_ptr(dev)))
        _record([table, index.keys, like, out], dev)
    return out


# ---------------------------------------------------------------------------
# statistics along time (include/nd_amd.h "Statistics along time"; tests/temporal_ref.py restates it bit for bit)
# ---------------------------------------------------------------------------
TEMPORAL_STATS = ('count', 'nan_count', 'sum', 'mean', 'min', 'max', 'argmin', 'argmax', 'm2', 'var', 'std', 'cv',
                  'median')
# the order of nd_amd_temporal_stats' outputs
_TEMPORAL_OUT = ('count', 'nan_count', 'sum', 'mean', 'min', 'max', 'argmin', 'argmax', 'm2', 'var', 'std', 'cv',
                 'median')
_TEMPORAL_INT = ('count', 'nan_count', 'argmin', 'argmax')
_TEMPORAL_T = ('min', 'max', 'median')
# the longest series the register form holds, and the longest whose order statistics are served (the LDS form)
TEMPORAL_REG_MAX = {torch.float32: _lib.TEMPORAL_REG_MAX[_lib.F32], torch.float64: _lib.TEMPORAL_REG_MAX[_lib.F64]}
TEMPORAL_LDS_MAX = {torch.float32: _lib.TEMPORAL_LDS_MAX[_lib.F32], torch.float64: _lib.TEMPORAL_LDS_MAX[_lib.F64]}


def temporal_percentiles(q):
    """`q` (None, a number or a sequence of numbers) as a tuple of floats in [0, 100]; ValueError otherwise"""
    if q is None:
        return ()
    values = [q] if np.ndim(q) == 0 else list(q)
    out = []
    for p in values:
        if isinstance(p, (bool, str)) or not np.isreal(p) or not 0 <= float(p) <= 100:
            raise ValueError('q must be numbers in [0, 100], got %r' % (p,))
        out.append(float(p))
    names = [temporal_percentile_name(p) for p in out]
    if len(set(names)) != len(names):
        raise ValueError('q holds percentiles that share a name (%s): each is named with %%g'
                         % ', '.join(sorted(n for n in set(names) if names.count(n) > 1)))
    return tuple(out)


def _temporal_in_form(form):
    """nd_amd_temporal_stats_in_form (temporal.hip; in no header) with `form` bound: the tests' way to one kernel form"""
    fn = _lib.lib().nd_amd_temporal_stats_in_form
    if fn.argtypes is None:
        fn.restype = C.c_int
        fn.argtypes = list(_lib.lib().nd_amd_temporal_stats.argtypes[:-1]) + [C.c_int, C.c_void_p]
    return lambda *args: fn(*(args[:-1] + (_lib.TEMPORAL_FORMS[form], args[-1])))


def temporal_percentile_name(p):
    """the key of percentile p in temporal_stats' result: 'p2', 'p97.5'"""
    return 'p%g' % p


def temporal_stats(x, stats=('mean', 'std'), q=(), skipna=True, ddof=0, axis=0, _form='auto'):
    """Per-pixel statistics along axis `axis` of a 3-D ROCm tensor with any non-negative strides: the other two axes,
    in their order, are (y, x), so a (time, y, x) stack has axis=0 and a (y, x, time) stack axis=2; both are read where
    they lie.  float32 and float64 are computed as they are, every other real type as float64.  stats: names among
    TEMPORAL_STATS; q: percentiles in [0, 100].  -> a dict of (ny, nx) tensors: the statistics by name, percentile p as
    temporal_percentile_name(p); min, max, median and percentiles of the type computed in, count, nan_count, argmin
    and argmax int32, the rest float64.  Order statistics of series longer than TEMPORAL_LDS_MAX raise
    NotImplementedError; the moments are served for every length.  `_form` names one kernel form for the tests."""
    stats = (stats,) if isinstance(stats, str) else tuple(stats)
    for s in stats:
        if s not in TEMPORAL_STATS:
            raise ValueError('stats must be among %s, got %r' % (TEMPORAL_STATS, s))
    q = temporal_percentiles(q)
    if isinstance(ddof, bool) or int(ddof) != ddof or ddof < 0:
        raise ValueError('ddof must be a non-negative integer, got %r' % (ddof,))
    if not isinstance(x, torch.Tensor):
        raise TypeError('x must be a torch.Tensor, got %r' % type(x))
    if x.is_complex():
        raise TypeError('x is complex: statistics along time are defined on real data')
    if x.dim() != 3:
        raise ValueError('x must have three axes (the series and y, x), got %d' % x.dim())
    if not x.is_cuda:
        raise ValueError('x must live on a ROCm device (got %s); nd_amd has no CPU path' % x.device)
    if x.dtype not in _DT:
        x = x.to(torch.float64)
    axis = axis % 3
    view = x.movedim(axis, 0)
    k, ny, nx = view.shape
    if k < 1:
        raise ValueError('the series has no date')
    if (('median' in stats or q) and k > TEMPORAL_LDS_MAX[x.dtype]
            and not (_form == 'register' and k <= TEMPORAL_REG_MAX[x.dtype])):
        raise NotImplementedError('order statistics of %s series are served up to %d dates (TEMPORAL_LDS_MAX), got %d'
                                  % (x.dtype, TEMPORAL_LDS_MAX[x.dtype], k))
    dev = x.device
    with torch.cuda.device(dev):
        out = {s: torch.empty((ny, nx), dtype=torch.int32 if s in _TEMPORAL_INT else
                              (x.dtype if s in _TEMPORAL_T else torch.float64), device=dev)
               for s in _TEMPORAL_OUT if s in stats}
        pct = torch.empty((len(q), ny, nx), dtype=x.dtype, device=dev) if q else None
        if ny * nx:
            entry = _lib.lib().nd_amd_temporal_stats if _form == 'auto' else _temporal_in_form(_form)
            _lib.check(entry(
                _ptr(view), _DT[x.dtype], k, ny, nx, _lib.i64_array(view.stride()), int(bool(skipna)), int(ddof),
                (C.c_double * len(q))(*q) if q else None, len(q),
                *([_ptr(out[s]) if s in out else None for s in _TEMPORAL_OUT] + [_ptr(pct) if q else None]),
                _stream_ptr(dev)))
            _record([x, pct] + list(out.values()), dev)
    res = {s: out[s] for s in stats}
    for j, p in enumerate(q):
        res[temporal_percentile_name(p)] = pct[j]
    return res


def _lib_device(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError('nd_amd needs a ROCm GPU: the compute path is HIP only')
    return torch.device('cuda', torch.cuda.current_device())
