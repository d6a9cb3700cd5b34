"""
nd_amd/filters.py -- the reference's filter classes (nd/filters.py) with the arithmetic on the GPU.

  Filter             dataset marshalling of nd/filters.py:82-198 (per-variable or stacked-variable
                     application, complex handling, dimension reordering), unchanged in meaning;
                     `_filter(self, arr, axes, output)` still writes in place into `output`.
  ConvolutionFilter  scipy.ndimage.convolve semantics (nd/filters.py:205-267) -> nd_amd_correlate
  BoxcarFilter       ones/w**N kernel (nd/filters.py:277-298)
  NLMeansFilter      nd/filters.py:388-466 -> nd_amd_nlmeans3d
  GaussianFilter     nd/filters.py:308-378 -> scipy.ndimage.gaussian_filter restated as one
                     nd_amd_correlate1d pass per filtered axis
  LeeFilter          extension (no reference counterpart): Lee / Kuan local statistics -> nd_amd_speckle_lee
  MultitemporalFilter  extension: Quegan & Yu 2001 over all dates -> nd_amd_speckle_multitemporal

Arrays may be numpy (copied to the device and back: the drop-in case) or torch ROCm tensors
(device-resident pipelines, no host copies).
"""
from abc import abstractmethod

import numpy as np
import torch

from . import _adapter, _device, _lib, kernels
from .algorithm import Algorithm, parallelize, wrap_algorithm
from .io import assemble_complex, disassemble_complex

__all__ = ['Filter', 'ConvolutionFilter', 'convolution', 'BoxcarFilter', 'boxcar',
           'GaussianFilter', 'gaussian', 'NLMeansFilter', 'nlmeans', 'LeeFilter', 'lee',
           'MultitemporalFilter', 'multitemporal', 'multitemporal_looks', '_expand_kernel']


def _expand_kernel(kernel, kernel_dims, new_dims):
    """View `kernel` (one axis per entry of `kernel_dims`) as an array with one axis per entry of
    `new_dims`, length 1 on the axes it does not span.  Same contract and error messages as
    nd/filters.py:36-75 (its test: nd/tests/test_filters_common.py)."""
    missing = [d for d in kernel_dims if d not in new_dims]
    if missing:
        raise ValueError('`new_dims` must be a superset of `kernel_dims`.')
    if len(kernel_dims) != kernel.ndim:
        raise ValueError('The length of `kernel_dims` must match the dimension of `kernel`.')
    extent = dict(zip(kernel_dims, kernel.shape))
    return kernel.reshape([extent.get(d, 1) for d in new_dims])


def _largest_dim(ds, dims):
    return max(dims, key=lambda d: ds.sizes[d])


def _split_dimension(filt, ds):
    """Dimension to cut when a filter is applied in chunks: the longest one the filter does not
    touch (no halo needed), else the longest one overall."""
    free = [d for d in ds.dims if d not in filt.dims]
    return _largest_dim(ds, free or list(ds.dims))


class Filter(Algorithm):
    """Common dataset handling of all filters (the marshalling of nd/filters.py:82-198).

    A subclass sets `dims` (names of the dimensions it filters along) and implements
    `_filter(arr, axes, output)`, which filters the plain array `arr` along the integer `axes`
    and stores the result in `output` (same shape and dtype, never aliased with `arr`).

    Class attributes
      per_variable      True: `_filter` sees one variable at a time.  False: it sees all variables
                        that carry `dims`, stacked along a trailing 'variable' axis, with the filter
                        dimensions leading.
      supports_complex  False: complex variables are presented as `<name>__re` / `<name>__im`.
    """

    per_variable = True
    supports_complex = False
    dims = ()

    @abstractmethod
    def __init__(self, *args, **kwargs):
        return

    @parallelize
    def apply(self, ds, inplace=False):
        """Filter a Dataset or DataArray and return the filtered copy; variables that lack one of
        `self.dims` pass through untouched.  `inplace=True` is rejected like in the reference
        (nd/filters.py:121-123)."""
        if inplace:
            raise NotImplementedError('Inplace filtering is not currently implemented.')
        staged = self._stage_on_device(ds)
        work = ds if staged is None else staged
        split_complex = (not self.supports_complex) and _adapter.is_complex(work)
        private = staged is not None
        if split_complex and not private and self._device_resident(work):
            # Device-resident nd_amd.xr_lite data: split a shallow copy instead of the caller's dataset -- nothing to
            # undo afterwards (re-assembling `ds` was three passes over every complex variable) -- and pack the two
            # halves of a contiguous complex tensor in one pass (nd_amd_split_complex) instead of handing the filter
            # two strided views, each of which it would pack by itself (GaussianFilter on a (time, y, x) dataset
            # with a complex64 C12, 12 x 1024 x 2048: 1.05 -> 0.6 ms).  Same values, same variable names and order.
            work = work.copy(deep=False)
            private = True
        if split_complex:
            # on `ds` itself like the reference does (and undoes below), or on a private copy, which leaves the
            # caller's dataset alone altogether
            disassemble_complex(work, inplace=True)
            if private:
                self._pack_split_halves(work)
        if isinstance(work, _adapter.namespace(work).DataArray):
            result = self._apply_array(work)
        elif self.per_variable:
            result = self._apply_each(work)
        else:
            result = self._apply_stacked(work)
        if staged is not None:
            result = self._fetch_to_host(result, ds)
        elif split_complex and not private:
            # the caller's dataset gets its complex variables back; the result keeps the split
            # form, as it does in the reference (nd/filters.py:186-188)
            assemble_complex(ds, inplace=True)
        return result

    @staticmethod
    def _device_resident(ds):
        from . import xr_lite
        if _adapter.namespace(ds) is not xr_lite or isinstance(ds, xr_lite.DataArray):
            return False
        return all(_device.is_tensor(v.values) for v in ds.data_vars.values())

    @staticmethod
    def _pack_split_halves(ds):
        """`<name>__re` / `<name>__im` that are the two strided views of one contiguous complex device tensor:
        both packed in one pass over it."""
        from .io import SPLIT_SUFFIXES
        for name in list(ds.data_vars):
            if not name.endswith(SPLIT_SUFFIXES[0]):
                continue
            stem = name[:-len(SPLIT_SUFFIXES[0])]
            other = stem + SPLIT_SUFFIXES[1]
            if other not in ds.data_vars:
                continue
            re, im = ds[name], ds[other]
            if not (_device.is_tensor(re.values) and _device.is_tensor(im.values)):
                continue
            pair = kernels.split_complex(re.values, im.values)
            if pair is not None:
                ds[name] = (tuple(re.dims), pair[0], re.attrs)
                ds[other] = (tuple(im.dims), pair[1], im.attrs)

    def _stage_on_device(self, ds):
        """Host-resident nd_amd.xr_lite data: upload every variable the filter touches once, in its
        own layout, and let the device-resident path do all the re-ordering (stacking, transposes)
        at HBM speed -- on the host the same steps run at 1-2 GB/s.  None = leave `ds` as it is
        (already on the device, or an xarray object, whose variables must stay numpy)."""
        from . import xr_lite
        if _adapter.namespace(ds) is not xr_lite:
            return None
        if isinstance(ds, xr_lite.DataArray):
            if _device.is_tensor(ds.values):
                return None
            dev = _device.device_of(ds.values)
            return xr_lite.DataArray(_device.to_device(ds.values, dev), ds.dims, ds.coords, ds.attrs,
                                     ds.name)
        names = _adapter.get_vars_for_dims(ds, self.dims)
        if not names or any(_device.is_tensor(ds[n].values) for n in names):
            return None
        dev = _device.device_of(*[ds[n].values for n in names])
        out = ds.copy(deep=False)
        for n in names:
            out[n] = (tuple(ds[n].dims), _device.to_device(ds[n].values, dev), ds[n].attrs)
        return out

    def _fetch_to_host(self, result, ds):
        """Results of a staged run back as numpy (page-locked downloads for large arrays)."""
        from . import xr_lite
        if isinstance(result, xr_lite.DataArray):
            return xr_lite.DataArray(_device.to_host(result.values), result.dims, result.coords,
                                     result.attrs, result.name)
        for n in list(result.data_vars):
            if _device.is_tensor(result[n].values):
                result[n] = (tuple(result[n].dims), _device.to_host(result[n].values),
                             result[n].attrs)
        return result

    def _axes_in(self, dims):
        return tuple(dims.index(d) for d in self.dims)

    # `_filter` overwrites every element of its output, so the result starts from uninitialised
    # buffers instead of the reference's deep copy of the input (a host copy of the whole dataset
    # would cost more than the filter); variables that are not filtered are still copied.
    def _apply_array(self, da):
        out = _adapter.empty_like(da)
        self._filter(da.values, self._axes_in(out.dims), output=out.values)
        return out

    def _apply_each(self, ds):
        out = ds.copy(deep=False)
        names = _adapter.get_vars_for_dims(ds, self.dims)
        for name in ds.data_vars:
            if name in names:
                target = _adapter.empty_like(ds[name])
                self._filter(ds[name].values, self._axes_in(target.dims), output=target.values)
                out[name] = target
            else:
                out[name] = ds[name].copy(deep=True)
        return out

    def _apply_stacked(self, ds):
        names = _adapter.get_vars_for_dims(ds, self.dims)
        passthrough = _adapter.get_vars_for_dims(ds, self.dims, invert=True)
        order = self.dims + tuple(d for d in ds.dims if d not in self.dims) + ('variable',)
        stacked = ds[names].to_array().transpose(*order)
        filtered = _adapter.empty_like(stacked)
        self._filter(stacked.values, self._axes_in(stacked.dims), output=filtered.values)
        out = _adapter.expand_variables(filtered)
        for name in list(out.data_vars):
            out[name] = out[name].transpose(*ds[name].dims)      # original axis order
        for name in passthrough:
            out[name] = ds[name]
        return out

    @abstractmethod
    def _filter(self, arr, axes, output=None):
        """Filter `arr` along `axes` into `output`."""
        return


# ---- convolution -----------------------------------------------------------------------------

def _convolve_into(arr, nd_kernel, output, device=None, **kwargs):
    """scipy.ndimage.convolve(arr, nd_kernel, output=output, **kwargs) on the GPU (real dtype)."""
    unknown = set(kwargs) - {'mode', 'cval', 'origin'}
    if unknown:
        raise TypeError('unsupported scipy.ndimage.convolve arguments: %s' % sorted(unknown))
    dev = _device.device_of(arr, output, device=device)
    dtype = _device.np_dtype(arr)
    with torch.cuda.device(dev):
        t = _device.to_device(arr, dev)
        if dtype not in (np.float32, np.float64):
            # scipy accumulates in double and casts to the array dtype on store
            raise TypeError('convolution on the GPU supports float32/float64 arrays, got %s' % dtype)
        squeeze = 0
        k = np.asarray(nd_kernel, np.float64)
        if t.dim() > 4:
            # fold leading axes the kernel does not span
            lead = t.dim() - 4
            if any(s != 1 for s in k.shape[:lead + 1]):
                raise NotImplementedError('kernels spanning more than 4 array axes')
            shape = t.shape
            t = t.reshape((-1,) + tuple(shape[lead + 1:]))
            k = k.reshape((1,) + k.shape[lead + 1:])
            squeeze = shape
        out_t = output if (_device.is_tensor(output) and not squeeze) else torch.empty_like(t)
        kernels.convolve(t, k, out=out_t, **kwargs)
        if squeeze:
            out_t = out_t.reshape(squeeze)
        if out_t is not output:
            _device.write_back(out_t, output)
    return output


class ConvolutionFilter(Filter):
    """Convolution with an arbitrary kernel, per variable (nd/filters.py:205-267).

    dims    names of the dataset dimensions the kernel axes refer to, in kernel-axis order
            (default ('y', 'x')); `len(dims)` must equal `kernel.ndim`
    kernel  array of weights; `None` means the identity (a single 1)
    kwargs  passed on with scipy.ndimage.convolve's meaning: `mode` (default 'reflect'), `cval`,
            `origin`

    Complex variables are filtered as two real arrays.  Results are those of
    scipy.ndimage.convolve, bit for bit (tests/test_correlate_gpu.py)."""

    per_variable = True
    supports_complex = True
    kwargs = {}

    def __init__(self, dims=('y', 'x'), kernel=None, **kwargs):
        self.dims = tuple(dims)
        self.kernel = np.ones((1,) * len(self.dims)) if kernel is None else np.asarray(kernel)
        self.kwargs = kwargs

    def _parallel_dimension(self, ds):
        return _split_dimension(self, ds)

    def _buffer(self, dim):
        """Rows of context a chunk needs on each side along `dim`: half the kernel extent."""
        return self.kernel.shape[self.dims.index(dim)] // 2 if dim in self.dims else 0

    def _filter(self, arr, axes, output):
        shape = [1] * arr.ndim
        for axis, n in zip(axes, self.kernel.shape):
            shape[axis] = n
        nd_kernel = self.kernel.reshape(shape)
        if (self.kernel.size == 1 and float(np.real(self.kernel.flat[0])) == 1.0 and np.imag(self.kernel.flat[0]) == 0
                and not self.kwargs.get('origin') and _device.is_tensor(arr) and _device.is_tensor(output)):
            # the default kernel (a single 1, nd/filters.py:226-227): scipy's `tmp = 1.0 * v` in double, cast back, is
            # the value itself in every dtype and layout -- one copy instead of a round trip through the planar layout
            output.copy_(arr)
            return
        if not _adapter.iscomplexobj(arr):
            _convolve_into(arr, nd_kernel, output, **self.kwargs)
        elif _device.is_tensor(arr):
            halves_in = torch.view_as_real(arr).unbind(-1)
            # a contiguous complex variable whose window axes come last (time-first data): split
            # it in one pass, filter two packed arrays, merge in one pass -- instead of packing
            # and scattering each strided half separately
            tail_window = all(n == 1 for n in nd_kernel.shape[:-2]) if arr.ndim >= 2 else False
            pair = kernels.split_complex(*halves_in) if (tail_window and _device.is_tensor(output)
                                                          and output.is_contiguous()
                                                          and arr.numel() >= (1 << 16)) else None
            if pair is not None:
                done = [torch.empty_like(pair[0]), torch.empty_like(pair[1])]
                for part_in, part_out in zip(pair, done):
                    _convolve_into(part_in, nd_kernel, part_out, **self.kwargs)
                if kernels.merge_complex(done[0], done[1], output):
                    return
                for part, part_out in zip(done, torch.view_as_real(output).unbind(-1)):
                    part_out.copy_(part)
                return
            # interleaved complex memory seen as two strided real views
            for part_in, part_out in zip(halves_in, torch.view_as_real(output).unbind(-1)):
                _convolve_into(part_in, nd_kernel, part_out, **self.kwargs)
        else:
            # host complex array: one upload and one download of the interleaved data, the two
            # halves are filtered as strided views on the device
            dev = _device.device_of(arr, output)
            with torch.cuda.device(dev):
                t = _device.to_device(arr, dev)
                o = torch.empty_like(t)
                for part_in, part_out in zip(torch.view_as_real(t).unbind(-1),
                                             torch.view_as_real(o).unbind(-1)):
                    _convolve_into(part_in, nd_kernel, part_out, **self.kwargs)
                _device.write_back(o, output)


convolution = wrap_algorithm(ConvolutionFilter, 'convolution')


class BoxcarFilter(ConvolutionFilter):
    """Moving average over a `w`-wide window along each of `dims` (nd/filters.py:277-298): a
    ConvolutionFilter whose kernel is constant, `1 / w**len(dims)` in float64.  Use an odd `w` for
    a centred window; `kwargs` as for ConvolutionFilter."""

    def __init__(self, dims=('y', 'x'), w=3, **kwargs):
        ndim = len(dims)
        ConvolutionFilter.__init__(self, dims, np.ones((w,) * ndim, dtype=np.float64) / w**ndim,
                                   **kwargs)


boxcar = wrap_algorithm(BoxcarFilter, 'boxcar')


# ---- Gaussian --------------------------------------------------------------------------------

class GaussianFilter(Filter):
    """Gaussian smoothing with scipy.ndimage.gaussian_filter's semantics (nd/filters.py:308-378).

    dims    dimensions to smooth along (default ('y', 'x'))
    sigma   standard deviation in samples: one number for all of `dims`, or one per dimension
    kwargs  `mode`, `cval`, `truncate` as in scipy"""

    def __init__(self, dims=('y', 'x'), sigma=1, **kwargs):
        self.dims = tuple(dims)
        self.sigma = [sigma] * len(self.dims) if np.isscalar(sigma) else sigma
        self.kwargs = kwargs

    def _parallel_dimension(self, ds):
        return _split_dimension(self, ds)

    def _buffer(self, dim):
        """scipy truncates the kernel at 4 sigma: radius int(4 sigma + 0.5)."""
        if dim not in self.dims:
            return 0
        return int(4.0 * self.sigma[self.dims.index(dim)] + 0.5)

    def _filter(self, arr, axes, output):
        unknown = set(self.kwargs) - {'mode', 'cval', 'truncate'}
        if unknown:
            raise TypeError('unsupported scipy.ndimage.gaussian_filter arguments: %s'
                            % sorted(unknown))
        per_axis = [0] * arr.ndim                     # sigma 0 = axis left alone
        for axis, value in zip(axes, self.sigma):
            per_axis[axis] = value
        dev = _device.device_of(arr, output)
        with torch.cuda.device(dev):
            t = _device.to_device(arr, dev)
            if _device.np_dtype(arr) not in (np.float32, np.float64):
                raise TypeError('GaussianFilter on the GPU supports float32/float64 arrays')
            out_t = output if _device.is_tensor(output) else torch.empty_like(t)
            if out_t.data_ptr() == t.data_ptr():
                t = t.clone()
            # a variable in the reference's (y, x, time) layout smoothed along y and x: transpose
            # to planar on the device, filter there (x contiguous: the tiled passes), transpose back
            if t.dim() == 3 and per_axis[2] == 0 and t.numel() >= (1 << 16):
                planar = torch.empty((t.shape[2], t.shape[0], t.shape[1]), dtype=t.dtype, device=dev)
                if kernels.relayout_planar(t, planar):
                    smooth = kernels.gaussian_filter(planar, [0, per_axis[0], per_axis[1]], **self.kwargs)
                    if not kernels.relayout_pixel_major(smooth, out_t):
                        out_t.copy_(smooth.permute(1, 2, 0))
                    if out_t is not output:
                        _device.write_back(out_t, output)
                    return
            kernels.gaussian_filter(t, per_axis, out=out_t, **self.kwargs)
            if out_t is not output:
                _device.write_back(out_t, output)


gaussian = wrap_algorithm(GaussianFilter, 'gaussian')


# ---- non-local means -------------------------------------------------------------------------

class NLMeansFilter(Filter):
    """Non-local means over up to three dimensions, weights shared by all variables
    (nd/filters.py:388-466; kernel: nd/_filters.pyx:320-420).

    dims     dimensions that span the search window and the patches
    r        search radius: one number, or one per entry of `dims` (0 = do not search along it)
    sigma    noise standard deviation: patch distances below 2 sigma^2 count as zero
    h        decay of the weights with patch distance
    f        patch radius, applied along every dimension whose r is non-zero
    n_eff    target effective sample size; the weight of the centre pixel is solved for it
             (-1: the centre pixel gets the largest neighbour weight)
    patch_distances
             'reference' (default) is what the compiled reference computes on 64-bit platforms:
             its patch loops run over range(-f, f+1) with an UNSIGNED f, which is empty for f > 0,
             so every pixel of the search window gets weight 1 (nd/_filters.c:3539-3553).
             'signed' evaluates the patch distances the source text describes."""

    per_variable = False

    def __init__(self, dims=('y', 'x'), r=1, sigma=1, h=1, f=1, n_eff=-1,
                 patch_distances='reference'):
        if patch_distances not in ('reference', 'signed'):
            raise ValueError("patch_distances must be 'reference' or 'signed'")
        self.dims = tuple(dims)
        radii = [r] * len(self.dims) if np.isscalar(r) else list(r)
        self.r = np.asarray(radii).astype(np.uint32)
        self.f = np.where(self.r > 0, f, 0).astype(np.uint32)
        self.sigma, self.h, self.n_eff = sigma, h, n_eff
        self.patch_distances = patch_distances

    def _parallel_dimension(self, ds):
        return _split_dimension(self, ds)

    def _buffer(self, dim):
        """A chunk needs search radius + patch radius rows of context."""
        if dim not in self.dims:
            return 0
        i = self.dims.index(dim)
        return int(self.r[i]) + int(self.f[i])

    def _filter(self, arr, axes, output):
        # The kernel works on (d0, d1, d2, variable).  Like the reference (nd/filters.py:447-463,
        # which never looks at `axes`) the filter dimensions are taken to be the leading axes and
        # the variable axis the last one; missing axes are added in front with radius 0, unused
        # trailing ones get radius 0 too.
        lead, trail = 4 - arr.ndim, arr.ndim - 1 - len(self.r)
        r = np.array([0] * lead + list(self.r) + [0] * trail, dtype=np.uint32)
        f = np.array([0] * lead + list(self.f) + [0] * trail, dtype=np.uint32)
        dev = _device.device_of(arr, output)
        with torch.cuda.device(dev):
            t = _device.to_device(arr, dev)
            t4 = t[(None,) * (4 - t.dim())]
            # The tiled kernels want planar memory (variable outermost) with the last windowed
            # axis contiguous; datasets arrive with the variable axis fastest or -- stacked from
            # the reference's (y, x, time) variables -- with time fastest.  Re-lay the data out on
            # the device when that is the case: through the transpose kernels where each variable
            # is a (y, x, time)-ordered block, through a torch copy otherwise.
            if r[2] == 0 and f[2] == 0:
                fwd, back = (3, 2, 0, 1), (2, 3, 1, 0)       # memory (var, axis2, axis0, axis1)
                fast = t4.stride(1) == 1
            else:
                fwd, back = (3, 0, 1, 2), (1, 2, 3, 0)       # memory (var, axis0, axis1, axis2)
                fast = t4.stride(2) == 1
            # (float64 as well since round 6: the reference's own test datasets are float64 (y, x, time) variables,
            #  and NLMeansFilter() with its defaults on such a dataset took the per-pixel kernel -- 87 ms where the
            #  time-first layout takes 1.5 ms)
            relayout = (not fast) and t4.dtype in (torch.float32, torch.float64) and t4.numel() >= (1 << 14)
            pm = 0 if self.patch_distances == 'reference' else 1
            if not relayout:
                out4 = (output[(None,) * (4 - output.dim())] if _device.is_tensor(output)
                        else torch.empty_like(t4))
                kernels.pixelwise_nlmeans_3d(t4, out4, r, f, self.sigma, self.h, self.n_eff,
                                             patch_mode=pm)
            else:
                pv = t4.permute(*fwd)                                      # (var, A, B, C) view
                planar = torch.empty(pv.shape, dtype=t4.dtype, device=dev)
                if not all(kernels.relayout_planar(pv[v].permute(1, 2, 0), planar[v])
                           for v in range(pv.shape[0])):
                    planar.copy_(pv)
                planar_out = torch.empty_like(planar)
                kernels.pixelwise_nlmeans_3d(planar.permute(*back), planar_out.permute(*back), r, f,
                                             self.sigma, self.h, self.n_eff, patch_mode=pm)
                out4 = planar_out.permute(*back)
                if _device.is_tensor(output):
                    ov = output[(None,) * (4 - output.dim())].permute(*fwd)
                    if all(kernels.relayout_pixel_major(planar_out[v], ov[v].permute(1, 2, 0))
                           for v in range(ov.shape[0])):
                        return
            if _device.is_tensor(output):
                if out4.data_ptr() != output.data_ptr():
                    output.copy_(out4.reshape(output.shape))
            else:
                _device.write_back(out4.reshape(t.shape), output)


nlmeans = wrap_algorithm(NLMeansFilter, 'nlmeans')


# ---- adaptive speckle filters ----------------------------------------------------------------

multitemporal_looks = kernels.multitemporal_looks


def _is_integer(values):
    if _device.is_tensor(values):
        return not (values.is_floating_point() or values.is_complex())
    return np.asarray(values).dtype.kind in 'iub'


def _as_float64(values):
    return values.to(torch.float64) if _device.is_tensor(values) else np.asarray(values).astype(np.float64)


def _replace_values(da, values):
    """`da` with other values (possibly of another dtype), everything else kept."""
    from . import xr_lite
    if _adapter.namespace(da) is xr_lite:
        return xr_lite.DataArray(values, da.dims, da.coords, da.attrs, da.name)
    return da.copy(deep=False, data=values)


class _SpeckleFilter(Filter):
    """What LeeFilter and MultitemporalFilter share: they filter intensities, so a complex variable is an error
    (raised before Filter.apply would split it into two real halves and filter those), and integers are computed
    and returned as float64."""

    window_dims = ()

    def apply(self, ds, inplace=False, *, njobs=1, devices=None):
        self._check(ds)
        return Filter.apply(self, ds, inplace=inplace, njobs=njobs, devices=devices)

    apply.__doc__ = Filter.apply.__doc__

    def _touched(self, ds):
        if _adapter.is_dataarray(ds):
            return [ds]
        return [ds[n] for n in _adapter.get_vars_for_dims(ds, self.dims)]

    def _check(self, ds):
        for v in self._touched(ds):
            if _adapter.iscomplexobj(v.values):
                raise TypeError('%s filters intensities, variable %r is complex: filter |z|^2 or the covariance '
                                'diagonal, or split it knowingly with io.disassemble_complex'
                                % (type(self).__name__, v.name))

    def _buffer(self, dim):
        """Rows of context a chunk needs on each side along `dim`: half the window."""
        return self.w // 2 if dim in self.window_dims else 0

    def _run(self, da):
        src = _as_float64(da.values) if _is_integer(da.values) else da.values
        blank = torch.empty_like(src) if _device.is_tensor(src) else np.empty_like(src)
        self._filter(src, self._axes_in(tuple(da.dims)), output=blank)
        return _replace_values(da, blank)

    def _apply_array(self, da):
        return self._run(da)

    def _apply_each(self, ds):
        out = ds.copy(deep=False)
        names = _adapter.get_vars_for_dims(ds, self.dims)
        for name in ds.data_vars:
            out[name] = self._run(ds[name]) if name in names else ds[name].copy(deep=True)
        return out

    @staticmethod
    def _on_device(arr, output, run):
        """run(t, out_t) with `arr` on the device and a device output; host in means host out."""
        dev = _device.device_of(arr, output)
        with torch.cuda.device(dev):
            t = _device.to_device(arr, dev)
            out_t = output if _device.is_tensor(output) else torch.empty_like(t)
            run(t, out_t)
            if out_t is not output:
                _device.write_back(out_t, output)


def _pixel_major_through_planar(t, out_t, axes_yx, run):
    """(y, x, time) data that the transpose kernels take: filter a planar copy (lanes along x) and transpose the
    result back.  -> False where the data is not of that kind and nothing was done."""
    if t.dim() != 3 or tuple(axes_yx) != (0, 1) or t.numel() < (1 << 16):
        return False
    planar = torch.empty((t.shape[2], t.shape[0], t.shape[1]), dtype=t.dtype, device=t.device)
    if not kernels.relayout_planar(t, planar):
        return False
    done = run(planar)
    if not kernels.relayout_pixel_major(done, out_t):
        out_t.copy_(done.permute(1, 2, 0))
    return True


class LeeFilter(_SpeckleFilter):
    """The local-statistics speckle filter of Lee (1980) and Kuan et al. (1985) over a `w` x `w` window, per
    variable and per plane (README "Speckle filters" has the definition).  An extension: the reference has none.

    dims    the two window dimensions (default ('y', 'x'))
    w       odd window width, 1 to 31
    looks   equivalent number of looks of the intensities, any positive real
    method  'lee': b = 1 - Cu^2 / Cx^2;  'kuan': the same divided by 1 + Cu^2

    The output feeds Classifier and to_rgb.  It is no longer gamma distributed with `looks` looks: OmnibusTest
    keeps taking the unfiltered (or multilooked) stack."""

    def __init__(self, dims=('y', 'x'), w=7, looks=1, method='lee'):
        self.dims = tuple(dims)
        if len(self.dims) != 2:
            raise ValueError('LeeFilter works on two window dimensions, got %r' % (self.dims,))
        self.window_dims = self.dims
        self.w = kernels.speckle_window(w)
        if not float(looks) > 0 or not np.isfinite(1.0 / float(looks)):
            raise ValueError('looks must be positive, got %r' % (looks,))
        if method not in ('lee', 'kuan'):
            raise ValueError("method must be 'lee' or 'kuan', got %r" % (method,))
        self.looks, self.method = float(looks), method

    def _parallel_dimension(self, ds):
        return _split_dimension(self, ds)

    def _filter(self, arr, axes, output):
        names = ['d%d' % d for d in range(np.ndim(arr))]
        names[axes[0]], names[axes[1]] = 'y', 'x'

        def run(t, out_t):
            def planar(p):
                return kernels.speckle_lee(p, self.w, self.looks, self.method, dims=('time', 'y', 'x'))
            if not _pixel_major_through_planar(t, out_t, axes, planar):
                kernels.speckle_lee(t, self.w, self.looks, self.method, out=out_t, dims=names)

        self._on_device(arr, output, run)


lee = wrap_algorithm(LeeFilter, 'lee')


class MultitemporalFilter(_SpeckleFilter):
    """The multitemporal speckle filter of Quegan & Yu (2001): every date is replaced by its `w` x `w` local
    mean times the average over all dates of the ratio of the date to its local mean.  It trades the time axis
    for looks without losing spatial resolution (README "Speckle filters" has the definition).  An extension.

    dims    the two window dimensions (default ('y', 'x'))
    w       odd window width, 1 to 31
    time    name of the date dimension; variables without it pass through
    joint   True: one ratio average over all (up to 4) variables that carry `time` and `dims`, which must share
            type, shape and dims.  False: one variable at a time.

    multitemporal_looks(looks, k, w, variables) is the ENL of the output in homogeneous speckle.  The output is
    no longer gamma distributed and its dates are correlated: OmnibusTest keeps taking the unfiltered stack."""

    def __init__(self, dims=('y', 'x'), w=7, time='time', joint=False):
        self.window_dims = tuple(dims)
        if len(self.window_dims) != 2 or time in self.window_dims:
            raise ValueError('MultitemporalFilter works on two window dimensions and `time`, got %r and %r'
                             % (self.window_dims, time))
        self.time = time
        self.dims = self.window_dims + (time,)       # `_axes_in` hands `_filter` the time axis as well
        self.w = kernels.speckle_window(w)
        self.joint = bool(joint)
        self.per_variable = not self.joint

    def _parallel_dimension(self, ds):
        """The longer window dimension, never `time`: a chunk in time would change the average over the dates."""
        return _largest_dim(ds, self.window_dims)

    def _check(self, ds):
        if self.time not in ds.dims:
            raise KeyError('MultitemporalFilter needs the dimension %r; the data has %s'
                           % (self.time, tuple(ds.dims)))
        _SpeckleFilter._check(self, ds)
        touched = self._touched(ds)
        for v in touched:
            if len(v.dims) != 3:
                raise NotImplementedError('variable %r has dims %s: (time, y, x) in any order is served'
                                          % (v.name, tuple(v.dims)))
        if self.joint and not _adapter.is_dataarray(ds):
            if len(touched) > kernels.SPECKLE_MAX_VARIABLES:
                raise NotImplementedError('joint=True over %d variables: at most %d are served'
                                          % (len(touched), kernels.SPECKLE_MAX_VARIABLES))
            v0 = touched[0] if touched else None
            for v in touched:
                if (tuple(v.dims) != tuple(v0.dims) or tuple(v.shape) != tuple(v0.shape)
                        or _device.np_dtype(v.values) != _device.np_dtype(v0.values)):
                    raise NotImplementedError('joint=True needs variables of one type, shape and dims; %r and %r '
                                              'differ' % (v0.name, v.name))

    def _names(self, axes, ndim):
        names = [None] * ndim
        names[axes[0]], names[axes[1]], names[axes[2]] = 'y', 'x', 'time'
        return names

    def _filter(self, arr, axes, output):
        names = self._names(axes, np.ndim(arr))

        def run(t, out_t):
            def planar(p):
                return kernels.speckle_multitemporal(p, self.w, dims=('time', 'y', 'x'))
            if not _pixel_major_through_planar(t, out_t, axes[:2], planar):
                kernels.speckle_multitemporal(t, self.w, dims=names, out=out_t)

        self._on_device(arr, output, run)

    def _apply_stacked(self, ds):
        """joint=True: the variables' tensors go to the kernel where they lie, nothing is stacked."""
        names = _adapter.get_vars_for_dims(ds, self.dims)
        out = ds.copy(deep=False)
        if names:
            v0 = ds[names[0]]
            dims = self._names(self._axes_in(tuple(v0.dims)), 3)
            values = [ds[n].values for n in names]
            dev = _device.device_of(*values)
            with torch.cuda.device(dev):
                planes = [_device.to_device(v, dev) for v in values]
                done = kernels.speckle_multitemporal(planes, self.w, dims=dims)
                for n, v, t in zip(names, values, done):
                    out[n] = _replace_values(ds[n], t if _device.is_tensor(v) else _device.to_host(t))
        for n in ds.data_vars:
            if n not in names:
                out[n] = ds[n].copy(deep=True)
        return out


multitemporal = wrap_algorithm(MultitemporalFilter, 'multitemporal')
