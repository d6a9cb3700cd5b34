"""
nd_amd/warp.py -- Coregistration (nd/warp.py:1104-1163) and, within one coordinate system, Resample, Reprojection
and Alignment (nd/warp.py:872-1097) with the arithmetic on the GPU.

  Coregistration  every date of a stack aligned to a reference date.  The shift of each date's C11
                  plane against the reference's (skimage.registration.phase_cross_correlation with
                  upsample_factor=upsampling, scikit-image 0.18) -> nd_amd_coregister_shifts; every
                  variable with the dimensions time, y and x translated by it (skimage.transform.warp,
                  bicubic, 0 outside, clipped to the plane's input range) -> nd_amd_warp_translate.

  get_transform / get_resolution / get_bounds   the coordinate-based arithmetic of nd/warp.py:175-251 as plain
                  tuples (no affine / rasterio objects): what nd_amd.vector.rasterize places its grid with.

  Resample / Reprojection / Alignment   a dataset brought onto another rotation-free grid of the same coordinate
                  system: every output pixel a separable weighted sum of source pixels ('nearest', 'bilinear',
                  'cubic', 'average'; the definition is this project's, README.md "Resampling and reprojection")
                  -> nd_amd_resample / nd_amd_resample_nearest.  (time, y, x) and (y, x, time) variables are read
                  where they lie.  A change of CRS, rotated transforms and rasterio's other methods are not served.
  get_common_bounds / get_common_resolution   nd/warp.py:395-487 as plain tuples.

Arrays may be numpy (copied to the device and back) or torch ROCm tensors (the result stays on the device).
"""
import math
import operator
import warnings
from collections import OrderedDict

import numpy as np

from . import _adapter, _device, kernels
from .algorithm import Algorithm, wrap_algorithm
from .io import disassemble_complex

__all__ = ['Coregistration', 'coregister', 'get_transform', 'get_resolution', 'get_bounds',
           'Resample', 'resample', 'Reprojection', 'reproject', 'Alignment', 'align',
           'get_common_bounds', 'get_common_resolution']

NAN_MESSAGE = ('NaN values found, please remove NaNs from your input data or use the '
               '`reference_mask`/`moving_mask` keywords, eg: phase_cross_correlation(reference_image, '
               'moving_image, reference_mask=~np.isnan(reference_image), '
               'moving_mask=~np.isnan(moving_image))')


class Coregistration(Algorithm):
    """Coregister a time series (stack) of images to a master image.

    At the moment only supports coregistration by translation.

    Parameters
    ----------
    reference : int, optional
        The time index to use as reference for coregistration (default: 0).
    upsampling : int, optional
        The upsampling factor for shift estimation (default: 10).
    """

    def __init__(self, reference=0, upsampling=10):
        self.reference = reference
        self.upsampling = upsampling

    def apply(self, ds):
        """Apply the coregistration to a dataset and return the coregistered copy (complex variables
        disassembled into `<name>__re` / `<name>__im`, as in the reference).  Raises ValueError, like
        skimage, when a NaN in C11 reaches the correlation."""
        return _coregister(ds, reference=self.reference, upsampling=self.upsampling)


def _planar_view(t, dims):
    """(tensor, layout, inverse permutation) for a (time, a, b) or (a, b, time) variable; any other
    order is copied into (time, a, b) and the result viewed back in the variable's own order."""
    if dims[0] == 'time':
        return t.contiguous(), 'planar', None
    if dims[-1] == 'time':
        return t.contiguous(), 'pixel_major', None
    at = dims.index('time')
    perm = [at] + [i for i in range(3) if i != at]
    inv = [perm.index(i) for i in range(3)]
    return t.permute(*perm).contiguous(), 'planar', inv


def _coregister(ds, reference, upsampling, ref_var='C11'):
    import torch
    ds_new = disassemble_complex(ds)
    if ref_var not in ds_new.data_vars:
        raise KeyError(ref_var)
    names = _adapter.get_vars_for_dims(ds_new, ['time', 'x', 'y'])
    if ref_var not in names:
        raise ValueError("'%s' must have the dimensions time, y and x" % ref_var)
    k = ds_new[ref_var].sizes['time']
    ref = operator.index(reference)
    if not -k <= ref < k:
        raise IndexError('reference %d is out of bounds for %d dates' % (ref, k))
    ref %= k
    upsampling = operator.index(upsampling)
    if not 1 <= upsampling <= 128:
        raise ValueError('upsampling must be in [1, 128], got %d' % upsampling)
    for n in names:
        da = ds_new[n]
        if len(da.dims) != 3:
            raise ValueError("'%s' has dimensions %s: Coregistration handles (time, y, x) variables only"
                             % (n, tuple(da.dims)))
        dt = _device.np_dtype(da.values)
        if dt not in (np.float32, np.float64):
            raise TypeError("'%s' is %s: Coregistration serves float32 and float64 data only" % (n, dt))
    host = {n: not _device.is_tensor(ds_new[n].values) for n in names}
    dev = _device.device_of(*[ds_new[n].values for n in names])
    with torch.cuda.device(dev):
        vals = {n: _device.to_device(ds_new[n].values, dev) for n in names}
        c11 = ds_new[ref_var]
        shifts, status = kernels.coregister_shifts(vals[ref_var], ref, upsampling, dims=tuple(c11.dims))
        # one warp call per (dtype, layout, shape) group of variables
        groups = {}
        for n in names:
            t, layout, inv = _planar_view(vals[n], tuple(ds_new[n].dims))
            groups.setdefault((t.dtype, layout, tuple(t.shape)), []).append((n, t, inv))
        out = {}
        for (_, layout, _), members in groups.items():
            res = kernels.warp_translate([t for _, t, _ in members], shifts, ref, layout)
            for (n, _, inv), r in zip(members, res):
                out[n] = r if inv is None else r.permute(*inv)
        if bool(status.any().item()):
            raise ValueError(NAN_MESSAGE)
    for n in names:
        da = ds_new[n]
        v = _device.to_host(out[n].contiguous()) if host[n] else out[n]
        ds_new[n] = (tuple(da.dims), v, da.attrs)
    return ds_new


coregister = wrap_algorithm(Coregistration, 'coregister')


# ---- the grid of a dataset, read off its x / y coordinates ----------------------------------------------------
def _xy_coords(ds):
    """the x and y coordinate arrays (float64) where the dataset has both with at least two entries, else None"""
    coords = getattr(ds, 'coords', {})
    if 'x' in coords and 'y' in coords:
        x = np.asarray(getattr(coords['x'], 'values', coords['x']), dtype=np.float64)
        y = np.asarray(getattr(coords['y'], 'values', coords['y']), dtype=np.float64)
        if x.ndim == 1 and y.ndim == 1 and len(x) > 1 and len(y) > 1:
            return x, y
    return None


def _attrs_transform(ds):
    t = getattr(ds, 'attrs', {}).get('transform')
    if t is None:
        raise ValueError('the dataset has neither x / y coordinates (two or more each) nor attrs[\'transform\']')
    t = tuple(float(v) for v in tuple(t)[:6])
    if len(t) != 6:
        raise ValueError("attrs['transform'] must hold the six terms (a, b, c, d, e, f), got %r" % (t,))
    return t


def get_transform(ds):
    """The geographic transform of a dataset as the 6-tuple (a, b, c, d, e, f) of nd.warp.get_transform
    (nd/warp.py:175-199): from the coordinates, a = (x[-1] - x[0]) / (len(x) - 1), c = x[0], e and f likewise
    from y, b = d = 0 -- x[0] / y[0] taken as the corner of pixel (0, 0), as the reference passes it on.  Falls
    back to attrs['transform']; ValueError without either."""
    xy = _xy_coords(ds)
    if xy is None:
        return _attrs_transform(ds)
    x, y = xy
    resx = (x[-1] - x[0]) / (len(x) - 1)
    resy = (y[-1] - y[0]) / (len(y) - 1)
    return (float(resx), 0.0, float(x[0]), 0.0, float(resy), float(y[0]))


def get_resolution(ds):
    """(|a|, |e|): the pixel size along x and y in the units of the coordinates, as nd.warp.get_resolution
    (nd/warp.py:202-224)."""
    xy = _xy_coords(ds)
    if xy is None:
        t = _attrs_transform(ds)
        return (abs(t[0]), abs(t[4]))
    x, y = xy
    return (float(abs(x[-1] - x[0]) / (len(x) - 1)), float(abs(y[-1] - y[0]) / (len(y) - 1)))


def get_bounds(ds):
    """(left, bottom, right, top) in the units of the coordinates: the smallest and largest x and y values, as
    nd.warp.get_bounds
    (nd/warp.py:227-251); from attrs['transform'] and the raster's size where there are no coordinates."""
    xy = _xy_coords(ds)
    if xy is not None:
        x, y = xy
        return (float(x.min()), float(y.min()), float(x.max()), float(y.max()))
    a, _, c, _, e, f = _attrs_transform(ds)
    nx, ny = int(ds.sizes['x']), int(ds.sizes['y'])
    xs, ys = (c, c + a * nx), (f, f + e * ny)
    return (min(xs), min(ys), max(xs), max(ys))


# ---- Resample, Reprojection, Alignment: a dataset on another grid of the same coordinate system ---------------------
RESAMPLINGS = ('nearest', 'bilinear', 'cubic', 'average')
# the names of rasterio.warp.Resampling this package does not serve
_OTHER_RESAMPLINGS = ('cubic_spline', 'lanczos', 'mode', 'gauss', 'max', 'min', 'med', 'q1', 'q3', 'sum', 'rms')


def _check_resampling(resampling):
    if resampling is None or resampling in RESAMPLINGS:
        return resampling
    name = getattr(resampling, 'name', resampling)          # a rasterio.warp.Resampling member
    if name in RESAMPLINGS:
        return name
    if name in _OTHER_RESAMPLINGS:
        raise NotImplementedError("resampling=%r is not served: one of %s" % (name, RESAMPLINGS))
    raise ValueError('resampling must be None or one of %s, got %r' % (RESAMPLINGS, resampling))


def _check_grid(transform, what='transform'):
    t = tuple(float(v) for v in tuple(transform)[:6])
    if len(t) != 6:
        raise ValueError('%s must hold the six terms (a, b, c, d, e, f), got %r' % (what, transform))
    if t[1] != 0.0 or t[3] != 0.0:
        raise ValueError('%s is rotated (b = %r, d = %r): only rotation-free grids are served' % (what, t[1], t[3]))
    if not all(math.isfinite(v) for v in t) or t[0] == 0.0 or t[4] == 0.0:
        raise ValueError('%s needs finite terms and pixel sizes other than 0, got %r' % (what, t))
    return t


def _res_pair(res):
    rx, ry = (res, res) if np.ndim(res) == 0 else tuple(res)
    rx, ry = float(rx), float(ry)
    if not (rx > 0.0 and ry > 0.0 and math.isfinite(rx) and math.isfinite(ry)):
        raise ValueError('res must be positive, got %r' % (res,))
    return rx, ry


def resample_grid(transform, ny, nx, res=None, width=None, height=None):
    """The grid Resample puts a (ny, nx) raster on: it covers the raster's full extent, c_s ... c_s + a_s * nx and
    f_s ... f_s + e_s * ny, with the signs of a_s and e_s kept.  res (a float or (rx, ry)) wins over width / height:
    W = max(1, floor(|a_s| * nx / rx + 0.5)), a_d = sign(a_s) * rx.  Otherwise a_d = a_s * nx / W; with one of
    width and height the other keeps the aspect ratio (nd/warp.py:635-638); with neither the grid is unchanged.
    -> (transform, H, W)"""
    a, _, c, _, e, f = _check_grid(transform)
    ny, nx = int(ny), int(nx)
    if res is not None:
        rx, ry = _res_pair(res)
        W = max(1, int(math.floor(abs(a) * nx / rx + 0.5)))
        H = max(1, int(math.floor(abs(e) * ny / ry + 0.5)))
        return (math.copysign(rx, a), 0.0, c, 0.0, math.copysign(ry, e), f), H, W
    if width is None and height is None:
        return (a, 0.0, c, 0.0, e, f), ny, nx
    if width is None:
        width = int(nx * height / ny)
    elif height is None:
        height = int(ny * width / nx)
    W, H = operator.index(width), operator.index(height)
    if W < 1 or H < 1:
        raise ValueError('width and height must be at least 1, got %d and %d' % (W, H))
    return (a * nx / W, 0.0, c, 0.0, e * ny / H, f), H, W


def reproject_grid(src_transform, ny, nx, transform=None, extent=None, res=None, width=None, height=None):
    """The grid Reprojection puts a (ny, nx) raster on.  transform with width and height: as given.  extent =
    (left, bottom, right, top) with res: W = int(|right - left| / rx) + 1 and H likewise (nd/warp.py:668-671), the
    resolution with the source's signs; with width and height: a_d = +-(right - left) / W.  The origin is `left`
    for a_s > 0, else `right`, and `top` for e_s < 0, else `bottom`.  Without transform and extent: resample_grid.
    -> (transform, H, W)"""
    a, _, c, _, e, f = _check_grid(src_transform, 'the source transform')
    if transform is not None:
        if width is None or height is None:
            raise ValueError('If `transform` is given, you must also specify the `width` and `height` arguments.')
        W, H = operator.index(width), operator.index(height)
        if W < 1 or H < 1:
            raise ValueError('width and height must be at least 1, got %d and %d' % (W, H))
        return _check_grid(transform), H, W
    if extent is None:
        return resample_grid(src_transform, ny, nx, res=res, width=width, height=height)
    left, bottom, right, top = (float(v) for v in extent)
    if res is not None:
        rx, ry = _res_pair(res)
        W = int(abs((right - left) / rx)) + 1
        H = int(abs((top - bottom) / ry)) + 1
    elif width is not None and height is not None:
        W, H = operator.index(width), operator.index(height)
        if W < 1 or H < 1:
            raise ValueError('width and height must be at least 1, got %d and %d' % (W, H))
        rx, ry = abs(right - left) / W, abs(top - bottom) / H
    else:
        raise ValueError('Need to provide either `width` and `height` or resolution when specifying the extent.')
    return (math.copysign(rx, a), 0.0, left if a > 0 else right, 0.0,
            math.copysign(ry, e), top if e < 0 else bottom), H, W


def _grid_of(ds):
    """(transform, ny, nx) of a dataset with y and x"""
    sizes = ds.sizes
    if 'y' not in sizes or 'x' not in sizes:
        raise ValueError('the dataset needs the dimensions y and x')
    return _check_grid(get_transform(ds), "the dataset's transform"), int(sizes['y']), int(sizes['x'])


def _plain_coords(ds, ns):
    """the coordinates that do not run along y or x (those are made anew; 2-D ones are not carried over)"""
    from . import xr_lite
    out = OrderedDict()
    for k, v in ds.coords.items():
        if ns is xr_lite:
            if k not in ('y', 'x') and np.ndim(v) <= 1:
                out[k] = v
        elif not {'y', 'x'} & set(v.dims):
            out[k] = v
    return out


def _regrid_values(values, dims, tables, fill=None):
    """one variable's array through kernels.resample; more than two axes besides y and x are flattened into one"""
    extra = [d for d in dims if d not in ('y', 'x')]
    if len(extra) <= 2:
        return kernels.resample(values, tables[0], tables[1], dims=tuple(dims), fill=fill)
    order = [dims.index(d) for d in extra] + [dims.index('y'), dims.index('x')]
    inv = [order.index(i) for i in range(len(dims))]
    flat = values.permute(*order)
    lead = tuple(flat.shape[:-2])
    out = kernels.resample(flat.reshape((-1,) + tuple(flat.shape[-2:])), tables[0], tables[1],
                           dims=('time', 'y', 'x'), fill=fill)
    return out.reshape(lead + tuple(out.shape[-2:])).permute(*inv)


def _regrid(ds, dst, H, W, resampling=None):
    """`ds` on the grid (dst, H, W).  Every variable with y and x is resampled where it lies; variables with
    neither pass through; complex variables come back as `<name>__re` / `<name>__im`."""
    import torch
    ns = _adapter.namespace(ds)
    was_array = isinstance(ds, ns.DataArray)
    resampling = _check_resampling(resampling)
    dst = _check_grid(dst, 'the destination transform')
    H, W = int(H), int(W)
    ds_new = disassemble_complex(ds)
    src, ny, nx = _grid_of(ds_new)
    todo = []
    for n in ds_new.data_vars:
        dims = tuple(ds_new[n].dims)
        if 'y' in dims and 'x' in dims:
            todo.append(n)
        elif 'y' in dims or 'x' in dims:
            raise NotImplementedError("'%s' has dimensions %s: variables with only one of y and x are not served"
                                      % (n, dims))
    coords = _plain_coords(ds_new, ns)
    coords['x'] = dst[2] + dst[0] * np.arange(W, dtype=np.float64)
    coords['y'] = dst[5] + dst[4] * np.arange(H, dtype=np.float64)
    attrs = OrderedDict(ds_new.attrs)
    attrs['transform'] = dst
    for key, n in (('lines', H), ('samples', W)):
        if key in attrs:
            attrs[key] = n
    out = ns.Dataset(coords=coords, attrs=attrs)
    results = {}
    if todo:
        dev = _device.device_of(*[ds_new[n].values for n in todo])
        with torch.cuda.device(dev):
            tables = {}                                 # one pair per method, uploaded once for all its variables
            for n in todo:
                da = ds_new[n]
                kind = _device.np_dtype(da.values).kind
                method = resampling or ('nearest' if kind in 'biu' else 'bilinear')
                if method not in tables:
                    tables[method] = (kernels.resample_axis(ny, H, (src[4], src[5]), (dst[4], dst[5]), method).to(dev),
                                      kernels.resample_axis(nx, W, (src[0], src[2]), (dst[0], dst[2]), method).to(dev))
                host = not _device.is_tensor(da.values)
                r = _regrid_values(_device.to_device(da.values, dev), tuple(da.dims), tables[method])
                results[n] = _device.to_host(r.contiguous()) if host else r
    for n in ds_new.data_vars:
        da = ds_new[n]
        out[n] = (tuple(da.dims), results[n] if n in results else da.values, da.attrs)
    if was_array and len(out.data_vars) == 1:
        return out[list(out.data_vars)[0]]
    return out


class Resample(Algorithm):
    """Resample a dataset to the specified resolution or width and height.

    The output grid covers the raster's full extent (resample_grid).

    Parameters
    ----------
    res : float or tuple, optional
        The desired resolution in the dataset coordinates.
    width : int, optional
        The desired output width. Ignored if the resolution is specified.
        If only the height is given, the width is calculated automatically.
    height : int, optional
        The desired output height. Ignored if the resolution is specified.
        If only the width is given, the height is calculated automatically.
    resampling : str, optional
        'nearest', 'bilinear', 'cubic' or 'average' for every variable. Default: 'nearest' for integer and
        bool variables (which keep their type), 'bilinear' for floating ones.
    """

    def __init__(self, res=None, width=None, height=None, resampling=None):
        self.res = res
        self.width = width
        self.height = height
        self.resampling = _check_resampling(resampling)

    def apply(self, ds):
        """Resample the dataset and return the resampled copy."""
        src, ny, nx = _grid_of(ds)
        dst, H, W = resample_grid(src, ny, nx, res=self.res, width=self.width, height=self.height)
        return _regrid(ds, dst, H, W, self.resampling)


resample = wrap_algorithm(Resample, 'resample')


class Reprojection(Algorithm):
    """Bring a dataset onto another grid of the same coordinate reference system.

    Parameters
    ----------
    target : Dataset or DataArray, optional
        A reference to which a dataset will be aligned: its transform and size are the output grid.
    src_crs, dst_crs, crs : optional
        Must be None: a change of the coordinate reference system is not served.
    extent : tuple, optional
        The output extent (left, bottom, right, top); needs `res` or `width` and `height`.
    res : float or tuple, optional
        The output resolution.
    width, height : int, optional
        The output size.
    transform : tuple, optional
        The output transform (a, b, c, d, e, f), rotation-free; needs `width` and `height`.
    resampling : str, optional
        As for Resample.
    """

    def __init__(self, target=None, src_crs=None, dst_crs=None, crs=None, extent=None, res=None, width=None,
                 height=None, transform=None, resampling=None):
        for name, value in (('src_crs', src_crs), ('dst_crs', dst_crs), ('crs', crs)):
            if value is not None:
                raise NotImplementedError('`%s` must be None: a change of the coordinate reference system is not '
                                          'served' % name)
        if target is not None:
            given = dict(transform=transform, width=width, height=height, extent=extent, res=res)
            for param in ('transform', 'width', 'height', 'extent', 'res'):
                if given[param] is not None:
                    warnings.warn('`{}` is ignored if `target` is specified.'.format(param))
            transform, height, width = _grid_of(target)
            res = extent = None
        elif transform is not None and (width is None or height is None):
            raise ValueError('If `transform` is given, you must also specify the `width` and `height` arguments.')
        elif extent is not None and res is None and (width is None or height is None):
            raise ValueError('Need to provide either `width` and `height` or resolution when specifying the '
                             'extent.')
        if transform is not None:
            transform = _check_grid(transform)
        self.extent = extent
        self.res = res
        self.width = width
        self.height = height
        self.transform = transform
        self.resampling = _check_resampling(resampling)

    def apply(self, ds):
        """Put the dataset on the grid and return the copy."""
        src, ny, nx = _grid_of(ds)
        dst, H, W = reproject_grid(src, ny, nx, transform=self.transform, extent=self.extent, res=self.res,
                                   width=self.width, height=self.height)
        return _regrid(ds, dst, H, W, self.resampling)


reproject = wrap_algorithm(Reprojection, 'reproject')


def _full_bounds(ds):
    """(left, bottom, right, top) of the raster's full extent: one pixel more than get_bounds, which spans the
    coordinates"""
    (a, _, c, _, e, f), ny, nx = _grid_of(ds)
    xs, ys = (c, c + a * nx), (f, f + e * ny)
    return (min(xs), min(ys), max(xs), max(ys))


def get_common_bounds(datasets):
    """The common bounding box (left, bottom, right, top) of the datasets (nd/warp.py:395-425): the smallest left and
    bottom and the largest right and top of the rasters' full extents."""
    b = np.array([_full_bounds(ds) for ds in datasets], dtype=np.float64)
    return tuple(float(v) for v in np.concatenate((b[:, :2].min(axis=0), b[:, 2:].max(axis=0))))


def get_common_resolution(datasets, mode='min'):
    """The common resolution (x, y) of the datasets (nd/warp.py:451-487): the smallest ('min'), largest ('max') or
    average ('mean') of their pixel sizes."""
    if mode not in ['min', 'max', 'mean']:
        raise ValueError("Unsupported mode: '{}'".format(mode))
    r = np.array([get_resolution(ds) for ds in datasets], dtype=np.float64)
    return tuple(float(v) for v in getattr(r, mode)(axis=0))


class Alignment(Algorithm):
    """Align a list of datasets to the same coordinate grid.

    Parameters
    ----------
    target : Dataset, optional
        Align the datasets with respect to the target dataset.
    extent : tuple, optional
        The bounding box of the output. By default, the common bounds of all datasets.
    res : float or tuple, optional
        The output resolution. By default, the common (smallest) resolution of all datasets.
    resampling : str, optional
        As for Resample.
    """

    def __init__(self, target=None, extent=None, res=None, resampling=None):
        self.target = target
        self.extent = extent
        self.res = res
        self.resampling = _check_resampling(resampling)

    def apply(self, datasets):
        """Resample the datasets to the target's grid, or to their common extent and resolution, and return them as
        a list.  (Files and an output path are not served.)"""
        datasets = list(datasets)
        if len(datasets) == 0:
            raise ValueError('No datasets given!')
        if any(isinstance(ds, str) for ds in datasets):
            raise NotImplementedError('Alignment serves opened datasets, not files')
        if self.target is not None:
            proj = Reprojection(target=self.target, resampling=self.resampling)
        else:
            extent = get_common_bounds(datasets) if self.extent is None else self.extent
            res = get_common_resolution(datasets) if self.res is None else self.res
            proj = Reprojection(extent=extent, res=res, resampling=self.resampling)
        return [proj.apply(ds) for ds in datasets]


align = wrap_algorithm(Alignment, 'align')
