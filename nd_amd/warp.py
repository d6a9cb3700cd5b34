"""
nd_amd/warp.py -- Coregistration (nd/warp.py:1104-1163) with the arithmetic on the GPU.

  Coregistration  every date of a stack aligned to a reference date.  The shift of each date's C11
                  plane against the reference's (skimage.registration.phase_cross_correlation with
                  upsample_factor=upsampling, scikit-image 0.18) -> nd_amd_coregister_shifts; every
                  variable with the dimensions time, y and x translated by it (skimage.transform.warp,
                  bicubic, 0 outside, clipped to the plane's input range) -> nd_amd_warp_translate.

  get_transform / get_resolution / get_bounds   the coordinate-based arithmetic of nd/warp.py:175-251 as plain
                  tuples (no affine / rasterio objects): what nd_amd.vector.rasterize places its grid with.

Reprojection, Resample and Alignment (GDAL wrappers) are not part of this package.  Arrays may be
numpy (copied to the device and back) or torch ROCm tensors (the result stays on the device).
"""
import operator

import numpy as np

from . import _adapter, _device, kernels
from .algorithm import Algorithm, wrap_algorithm
from .io import disassemble_complex

__all__ = ['Coregistration', 'coregister', 'get_transform', 'get_resolution', 'get_bounds']

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
