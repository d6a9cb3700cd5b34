"""
nd_amd/regions.py -- the connected regions of per-pixel maps, on the GPU: what a user does first with a change map
(OmnibusTest), a class map (Classifier.predict, DeviceKMeans) or a label raster (vector.rasterize).  An extension:
the reference has no counterpart.  README.md "Regions of a map" has the definition, which scipy.ndimage.label pins.

  label_regions   every (y, x) plane's regions numbered from 1 in raster order of their first pixel
                  -> nd_amd_label_regions
  region_sizes    the pixel count of every region, per plane -> nd_amd_label_regions + nd_amd_region_sizes
  Sieve / sieve   regions below a minimum mapping unit replaced by a fill value -> nd_amd_sieve_regions

Every plane is labelled on its own: no link is made along time or any other axis besides y and x.  Merging a removed
region into its largest neighbour (gdal_sieve), polygonising, and `njobs` / `devices` row sharding (a region crosses
shards) are not served.

Arrays may be numpy (copied to the device and back) or torch ROCm tensors (the result stays on the device).
"""
import warnings

import numpy as np

from . import _adapter, _device, kernels
from .algorithm import Algorithm, wrap_algorithm

__all__ = ['label_regions', 'region_sizes', 'Sieve', 'sieve']


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError('connectivity must be 4 or 8, got %r' % (connectivity,))
    return int(connectivity)


def _upload(values, dev):
    """a variable's array on the device, in the memory order it has on the host"""
    import torch
    if _device.is_tensor(values):
        return _device.to_device(values, dev)
    a = np.asarray(values)
    if a.dtype.byteorder == '>' or any(s < 0 for s in a.strides) or any(s % a.itemsize for s in a.strides):
        a = np.ascontiguousarray(a)
    with warnings.catch_warnings():
        warnings.filterwarnings('ignore', message='The given NumPy array is not writable')
        return torch.from_numpy(a).to(dev)


def _variables(obj):
    """-> (namespace, is DataArray, [(name, DataArray)] of the variables with y and x); complex ones raise"""
    ns = _adapter.namespace(obj)
    if isinstance(obj, ns.DataArray):
        todo = [(obj.name, obj)]
        if 'y' not in obj.dims or 'x' not in obj.dims:
            raise ValueError('the array needs the dimensions y and x, it has %s' % (tuple(obj.dims),))
    else:
        todo = [(n, obj[n]) for n in obj.data_vars if 'y' in obj[n].dims and 'x' in obj[n].dims]
    for n, da in todo:
        if _adapter.iscomplexobj(da.values):
            raise TypeError('variable %r is complex: regions are defined on real maps' % (n,))
    return ns, isinstance(obj, ns.DataArray), todo


def _like(da, values, attrs=None):
    """`da` with other values (possibly of another dtype) and, if given, other attrs; the rest kept"""
    from . import xr_lite
    attrs = da.attrs if attrs is None else attrs
    if _adapter.namespace(da) is xr_lite:
        return xr_lite.DataArray(values, da.dims, da.coords, attrs, da.name)
    out = da.copy(deep=False, data=values)
    out.attrs = dict(attrs)
    return out


def _map_variables(obj, run):
    """run(da, device tensor, dims) -> (device tensor, attrs or None) over the variables with y and x; the others pass
    through.  numpy in gives numpy out."""
    import torch
    _, is_array, todo = _variables(obj)
    results = {}
    if todo:
        dev = _device.device_of(*[da.values for _, da in todo])
        with torch.cuda.device(dev):
            for n, da in todo:
                host = not _device.is_tensor(da.values)
                r, attrs = run(da, _upload(da.values, dev), tuple(da.dims))
                results[n] = _like(da, _device.to_host(r) if host else r, attrs)
    if is_array:
        return results[obj.name]
    out = obj.copy(deep=False)
    for n, da in results.items():
        out[n] = da
    return out


def label_regions(obj, connectivity=4, background=0, by_value=False):
    """The connected regions of every (y, x) plane of a DataArray, or of every variable of a Dataset that has both
    `y` and `x` (the others pass through): int32 labels over the input's dims, 0 on background -- pixels equal to
    `background`, and NaN -- else 1 + the rank of the pixel's region in raster order of its first pixel.  With
    by_value=False this is scipy.ndimage.label(values != background) per plane; by_value=True joins neighbours only
    where their values are equal (the regions of a class map).  connectivity: 4 (edges) or 8 (edges and corners).
    attrs['n_regions'] is the number of regions per plane, a list of ints in plane order (C order of the axes besides
    y and x)."""
    conn = _check_connectivity(connectivity)

    def run(da, t, dims):
        labels, counts = kernels.label_regions(t, conn, background, by_value, dims=dims)
        attrs = dict(da.attrs)
        attrs['n_regions'] = [int(v) for v in counts.reshape(-1).cpu().tolist()]
        return labels, attrs

    return _map_variables(obj, run)


def region_sizes(obj, connectivity=4, background=0, by_value=False):
    """The pixel counts of the regions label_regions finds: a list with one int array per plane (plane order as
    for attrs['n_regions']), entry l - 1 the size of label l.  For a Dataset: a dict of such lists by variable."""
    import torch
    conn = _check_connectivity(connectivity)
    _, is_array, todo = _variables(obj)
    out = {}
    if todo:
        dev = _device.device_of(*[da.values for _, da in todo])
        with torch.cuda.device(dev):
            for n, da in todo:
                t = _upload(da.values, dev)
                labels, counts = kernels.label_regions(t, conn, background, by_value, dims=tuple(da.dims))
                sizes, offsets = kernels.region_sizes(labels, counts, dims=tuple(da.dims))
                sizes = sizes.cpu().numpy()
                out[n] = [sizes[a:b].astype(np.int64) for a, b in zip(offsets[:-1], offsets[1:])]
    return out[obj.name] if is_array else out


class Sieve(Algorithm):
    """Remove the regions of a map that are smaller than a minimum mapping unit.

    Every (y, x) plane of a DataArray, or of every variable of a Dataset that has both `y` and `x`, is labelled on
    its own (see label_regions); pixels of regions with fewer than `min_size` pixels become `fill`.  Background
    pixels keep their value (NaN its bits), dims, coords, attrs, dtype (bool stays bool) and memory order are kept.

    Parameters
    ----------
    min_size : int
        The smallest region kept, in pixels.  0 and 1 copy the input.
    connectivity : int, optional
        4 (default): regions are joined along edges.  8: along edges and corners.
    background : scalar, optional
        The value that belongs to no region (default: 0).  It must be representable in the map's type.
    by_value : bool, optional
        True: neighbours are joined only where their values are equal, as the classes of a class map are.
    fill : scalar, optional
        What the removed pixels become (default: `background`).

    Removed regions are not merged into a neighbouring region, as gdal_sieve does, and `njobs` / `devices` are not
    served: a region crosses the shards."""

    def __init__(self, min_size, connectivity=4, background=0, by_value=False, fill=None):
        if isinstance(min_size, bool) or int(min_size) != min_size:
            raise ValueError('min_size must be an integer, got %r' % (min_size,))
        self.min_size = int(min_size)
        self.connectivity = _check_connectivity(connectivity)
        self.background = background
        self.by_value = bool(by_value)
        self.fill = fill

    def apply(self, ds):
        """Sieve the dataset and return the sieved copy."""
        def run(da, t, dims):
            return kernels.sieve_regions(t, self.min_size, self.connectivity, self.background, self.by_value,
                                         self.fill, dims=dims), None
        return _map_variables(ds, run)


sieve = wrap_algorithm(Sieve, 'sieve')
