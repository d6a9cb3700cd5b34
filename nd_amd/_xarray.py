"""
nd_amd/_xarray.py -- optional xarray accessors mirroring nd/_xarray.py:135-161 for the algorithms
this package provides: `ds.nd_amd.change_omnibus(...)`, `ds.nd_amd.nlmeans(...)`,
`ds.nd_amd.boxcar(...)`, `ds.nd_amd.convolve(...)`, `ds.nd_amd.gaussian(...)`, `ds.nd_amd.to_rgb(...)`,
`ds.nd_amd.resample(...)`, `ds.nd_amd.reproject(...)`, `ds.nd_amd.lee(...)`, `ds.nd_amd.multitemporal(...)`,
`ds.nd_amd.sieve(...)`, `ds.nd_amd.label_regions(...)`, `ds.nd_amd.zonal_stats(...)`, `ds.nd_amd.zonal_paint(...)`,
`ds.nd_amd.temporal_stats(...)`, `ds.nd_amd.composite(...)`.

Registered only when xarray is importable (it is not installed in the build or GPU images); the
accessor name differs from the reference's (`nd`, `filter`) so both can be loaded side by side.
"""
try:
    import xarray as xr
except Exception:            # pragma: no cover - xarray absent here
    xr = None


# accessor method -> (module, function form of the algorithm)
_METHODS = {
    'change_omnibus': ('change', 'omnibus'),
    'nlmeans': ('filters', 'nlmeans'),
    'boxcar': ('filters', 'boxcar'),
    'convolve': ('filters', 'convolution'),
    'gaussian': ('filters', 'gaussian'),
    'lee': ('filters', 'lee'),
    'multitemporal': ('filters', 'multitemporal'),
    'resample': ('warp', 'resample'),
    'reproject': ('warp', 'reproject'),
    'sieve': ('regions', 'sieve'),
    'label_regions': ('regions', 'label_regions'),
    'zonal_stats': ('zonal', 'zonal_stats'),
    'zonal_paint': ('zonal', 'zonal_paint'),
    'temporal_stats': ('temporal', 'temporal_stats'),
    'composite': ('temporal', 'composite'),
}


def _forward(target):
    def method(accessor, *args, **kwargs):
        return target(accessor._obj, *args, **kwargs)
    method.__name__ = target.__name__
    method.__doc__ = target.__doc__
    return method


def _to_rgb(accessor, rgb=None, *args, **kwargs):
    """nd/_xarray.py:98-115: a DataArray is one grey channel; a Dataset goes through `rgb`, a callable
    returning the R, G, B channels (default [C11, C22, C11 / C22]).  See nd_amd.visualize.to_rgb."""
    from . import visualize
    obj = accessor._obj
    if isinstance(obj, xr.DataArray) and rgb is None:
        data = obj
    else:
        if rgb is None:
            def rgb(d):
                return [d.C11, d.C22, d.C11 / d.C22]
        data = rgb(obj)
    return visualize.to_rgb(data, *args, **kwargs)


def register():
    """Attach the `nd_amd` accessor to xarray Datasets and DataArrays; False without xarray."""
    if xr is None:
        return False
    from . import change, filters, regions, temporal, warp, zonal
    modules = {'change': change, 'filters': filters, 'regions': regions, 'warp': warp, 'zonal': zonal,
               'temporal': temporal}
    namespace = {'__init__': lambda accessor, obj: setattr(accessor, '_obj', obj)}
    for name, (module, function) in _METHODS.items():
        namespace[name] = _forward(getattr(modules[module], function))
    namespace['to_rgb'] = _to_rgb
    accessor = type('NdAmdAccessor', (), namespace)
    xr.register_dataset_accessor('nd_amd')(accessor)
    xr.register_dataarray_accessor('nd_amd')(accessor)
    return True
