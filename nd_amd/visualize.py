"""
nd_amd/visualize.py -- percentile-stretched RGB composites (nd/visualize.py:116-215, 258-305) on the GPU.

  to_rgb          nd.visualize.to_rgb for categorical=False without its cv2 steps: every channel
                  stretched between its own np.nanpercentile(pmin) and (pmax) -- or vmin / vmax -- and
                  packed into (y, x, 3) uint8.  -> nd_amd_rgb_limits + nd_amd_rgb_compose
  to_rgb_stack    the frames nd.visualize.write_video computes before its cv2 calls, all dates in one
                  batch: (time, y, x, 3) uint8.  The default channels [C11, C22, C11 / C22] are served
                  without forming the quotient.
  stretch_limits  the (time, channel, 2) limits alone.

The percentiles are what numpy 2.2.6 returns for data of the same type, bit for bit (exact selection and
numpy's index and interpolation arithmetic in that type; include/nd_amd.h has the definition).  numpy
leaves the cast of NaN to uint8 undefined; this module gives 0, which is what numpy gives on x86-64.

Writing image or video files, resizing, colour maps, `colorize` and `plot_map` (cv2, imageio, cartopy) are
not part of this package.  Arrays may be numpy (copied to the device whole, result copied back) or torch
ROCm tensors (the result stays on the device).
"""
import numpy as np

from . import _adapter, _device, kernels

__all__ = ['to_rgb', 'to_rgb_stack', 'stretch_limits']

_CV2 = ('%s needs cv2 in the reference (nd.visualize.to_rgb); nd_amd computes the percentile-stretched '
        '(y, x, 3) uint8 image only')


def _values(d):
    """the array behind a DataArray (xarray or xr_lite), a numpy array or a tensor"""
    if _device.is_tensor(d) or isinstance(d, np.ndarray):
        return d
    if hasattr(d, 'dims') and hasattr(d, 'values'):
        return d.values
    return np.asarray(d)


def _float_plane(v, dev):
    """device tensor of float32 / float64; integers are computed as float64, as numpy's percentile and
    the stretch do.  bool raises like np.nanpercentile does in numpy 2.2.6."""
    import torch
    dt = _device.np_dtype(v)
    if dt == np.bool_:
        raise TypeError("to_rgb: boolean data cannot be stretched (numpy boolean subtract, the `-` operator, "
                        "is not supported by np.nanpercentile): pass change.astype('uint8')")
    if dt.kind == 'c':
        raise TypeError('to_rgb: complex data is not supported')
    if dt.kind not in 'fiu' or dt == np.float16:
        raise TypeError('to_rgb: unsupported dtype %s' % dt)
    t = _device.to_device(v, dev)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t


def _per_channel(v, n, name):
    if v is None:
        return None
    if np.ndim(v) == 0:
        return [float(v)] * n
    v = [float(x) for x in v]
    if len(v) != n:
        raise ValueError('%s needs one value per channel (%d), got %d' % (name, n, len(v)))
    return v


def _mask(mask, shape, dev):
    import torch
    if mask is None:
        return None
    m = _values(mask)
    m = m if _device.is_tensor(m) else np.asarray(m)
    if tuple(m.shape) != tuple(shape):
        raise ValueError('mask has shape %s, the image %s' % (tuple(m.shape), tuple(shape)))
    m = _device.to_device(m, dev)
    return m if m.dtype in (torch.bool, torch.uint8) else (m != 0)


def _same_layout(planes):
    """(frames, y, x) views that share dtype and strides, copying only where they do not"""
    import torch
    dt = planes[0].dtype
    if any(t.dtype != dt for t in planes):
        dt = torch.float64
        planes = [t.to(dt) for t in planes]
    if len({kernels._rgb_strides(t) for t in planes}) > 1:
        planes = [t.contiguous() for t in planes]
    return planes


def _run(channels, vmin, vmax, pmin, pmax, mask, limits_only=False):
    nch = len(channels)
    vmin, vmax = _per_channel(vmin, nch, 'vmin'), _per_channel(vmax, nch, 'vmax')
    limits = None
    if vmin is None or vmax is None or limits_only:
        limits, _ = kernels.rgb_limits(channels, pmin, pmax)
    if limits_only:
        return limits
    return kernels.rgb_compose(channels, limits, vmin, vmax, mask)


def to_rgb(data, output=None, vmin=None, vmax=None, pmin=2, pmax=98, categorical=False, mask=None,
           shape=None, cmap=None):
    """Turn some data into an array representing an RGB image.

    Parameters
    ----------
    data : 2-D array / DataArray, or list of one or three
    output : not supported (cv2.imwrite)
    vmin, vmax : float or list of float
        minimum / maximum value, or one per channel (default: None).  Python numbers.
    pmin, pmax : float
        lowest / highest percentile to plot (default: 2, 98).  Ignored where vmin / vmax is passed.
    categorical, cmap : not supported (cv2.applyColorMap)
    mask : bool array (y, x), optional
        parts of the image outside of the mask will be black.
    shape : tuple, optional
        only None or the image's own (height, width): resizing needs cv2.

    Returns
    -------
    (y, x, 3) uint8: a numpy array for numpy input, a device tensor for device input.  A NaN pixel is 0
    (numpy leaves that cast undefined and gives 0 on x86-64).

    Deviations from numpy's type rules: integer planes are computed as float64 throughout, which is what
    numpy does with percentile limits and with vmin / vmax given as Python floats; with a Python *int*
    vmin numpy 2 subtracts in the plane's integer type (wrapping, or raising when the number does not
    fit) -- pass floats.  float16 planes are not supported (TypeError), numpy computes them in float16.
    """
    import torch
    if isinstance(data, (list, tuple)):
        data = list(data)
    elif hasattr(data, 'shape'):
        data = [data]
    else:
        raise ValueError("`data` must be a DataArray or list of DataArrays")
    for d in data:
        if len(d.shape) > 2:
            raise ValueError("The RGB channels must be two-dimensional. "
                             "Found dimensions {}".format(getattr(d, 'dims', tuple(d.shape))))
    if output is not None:
        raise NotImplementedError(_CV2 % 'output')
    if categorical:
        raise NotImplementedError(_CV2 % 'categorical=True')
    if cmap is not None:
        raise NotImplementedError(_CV2 % 'cmap')
    if len(data) not in (1, 3):
        raise ValueError('to_rgb takes one channel or three, got %d' % len(data))
    values = [_values(d) for d in data]
    for v in values:
        if len(v.shape) != 2 or tuple(v.shape) != tuple(values[0].shape):
            raise ValueError('the channels must be two-dimensional and of one shape')
    if shape is not None:
        h, w = shape
        if (h is not None and h != values[0].shape[0]) or (w is not None and w != values[0].shape[1]):
            raise NotImplementedError(_CV2 % 'a shape that resizes the image')
    host = not any(_device.is_tensor(v) and v.is_cuda for v in values)
    dev = _device.device_of(*values)
    with torch.cuda.device(dev):
        planes = _same_layout([_float_plane(v, dev).unsqueeze(0) for v in values])
        out = _run(planes, vmin, vmax, pmin, pmax, _mask(mask, values[0].shape, dev))[0]
    return _device.to_host(out) if host else out


def _stack_channels(ds, rgb, dev):
    """-> (channels for kernels.rgb_*, whether every input was host data)"""
    ns = _adapter.namespace(ds)

    def frames(da):
        if not (hasattr(da, 'dims') and hasattr(da, 'values')):
            raise ValueError('to_rgb_stack: `rgb` must return DataArrays with the dimensions time, y and x')
        if sorted(da.dims) != ['time', 'x', 'y']:
            raise ValueError("to_rgb_stack: a channel has dimensions %s, need time, y and x" % (tuple(da.dims),))
        t = _float_plane(da.values, dev)
        return t.permute(*[da.dims.index(d) for d in ('time', 'y', 'x')])

    if rgb is None and isinstance(ds, ns.DataArray):
        chans = [ds]
    elif rgb is None:
        c11, c22 = frames(ds['C11']), frames(ds['C22'])
        c11, c22 = _same_layout([c11, c22])
        host = not (_device.is_tensor(ds['C11'].values) or _device.is_tensor(ds['C22'].values))
        return [c11, c22, (c11, c22)], host
    else:
        chans = rgb(ds)
        if not isinstance(chans, (list, tuple)):
            chans = [chans]
    if len(chans) not in (1, 3):
        raise ValueError('to_rgb_stack: `rgb` must return one channel or three, got %d' % len(chans))
    host = not any(_device.is_tensor(c.values) for c in chans if hasattr(c, 'values'))
    return _same_layout([frames(c) for c in chans]), host


def _stack(ds, rgb, vmin, vmax, pmin, pmax, mask, limits_only):
    import torch
    ns = _adapter.namespace(ds)
    arrays = [ds.values] if isinstance(ds, ns.DataArray) else [v.values for v in ds.data_vars.values()]
    dev = _device.device_of(*arrays)
    with torch.cuda.device(dev):
        channels, host = _stack_channels(ds, rgb, dev)
        first = channels[0]
        m = None if limits_only else _mask(mask, tuple(first.shape[1:]), dev)
        out = _run(channels, vmin, vmax, pmin, pmax, m, limits_only)
    return _device.to_host(out) if host else out


def to_rgb_stack(ds, rgb=None, vmin=None, vmax=None, pmin=2, pmax=98, mask=None):
    """The frames nd.visualize.write_video computes (nd/visualize.py:303-305) before its cv2 calls:
    to_rgb(rgb(ds.sel(time=t)), mask=mask) for every date, in one batch.

    ds : Dataset or DataArray with the dimensions time, y and x, in any order ((time, y, x) is the fast
        layout).  rgb : callable returning one or three DataArrays of the dataset's dimensions; default
        [C11, C22, C11 / C22] for a Dataset (the quotient is never stored), grey frames for a DataArray.
    Returns (time, y, x, 3) uint8, numpy for host data, a device tensor for device data."""
    return _stack(ds, rgb, vmin, vmax, pmin, pmax, mask, False)


def stretch_limits(ds, rgb=None, pmin=2, pmax=98):
    """The stretch limits to_rgb_stack would use: (time, channel, 2) of the data type,
    [..., 0] = np.nanpercentile(channel, pmin), [..., 1] = (channel, pmax), per date and channel."""
    return _stack(ds, rgb, None, None, pmin, pmax, None, True)
