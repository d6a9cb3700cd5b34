"""
tests/rgb_ref.py -- numpy-only restatement of what nd.visualize.to_rgb computes (nd/visualize.py:176-193,
206) with numpy 2.2.6, written from the description in include/nd_amd.h: the test-side oracle of
nd_amd.visualize, as tests/coreg_ref.py is for Coregistration.

  nanpercentile(a, p)        np.nanpercentile(a, p) by a full sort and the index arithmetic in a's type
  limits(channel, pmin, pmax)
  composite(channels, ...)   the (y, x, 3) uint8 image of to_rgb without its cv2 steps
  numpy_composite(...)       the same image as numpy computes it (np.nanpercentile, numpy's type rules)
"""
import warnings

import numpy as np


def _as_float(a):
    a = np.asarray(a)
    return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)


def nanpercentile(a, p):
    """np.nanpercentile(a, p) for a float32 / float64 array and a Python number p, as a scalar of a's
    type.  Every step is rounded to that type: q = p / 100, the virtual index (n - 1) * q (for float32
    data beyond 2^24 values a coarse index), the weight, and the two-sided interpolation."""
    a = _as_float(a).ravel()
    T = a.dtype.type
    v = np.sort(a[~np.isnan(a)])
    n = v.size
    if n == 0:
        return T(np.nan)
    q = T(p) / T(100)
    last = T(n - 1)
    vi = last * q
    if vi >= last:
        lo = hi = n - 1
    else:
        lo = int(np.floor(vi))
        hi = min(lo + 1, n - 1)
    g = T(np.float64(vi) - np.float64(lo))
    A, B = v[lo], v[hi]
    with np.errstate(invalid='ignore', over='ignore'):
        d = B - A
        res = A + d * g
        if g >= T(0.5):
            res = B - d * (T(1) - g)
    return T(res)


def limits(channel, pmin=2, pmax=98):
    return nanpercentile(channel, pmin), nanpercentile(channel, pmax)


def _per_channel(v, n):
    if v is None:
        return None
    if isinstance(v, (int, float)):
        return [v] * n
    return list(v)


def composite(channels, vmin=None, vmax=None, pmin=2, pmax=98, mask=None, lims=None):
    """(y, x, 3) uint8.  channels: one or three 2-D arrays.  vmin / vmax: a Python number or one per
    channel.  lims: optional per-channel (minval, maxval) pairs standing in for the percentiles (scalars
    of the data type, e.g. read back from the device)."""
    channels = [np.asarray(c) for c in channels]
    n = len(channels)
    vmin, vmax = _per_channel(vmin, n), _per_channel(vmax, n)
    im = np.empty(channels[0].shape + (n,))
    with np.errstate(all='ignore'):
        for i, channel in enumerate(channels):
            if vmin is not None:
                minval = vmin[i]
            else:
                minval = lims[i][0] if lims is not None else nanpercentile(channel, pmin)
            if vmax is not None:
                maxval = vmax[i]
            else:
                maxval = lims[i][1] if lims is not None else nanpercentile(channel, pmax)
            if maxval > minval:
                channel = (channel - minval) / (maxval - minval) * 255
            im[:, :, i] = channel
        im = np.clip(im, 0, 255)
        # numpy leaves the cast of NaN to uint8 undefined; on x86-64 / numpy 2.2.6 it gives 0
        im = np.where(np.isnan(im), 0.0, im).astype(np.uint8)
    if n == 1:
        im = np.repeat(im, 3, axis=2)
    if mask is not None:
        im[~np.asarray(mask, dtype=bool)] = 0
    return im


def numpy_composite(channels, vmin=None, vmax=None, pmin=2, pmax=98, mask=None):
    """What numpy itself computes for the composite, a restatement like the rest of this file: the limits
    are np.nanpercentile's (not this file's), and the stretch, the float64 image, the clip and the cast
    are numpy's own arithmetic and type rules applied to whole planes.  Pins composite() on the CPU and
    makes the recorded golden bytes."""
    channels = [np.asarray(c) for c in channels]
    vmin, vmax = _per_channel(vmin, len(channels)), _per_channel(vmax, len(channels))
    stretched = []
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')                   # numpy warns about an all-NaN plane
        for i, plane in enumerate(channels):
            lo = np.nanpercentile(plane, pmin) if vmin is None else vmin[i]
            hi = np.nanpercentile(plane, pmax) if vmax is None else vmax[i]
            stretched.append((plane - lo) / (hi - lo) * 255 if hi > lo else plane)
        im = np.stack([np.asarray(p, dtype=np.float64) for p in stretched], axis=-1)
        im = np.clip(im, 0, 255).astype(np.uint8)
    if len(channels) == 1:
        im = np.concatenate([im] * 3, axis=-1)
    if mask is not None:
        im = im * np.asarray(mask, dtype=np.uint8)[:, :, None]
    return im
