"""
nd_amd/vector.py -- polygons burned into label rasters on the device (nd/vector.py:48-187).

  rasterize(shp, ds, ...)         nd.vector.rasterize: one variable per property column over ('y', 'x', 'time'),
                                  the `labels` that Classifier.fit(ds, labels) consumes
  rasterize_shapes(shapes, ...)   the plain form: a sequence of ring lists -> one (y, x) DataArray

The reference rasterises with rasterio / GDAL and reads vector files with geopandas; neither is needed here.
Features are read from GeoJSON-like Python objects (a FeatureCollection dict, a list of features, anything with
`__geo_interface__`, a .json / .geojson path), their vertices go to pixel coordinates on the host in float64, and
the burning -- scanline crossings of every polygon, highest index wins -- is nd_amd_rasterize_polygons
(nd_amd/csrc/rasterize.hip).  The inside rule is this project's and is written out in include/nd_amd.h and the
README: even-odd, half-open on both axes, bit for bit reproducible.

Not served: lines and points, all_touched, CRS transformation, shapefiles, rotated transforms, rasters of 2^32
pixels x layers or more.
"""
import datetime
import json
import numbers
import os
from collections import OrderedDict

import numpy as np

from . import _adapter, _device, warp, xr_lite

__all__ = ['rasterize', 'rasterize_shapes']


# ---------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------
def _read_features(shp):
    """-> [(geometry dict, properties dict)]"""
    if isinstance(shp, (str, os.PathLike)):
        path = os.fspath(shp)
        if os.path.splitext(path)[1].lower() not in ('.json', '.geojson'):
            raise NotImplementedError('nd_amd.vector reads .json / .geojson files only (no geopandas / fiona here): %s'
                                      % path)
        with open(path) as fh:
            shp = json.load(fh)
    if hasattr(shp, '__geo_interface__'):
        shp = shp.__geo_interface__
    if isinstance(shp, dict):
        kind = shp.get('type')
        if kind == 'FeatureCollection':
            shp = shp.get('features', [])
        elif kind == 'Feature':
            shp = [shp]
        else:
            raise ValueError("expected a GeoJSON FeatureCollection or Feature, got type %r" % (kind,))
    out = []
    for feat in list(shp):
        if hasattr(feat, '__geo_interface__'):
            feat = feat.__geo_interface__
        if not isinstance(feat, dict) or 'geometry' not in feat:
            raise ValueError('not a GeoJSON feature: %r' % (feat,))
        out.append((feat['geometry'], dict(feat.get('properties') or {})))
    return out


def _rings_of(geometry):
    """the rings of a Polygon or MultiPolygon geometry, all together: [(m, 2) float64 array]"""
    if geometry is None:
        return []
    if hasattr(geometry, '__geo_interface__'):
        geometry = geometry.__geo_interface__
    kind = geometry.get('type')
    if kind == 'Polygon':
        parts = [geometry['coordinates']]
    elif kind == 'MultiPolygon':
        parts = geometry['coordinates']
    else:
        raise NotImplementedError('nd_amd.vector serves Polygon and MultiPolygon geometries, not %r' % (kind,))
    return [_ring(ring) for part in parts for ring in part]


def _ring(ring):
    a = np.asarray(ring, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 2))
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError('a ring is a sequence of (X, Y) vertices, got an array of shape %s' % (a.shape,))
    a = np.ascontiguousarray(a[:, :2])              # a third ordinate (Z) plays no part
    if not np.all(np.isfinite(a)):
        raise ValueError('non-finite vertex coordinates')
    return a


def _check_transform(transform):
    t = tuple(float(v) for v in tuple(transform)[:6])
    if len(t) != 6:
        raise ValueError('a transform is the 6-tuple (a, b, c, d, e, f), got %r' % (transform,))
    a, b, c, d, e, f = t
    if b != 0 or d != 0:
        raise NotImplementedError('rotated transforms are not served: %r' % (t,))
    if a == 0 or e == 0 or not all(np.isfinite(t)):
        raise ValueError('a transform needs finite terms and non-zero pixel sizes, got %r' % (t,))
    return t


def _to_pixel(ring, t):
    a, _, c, _, e, f = t
    px = np.stack([(ring[:, 0] - c) / a, (ring[:, 1] - f) / e], axis=1)
    if not np.all(np.isfinite(px)):
        raise ValueError('non-finite pixel coordinates')
    return px


class _Geometry:
    """The polygons of one call in pixel coordinates; the device table is built once, on first use."""

    def __init__(self, polys, ny, nx):
        self.polys, self.ny, self.nx = polys, int(ny), int(nx)
        self._table = None

    def packed(self):
        verts, ring_offsets, poly_offsets = [], [0], [0]
        for rings in self.polys:
            for ring in rings:
                verts.append(ring)
                ring_offsets.append(ring_offsets[-1] + len(ring))
            poly_offsets.append(len(ring_offsets) - 1)
        verts = np.concatenate(verts) if verts else np.zeros((0, 2))
        return verts, np.asarray(ring_offsets, np.int64), np.asarray(poly_offsets, np.int64)

    def table(self, device):
        from . import kernels
        if self._table is None or self._table.device != device:
            self._table = kernels.PolygonTable(*self.packed(), self.ny, self.nx, device=device)
        return self._table


def _burn(geometry, values, layer, nlayers, fill, device):
    """(ny, nx, nlayers) device tensor of the values' type: the one call into the HIP library"""
    import torch
    from . import kernels
    dev = _device.device_of(device=device)
    if dev.index is None:                   # 'cuda': the current device, named with its index as tensors name it
        dev = torch.device(dev.type, torch.cuda.current_device())
    with torch.cuda.device(dev):
        dtype = torch.float64 if np.asarray(values).dtype.kind == 'f' else torch.int64
        buf = torch.empty((geometry.ny, geometry.nx, nlayers), dtype=dtype, device=dev)
        kernels.rasterize_polygons(geometry.table(dev), None, None, values, geometry.ny, geometry.nx, layer=layer,
                                   nlayers=nlayers, fill=fill, out=buf.permute(2, 0, 1))
    return buf


# ---------------------------------------------------------------------------
# columns and dates
# ---------------------------------------------------------------------------
def _column(data, name, encode_labels):
    """-> (values int64 / float64 array, attrs) of one property column"""
    present = [v for v in data if v is not None]
    if any(isinstance(v, str) for v in present) or not all(isinstance(v, numbers.Real) for v in present):
        if not encode_labels:
            raise NotImplementedError("column %r holds strings: burning them needs encode_labels=True" % (name,))
        # factorise in order of first appearance, plus 1: 0 is the background (and a missing label)
        codes, legend = [], OrderedDict()
        for v in data:
            codes.append(0 if v is None else legend.setdefault(v, len(legend) + 1))
        return np.asarray(codes, np.int64), {'legend': list(enumerate([None] + list(legend)))}
    if len(present) == len(data) and all(isinstance(v, numbers.Integral) for v in present):
        return np.asarray([int(v) for v in data], np.int64), {}
    return np.asarray([np.nan if v is None else float(v) for v in data], np.float64), {}


def _dates(props, date_field, date_fmt):
    """-> (time coordinate datetime64[ns], layer number of every feature)"""
    if date_field is None:
        stamps = np.full(len(props), np.datetime64(datetime.date.today()), dtype='datetime64[ns]')
    else:
        if not any(date_field in p for p in props):
            raise ValueError('Field {} does not exist.'.format(date_field))
        stamps = []
        for p in props:
            v = p.get(date_field)
            if v is None:
                raise ValueError('a feature has no %r' % (date_field,))
            if date_fmt is not None:
                v = datetime.datetime.strptime(str(v), date_fmt)
            stamps.append(np.datetime64(v, 'ns'))
        stamps = np.asarray(stamps, dtype='datetime64[ns]')
    if len(props) == 0:
        return stamps.astype('datetime64[ns]'), np.zeros(0, np.int32)
    times = np.unique(stamps)
    return times, np.searchsorted(times, stamps).astype(np.int32)


def _home(ds, device):
    """the device the result stays on: the one asked for, else that of the dataset's device tensors, else None
    (the result comes back as numpy)"""
    return device if device is not None else _adapter.home_device(ds)


# ---------------------------------------------------------------------------
# the public calls
# ---------------------------------------------------------------------------
def rasterize(shp, ds, columns=None, encode_labels=True, crs=None, date_field=None, date_fmt=None, transform=None,
              device=None):
    """Burn the polygons of a vector dataset into rasters on the grid of `ds` (nd.vector.rasterize).

    Parameters
    ----------
    shp : dict, list, object with ``__geo_interface__``, or str
        A GeoJSON FeatureCollection, a list of features, a GeoDataFrame-like object, or the path of a
        ``.json`` / ``.geojson`` file.  Polygon and MultiPolygon geometries are served.
    ds : Dataset
        The dataset whose ``y`` / ``x`` coordinates give the grid and the shape of the result.
    columns : list of str, optional
        The property columns to burn (default: all).
    encode_labels : bool, optional
        Convert string columns to integer codes, 1 + the order of first appearance; the legend is stored in the
        variable's ``attrs['legend']`` (default: True).  False raises NotImplementedError for such columns.
    crs : optional
        Must be None: there is no CRS transformation here.
    date_field : str, optional
        The property holding the timestamp; without it there is one layer, dated today.
    date_fmt : str, optional
        The format of date_field, passed to ``datetime.strptime``.
    transform : 6-tuple, optional
        (a, 0, c, 0, e, f); default ``nd_amd.warp.get_transform(ds)``.
    device : torch.device, optional
        Keep the result on this device.  Where `ds` holds device tensors it stays on theirs; otherwise it comes
        back as numpy.

    Returns
    -------
    Dataset
        One variable per column over ('y', 'x', 'time'); pixels no feature covers are 0.
    """
    if crs is not None:
        raise NotImplementedError('nd_amd.vector.rasterize: no CRS transformation here (crs must be None)')
    ns = _adapter.namespace(ds)
    t = _check_transform(warp.get_transform(ds) if transform is None else transform)
    ny, nx = int(ds.sizes['y']), int(ds.sizes['x'])
    feats = _read_features(shp)
    props = [p for _, p in feats]
    geometry = _Geometry([[_to_pixel(r, t) for r in _rings_of(g)] for g, _ in feats], ny, nx)
    times, layer = _dates(props, date_field, date_fmt)
    if len(times) == 0:
        times = np.asarray([np.datetime64(datetime.date.today())], dtype='datetime64[ns]')

    if columns is None:
        names = list(OrderedDict((k, None) for p in props for k in p))
    else:
        names = list(OrderedDict((k, None) for k in columns))
        missing = [k for k in names if k != 'geometry' and not any(k in p for p in props)]
        if missing:
            raise ValueError('Field {} does not exist.'.format(missing[0]))
    names = [k for k in names if k not in ('geometry', date_field)]

    coords = OrderedDict()
    for d in ('y', 'x'):
        if d in ds.coords:
            coords[d] = ds.coords[d]
    coords['time'] = times
    attrs = OrderedDict(transform=t)
    if 'crs' in ds.attrs:
        attrs['crs'] = ds.attrs['crs']
    out = ns.Dataset(coords=coords, attrs=attrs)
    home = _home(ds, device)
    for name in names:
        values, meta = _column([p.get(name) for p in props], name, encode_labels)
        burned = _burn(geometry, values, layer, len(times), 0, home)
        if home is None and _device.is_tensor(burned):
            burned = _device.to_host(burned)
        out[name] = (('y', 'x', 'time'), burned, meta)
    return out


def rasterize_shapes(shapes, ds_or_shape, values=None, transform=None, fill=0):
    """Burn a sequence of shapes -- each a list of rings, a ring a sequence of (X, Y) -- into one (y, x) DataArray.
    ds_or_shape: the reference dataset (its coordinates give the transform unless one is passed) or a (ny, nx)
    tuple, for which the coordinates are pixel coordinates unless a transform is passed.  values: one per shape,
    default 1, 2, 3, ...; later shapes replace earlier ones, `fill` where there is none.  The result lives where
    the dataset's variables live (numpy for a shape tuple)."""
    coords, home, ns = OrderedDict(), None, xr_lite
    if isinstance(ds_or_shape, (tuple, list)):
        ny, nx = (int(n) for n in ds_or_shape)
        t = _check_transform((1, 0, 0, 0, 1, 0) if transform is None else transform)
    else:
        ds = ds_or_shape
        ns = _adapter.namespace(ds)
        ny, nx = int(ds.sizes['y']), int(ds.sizes['x'])
        t = _check_transform(warp.get_transform(ds) if transform is None else transform)
        for d in ('y', 'x'):
            if d in ds.coords:
                coords[d] = ds.coords[d]
        home = _home(ds, None)
    polys = [[_to_pixel(_ring(r), t) for r in rings] for rings in shapes]
    if values is None:
        values = np.arange(1, len(polys) + 1, dtype=np.int64)
    values = np.asarray(values)
    if values.shape != (len(polys),):
        raise ValueError('values must be one per shape (%d), got shape %s' % (len(polys), values.shape))
    values, _ = _column(values.tolist(), 'values', False)
    burned = _burn(_Geometry(polys, ny, nx), values, None, 1, fill, home)[:, :, 0]
    if home is None and _device.is_tensor(burned):
        burned = _device.to_host(burned.contiguous())
    if ns is xr_lite:
        return xr_lite.DataArray(burned, ('y', 'x'), coords, OrderedDict(transform=t))
    return ns.DataArray(burned, dims=('y', 'x'), coords=coords, attrs={'transform': t})
