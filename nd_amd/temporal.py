"""
nd_amd/temporal.py -- per-pixel statistics and composites along time, on the GPU: the median composite, the temporal
mean and coefficient of variation, the date of the maximum, a percentile envelope, the number of changes of an
OmnibusTest map.  An extension: the reference has no counterpart.  README.md "Statistics along time" has the
definition, which tests/temporal_ref.py restates bit for bit and numpy's nanpercentile / nanmedian hold.

  temporal_stats       <var>__<stat> over the variable's dims without `dim` -> nd_amd_temporal_stats
  TemporalStatistics   the same as an Algorithm, with its wrap_algorithm form temporal_statistics
  composite            the dataset with the same variable names, each reduced by one statistic or percentile

Every real variable that has `dim` and at most two other dims is reduced; variables without `dim` pass through.
`njobs` / `devices` sharding and the streaming path are not offered.

Arrays may be numpy (copied to the device and back) or torch ROCm tensors (the result stays on the device).
"""
from . import _adapter, _device, kernels
from .algorithm import Algorithm, wrap_algorithm
from .regions import _upload

__all__ = ['temporal_stats', 'composite', 'TemporalStatistics', 'temporal_statistics', 'STATS']

STATS = kernels.TEMPORAL_STATS


def _check_stats(stats):
    stats = (stats,) if isinstance(stats, str) else tuple(stats)
    for s in stats:
        if s not in STATS:
            raise ValueError('stats must be among %s, got %r' % (STATS, s))
    return stats


def _check_ddof(ddof):
    if isinstance(ddof, bool) or int(ddof) != ddof or ddof < 0:
        raise ValueError('ddof must be a non-negative integer, got %r' % (ddof,))
    return int(ddof)


def _variables(obj, dim):
    """-> (namespace, is DataArray, [(name, DataArray)] of the variables with `dim`); complex ones and those with
    three or more other dims raise"""
    ns = _adapter.namespace(obj)
    is_array = isinstance(obj, ns.DataArray)
    if is_array:
        todo = [(obj.name if obj.name is not None else 'data', obj)]
    else:
        todo = [(n, obj[n]) for n in obj.data_vars]
    todo = [(n, da) for n, da in todo if dim in da.dims]
    if not todo:
        raise ValueError('no variable has the dimension %r' % (dim,))
    for n, da in todo:
        if _adapter.iscomplexobj(da.values):
            raise TypeError('variable %r is complex: statistics along time are defined on real data' % (n,))
        if len(da.dims) > 3:
            raise NotImplementedError('variable %r has %d dims besides %r: one or two are served'
                                      % (n, len(da.dims) - 1, dim))
    return ns, is_array, todo


def _reduce(da, dim, stats, q, skipna, ddof, dev):
    """{key: array over da's dims without `dim`} of one variable, on the host if the variable is"""
    values = da.values
    host = not _device.is_tensor(values)
    t = _upload(values, dev)
    axis = tuple(da.dims).index(dim)
    kept = tuple(n for i, n in enumerate(t.shape) if i != axis)
    view = t.movedim(axis, 0)
    while view.dim() < 3:                               # a (time, x) variable is ny = 1
        view = view.unsqueeze(1)
    got = kernels.temporal_stats(view, stats, q, skipna=skipna, ddof=ddof, axis=0)
    out = {}
    for key, r in got.items():
        r = r.reshape(kept)
        out[key] = _device.to_host(r) if host else r
    return out


def _coords_without(ds, dim):
    """the coordinates that do not run along `dim`"""
    out = {}
    for name in ds.coords:
        c = ds.coords[name]
        if name != dim and dim not in getattr(c, 'dims', ()):
            out[name] = c
    return out


def _on(dev):
    import torch
    return torch.cuda.device(dev)


def _run(ds, stats, q, dim, skipna, ddof, naming):
    ns, is_array, todo = _variables(ds, dim)
    dev = _device.device_of(*[da.values for _, da in todo])
    coords = _coords_without(ds, dim)
    data_vars = {}
    with _on(dev):
        reduced = {n: _reduce(da, dim, stats, q, skipna, ddof, dev) for n, da in todo}
    names = [n for n, _ in todo]
    for n, da in ([] if is_array else [(n, ds[n]) for n in ds.data_vars]):
        if n not in names:
            data_vars[n] = da                           # no `dim`: passes through
    for n, da in todo:
        dims = tuple(d for d in da.dims if d != dim)
        for key, values in reduced[n].items():
            data_vars[naming(n, key)] = ns.DataArray(values, dims=dims, attrs=dict(da.attrs))
    return ns, is_array, ns.Dataset(data_vars, coords=coords, attrs=dict(ds.attrs))


def temporal_stats(ds, stats=('mean', 'std'), q=None, dim='time', skipna=True, ddof=0):
    """Per-pixel statistics over `dim` of every real variable of `ds` (a Dataset or a DataArray) that has `dim` and
    at most two other dims: a Dataset of the variables `<var>__<stat>` (percentiles: `<var>__p<q>`, as `VV__p2`,
    `VV__p97.5`) over the variable's other dims, in their order, with coords and attrs kept.  Variables without
    `dim` pass through unchanged.

    stats: among count, nan_count, sum, mean, min, max, argmin, argmax, m2, var, std, cv, median.  q: a percentile or a
    sequence of them, each in [0, 100].  skipna: NaN dates are skipped (and counted by nan_count); with skipna=False
    they enter the arithmetic.  ddof: var and std divide by count - ddof and are NaN where that is not positive.
    float32 and float64 are computed as they are, integers, uint8 and bool as float64.  min, max, median and
    percentiles have the type computed in, count, nan_count, argmin and argmax are int32, the rest float64."""
    stats = _check_stats(stats)
    q = kernels.temporal_percentiles(q)
    ddof = _check_ddof(ddof)
    if not stats and not q:
        raise ValueError('no statistic and no percentile asked for')
    return _run(ds, stats, q, dim, bool(skipna), ddof, lambda n, key: '%s__%s' % (n, key))[2]


class TemporalStatistics(Algorithm):
    """Per-pixel statistics of a dataset's variables along a dimension.

    Parameters
    ----------
    stats : tuple of str, optional
        Among count, nan_count, sum, mean, min, max, argmin, argmax, m2, var, std, cv, median.
    q : float or sequence of float, optional
        Percentiles in [0, 100].
    dim : str, optional
        The dimension to reduce (default 'time').
    skipna : bool, optional
        Skip NaN dates (default True).
    ddof : int, optional
        var and std divide by count - ddof (default 0).

    `njobs` / `devices` are not served."""

    def __init__(self, stats=('mean', 'std'), q=None, dim='time', skipna=True, ddof=0):
        self.stats = _check_stats(stats)
        self.q = kernels.temporal_percentiles(q)
        self.dim = dim
        self.skipna = bool(skipna)
        self.ddof = _check_ddof(ddof)

    def apply(self, ds):
        """The statistics of the dataset along `dim` (see temporal_stats)."""
        return temporal_stats(ds, self.stats, self.q, self.dim, self.skipna, self.ddof)


temporal_statistics = wrap_algorithm(TemporalStatistics, 'temporal_statistics')


def composite(ds, how='median', dim='time', skipna=True):
    """`ds` with every variable that has `dim` reduced over it by `how`: a statistic's name, or a number in
    [0, 100] for that percentile.  The variables keep their names (and a DataArray stays one), so the result goes
    straight into to_rgb."""
    if isinstance(how, str):
        stats, q = _check_stats(how), ()
    else:
        stats, q = (), kernels.temporal_percentiles(how)
        if len(q) != 1:
            raise ValueError('how is one statistic or one percentile, got %r' % (how,))
    ns, is_array, out = _run(ds, stats, q, dim, bool(skipna), 0, lambda n, key: n)
    if is_array:
        da = out[ds.name if ds.name is not None else 'data']
        da.name = ds.name
        return da
    return out
