"""Seeded synthetic inputs shared by the CPU and GPU tests (numpy only)."""
import numpy as np


def wishart_c2(rng, shape, looks=9, dtype=np.float32, corr=0.3, power=(1.0, 0.5)):
    """n-look complex-Wishart dual-pol covariance samples.
    Returns c11, c12re, c12im, c22 arrays of `shape`."""
    def cn(sh):
        return (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(2.0)
    s1 = cn((looks,) + tuple(shape))
    s2 = corr * s1 + np.sqrt(1 - corr ** 2) * cn((looks,) + tuple(shape))
    s1 = s1 * np.sqrt(power[0])
    s2 = s2 * np.sqrt(power[1])
    c11 = (np.abs(s1) ** 2).mean(axis=0)
    c22 = (np.abs(s2) ** 2).mean(axis=0)
    c12 = (s1 * np.conj(s2)).mean(axis=0)
    return (c11.astype(dtype), c12.real.astype(dtype), c12.imag.astype(dtype),
            c22.astype(dtype))


def omnibus_stack(seed, k, ny, nx, looks=9, dtype=np.float32, change_frac=0.05,
                  factor=4.0):
    """Planar (time, y, x) Wishart stack with a fraction of pixels stepping in
    power by `factor` at a random date.  Returns 4 arrays (k, ny, nx)."""
    rng = np.random.default_rng(seed)
    planes = wishart_c2(rng, (k, ny, nx), looks, np.float64)
    if change_frac > 0:
        mask = rng.random((ny, nx)) < change_frac
        t0 = rng.integers(1, max(k, 2), size=(ny, nx))
        step = (np.arange(k)[:, None, None] >= t0[None]) & mask[None]
        gain = np.where(step, factor, 1.0)
        # second population: a drop, so both directions and multi-change pixels occur
        mask2 = rng.random((ny, nx)) < change_frac / 2
        t1 = rng.integers(1, max(k, 2), size=(ny, nx))
        gain = gain * np.where((np.arange(k)[:, None, None] >= t1[None]) & mask2[None], 0.3, 1.0)
        planes = tuple(p * gain for p in planes)
    return tuple(np.ascontiguousarray(p.astype(dtype)) for p in planes)


def reference_test_dataset(dims, mean, sigma, seed=42,
                           var=('C11', 'C12__im', 'C12__re', 'C22')):
    """nd.testing.generate_test_dataset (nd/testing.py:34-70) restated for
    plain arrays: np.random.seed(seed), one float64 normal draw per variable in
    `var` order, shape = dims values."""
    np.random.seed(seed)
    if np.isscalar(mean):
        mean = [mean] * len(var)
    out = {}
    for v, m in zip(var, mean):
        out[v] = np.random.normal(m, sigma, tuple(dims.values()))
    return out


def lite_test_dataset(dims=None, var=('C11', 'C12__im', 'C12__re', 'C22'), mean=0, sigma=1,
                      seed=42):
    """nd.testing.generate_test_dataset (nd/testing.py:34-70) as an nd_amd.xr_lite.Dataset:
    same seed, same draw order, same values; coordinates reduced to plain index arrays."""
    from collections import OrderedDict
    from nd_amd import xr_lite
    if dims is None:
        dims = OrderedDict([('y', 20), ('x', 20), ('time', 10)])
    data = reference_test_dataset(dims, mean, sigma, seed, var)
    coords = OrderedDict()
    for name, size in dims.items():
        if name == 'y':
            coords[name] = np.linspace(60.0, 50.0, size)
        elif name == 'x':
            coords[name] = np.linspace(-10.0, 0.0, size)
        else:
            coords[name] = np.arange(size)
    ds = xr_lite.Dataset(coords=coords, attrs={'attr1': 1, 'attr2': 2, 'attr3': 3})
    for v in var:
        ds[v] = (tuple(dims.keys()), data[v])
    return ds


def wishart_c3(rng, shape, looks=9, dtype=np.float32):
    """n-look complex-Wishart full-pol samples: 9 real planes
    [C11, C22, C33, C12re, C12im, C13re, C13im, C23re, C23im] of `shape`."""
    def cn(sh):
        return (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(2.0)
    s1 = cn((looks,) + tuple(shape))
    s2 = 0.4 * s1 + 0.9 * cn((looks,) + tuple(shape))
    s3 = 0.2 * s1 - 0.3j * s2 + 0.8 * cn((looks,) + tuple(shape))
    c = lambda a, b: (a * np.conj(b)).mean(axis=0)
    c12, c13, c23 = c(s1, s2), c(s1, s3), c(s2, s3)
    out = [c(s1, s1).real, c(s2, s2).real, c(s3, s3).real, c12.real, c12.imag, c13.real, c13.imag,
           c23.real, c23.imag]
    return [np.ascontiguousarray(o.astype(dtype)) for o in out]


def omnibus_stack_c3(seed, k, ny, nx, looks=9, dtype=np.float32, change_frac=0.1, factor=4.0):
    rng = np.random.default_rng(seed)
    planes = wishart_c3(rng, (k, ny, nx), looks, np.float64)
    if change_frac > 0:
        mask = rng.random((ny, nx)) < change_frac
        t0 = rng.integers(1, max(k, 2), size=(ny, nx))
        gain = np.where((np.arange(k)[:, None, None] >= t0[None]) & mask[None], factor, 1.0)
        planes = [p * gain for p in planes]
    return [np.ascontiguousarray(p.astype(dtype)) for p in planes]


# --------------------------------------------------------------------------------------------------
# Long series (hundreds to thousands of dates)
# --------------------------------------------------------------------------------------------------
# The reference multiplies the determinants of every date of a segment into ONE double
# (nd/_change.pyx:55-65).  On plain data that product leaves the double range after a few hundred
# dates: z = inf, P = NaN, no change anywhere -- and an all-zero map "equals the oracle" for a kernel
# that writes nothing.  long_series_stack keeps the running product of most pixels in range: every
# pixel is scaled so that its mean log-determinant is 0, and its changes barely move the determinant
# (a power swap between the channels and a phase turn of C12 leave C11 C22 - |C12|^2 as it was; a
# power step of one channel moves it by a factor of at most 1.35).  Degenerate pixels are then planted
# on purpose, in row 0, at known places.
LONG_DATES = (190, 193, 200, 1020, 1025, 2040, 2050, 2100, 3000)   # change dates around 192, 1024, 2048
PLANT = ('subnormal', 'underflow', 'overflow', 'nodata', 'nan', 'inf', 'negative', 'not_psd')


def long_series_stack(seed, k, ny, nx, looks=9, dtype=np.float32, change_frac=0.6, plant=True):
    """Planar (time, y, x) dual-pol stack of k dates whose running products of determinants stay in
    the normal double range for the ordinary pixels.  Returns (planes, planted): 4 arrays (k, ny, nx)
    and a dict {kind: [(y, x), ...]} of the pixels planted in row 0 (empty without `plant`):
      subnormal: the dates up to t scaled down so that the product over dates 0 .. t reaches 2^-1050
          (a subnormal double) at a date t chosen per pixel, the dates behind t scaled up so that the
          whole-series product is back at 1: the global test stays finite, the precision lost is kept;
      underflow / overflow: every date scaled so that the product over dates 0 .. t reaches 2^-1180
          (0 in double) / 2^+1040 (inf) at a date t chosen per pixel, and keeps moving behind it;
      nodata (all zero), nan (one NaN date), inf (an inf on the last date), negative (C11 < 0 on some
          dates), not_psd (|C12|^2 > C11 C22 on some dates)."""
    rng = np.random.default_rng(seed)
    shape = (k, ny, nx)

    def cn():
        return (rng.standard_normal((looks,) + shape) + 1j * rng.standard_normal((looks,) + shape)) / np.sqrt(2.0)
    t = np.arange(k)[:, None, None]
    p1 = np.ones(shape)
    p2 = np.full(shape, 0.5)
    phase = np.zeros(shape)
    changing = rng.random((ny, nx)) < change_frac
    dates = [d for d in LONG_DATES if d < k - 1] + [k - 1]
    for y in range(ny):
        for x in range(nx):
            if not changing[y, x]:
                continue
            for _ in range(int(rng.integers(1, 4))):
                t0 = int(rng.choice(dates)) if rng.random() < 0.7 else int(rng.integers(1, k))
                after = t[:, 0, 0] >= t0
                kind = int(rng.integers(0, 3))
                if kind == 0:          # power swap: C11 up, C22 down by the same factor
                    r = rng.uniform(1.3, 1.8)
                    p1[after, y, x] *= r
                    p2[after, y, x] /= r
                elif kind == 1:        # phase turn of C12
                    phase[after, y, x] += rng.uniform(0.6, 1.6) * rng.choice([-1.0, 1.0])
                else:                  # moderate power step of one channel
                    r = rng.uniform(1.2, 1.35) ** rng.choice([-1.0, 1.0])
                    (p1 if rng.random() < 0.5 else p2)[after, y, x] *= r
    rho = 0.75
    s1 = cn()
    s2 = rho * np.exp(1j * phase) * s1 + np.sqrt(1 - rho ** 2) * cn()
    s1 *= np.sqrt(p1)
    s2 *= np.sqrt(p2)
    c11 = (np.abs(s1) ** 2).mean(axis=0)
    c22 = (np.abs(s2) ** 2).mean(axis=0)
    c12 = (s1 * np.conj(s2)).mean(axis=0)
    del s1, s2
    # every pixel's mean log-determinant to 0: all four planes times exp(-mean / 2)
    logdet = np.log(c11 * c22 - np.abs(c12) ** 2)
    g = np.exp(-0.5 * logdet.mean(axis=0))[None]
    planes = [c11 * g, c12.real * g, c12.imag * g, c22 * g]
    planted = {kind: [] for kind in PLANT} if plant else {}
    if plant:
        if nx < len(PLANT) * 2:
            raise ValueError('planting needs at least %d pixels per row' % (2 * len(PLANT)))
        # the log2 of the running product over dates 0 .. t that row 0 has now (its values as stored)
        cast = [np.asarray(p[:, 0, :].astype(dtype), np.float64) for p in planes]
        cum = np.cumsum(np.log2(np.abs(cast[0] * cast[3] - (cast[1] ** 2 + cast[2] ** 2))), axis=0)
        targets = {'underflow': -1180.0, 'overflow': 1040.0}
        for i, kind in enumerate(PLANT):
            for x in (2 * i, 2 * i + 1):
                planted[kind].append((0, x))
                if kind == 'subnormal':
                    tx = int(rng.integers(k // 4, 3 * k // 4))
                    down = (-1050.0 - cum[tx, x]) / (tx + 1)
                    up = -(cum[k - 1, x] + (tx + 1) * down) / (k - 1 - tx)
                    f = np.where(np.arange(k) <= tx, 2.0 ** (down / 2), 2.0 ** (up / 2))
                    for p in planes:
                        p[:, 0, x] *= f
                elif kind in targets:
                    tx = int(rng.integers(k // 4, k))            # the date the product reaches the target
                    per_date = (targets[kind] - cum[tx, x]) / (tx + 1)     # log2 of the determinant's factor
                    for p in planes:
                        p[:, 0, x] *= 2.0 ** (per_date / 2)
                elif kind == 'nodata':
                    for p in planes:
                        p[:, 0, x] = 0.0
                elif kind == 'nan':
                    planes[int(rng.integers(0, 4))][int(rng.integers(0, k)), 0, x] = np.nan
                elif kind == 'inf':
                    planes[3][k - 1, 0, x] = np.inf
                elif kind == 'negative':
                    m = rng.random(k) < 0.05
                    planes[0][m, 0, x] *= -1.0
                elif kind == 'not_psd':
                    m = rng.random(k) < 0.05
                    planes[1][m, 0, x] *= 6.0
    return [np.ascontiguousarray(p.astype(dtype)) for p in planes], planted


def running_products(planes, y, x):
    """The reference's running product of determinants over dates 0 .. t of pixel (y, x) of planar
    (time, y, x) planes: the determinant in the planes' own type, the product in double, in date order
    (nd/_change.pyx:55-65)."""
    a, b, c, d = (p[:, y, x] for p in planes)
    det = (a * d) - ((b * b) + (c * c))
    out = np.empty(len(det))
    prod = 1.0
    with np.errstate(all='ignore'):
        for i, v in enumerate(det.astype(np.float64)):
            prod = prod * v
            out[i] = prod
    return out


def long_series_nonvacuity(k, maps, P, npix):
    """What makes a long-series parity case worth its time, from the ORACLE's output: `maps` {alpha: uint8
    (y, x, time)} of one stack at several thresholds, `P` its global-test P raster.  Raises AssertionError
    where a kernel that writes nothing, or stops searching at date 192 or 2047, could still pass.  Returns
    {alpha: (changes, changed pixels)} and the number of P = NaN pixels for the record."""
    nnan = int(np.isnan(P).sum())
    assert nnan < 0.15 * npix, '%d of %d pixels have P = NaN' % (nnan, npix)
    counts = {}
    for alpha in sorted(maps):
        ch = maps[alpha]
        px = int(ch.any(axis=-1).sum())
        assert px >= 0.15 * npix, 'alpha %g: only %d of %d pixels change' % (alpha, px, npix)
        dates = np.nonzero(ch)[-1]
        assert (dates >= 192).any(), 'alpha %g: no change at date 192 or later' % alpha
        if k >= 2048:
            assert (dates >= 2047).any(), 'alpha %g: no change at date 2047 or later' % alpha
        counts[alpha] = (int(ch.sum()), px)
    al = sorted(counts)
    for a, b in zip(al, al[1:]):
        assert counts[a][0] != counts[b][0], 'alpha %g and %g: the same number of changes' % (a, b)
    return counts, nnan
