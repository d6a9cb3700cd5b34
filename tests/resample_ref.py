"""The resampling definition of README.md ("Resampling and reprojection") restated in numpy: what
nd_amd_resample / nd_amd_resample_nearest must reproduce bit for bit.  Tables by a scalar loop in Python floats
(IEEE float64, one rounding per operation, bracketed as the definition writes them); the sums vectorised over the
pixels with a Python loop over the taps in the stated order; nearest by indexing.  Does not import nd_amd."""
import math

import numpy as np

METHODS = ('nearest', 'bilinear', 'cubic', 'average')


def _bilinear(d):
    d = abs(d)
    return 1.0 - d if d < 1.0 else 0.0


def _cubic(d):
    a = -0.5
    d = abs(d)
    if d < 1.0:
        return ((a + 2.0) * d - (a + 3.0)) * (d * d) + 1.0
    if d < 2.0:
        return (((d - 5.0) * d + 8.0) * d - 4.0) * a
    return 0.0


def taps(u, n, rho, method):
    """-> (first source index, [normalised weights]) of an inside sample at u; an empty list makes it outside"""
    if method == 'nearest':
        return int(math.floor(u)), [1.0]
    if method == 'average':
        lo, hi = u - rho / 2.0, u + rho / 2.0
        x0 = max(0, int(math.floor(lo)))
        x1 = min(n, int(math.ceil(hi)))
        w = [min(x + 1.0, hi) - max(float(x), lo) for x in range(x0, x1)]
    else:
        R, phi = (1.0, _bilinear) if method == 'bilinear' else (2.0, _cubic)
        s = max(rho, 1.0)
        x0 = max(0, int(math.floor(u - R * s + 0.5)))
        x1 = min(n, int(math.floor(u + R * s + 0.5)))
        w = [phi((x + 0.5 - u) / s) for x in range(x0, x1)]
    while w and w[0] == 0.0:
        w.pop(0)
        x0 += 1
    while w and w[-1] == 0.0:
        w.pop()
    total = 0.0
    for v in w:
        total = total + v
    return x0, [v / total for v in w]


def axis_table(n, m, src, dst, method):
    """One axis: n source samples with src = (a_s, c_s), m output samples with dst = (a_d, c_d).
    -> start int32 (m), count int32 (m, 0 = outside), weights float64 (T, m) tap-major, T the longest run (at least 1)"""
    if method not in METHODS:
        raise ValueError(method)
    a_s, c_s = float(src[0]), float(src[1])
    a_d, c_d = float(dst[0]), float(dst[1])
    rho = abs(a_d / a_s)
    runs = []
    for j in range(m):
        u = ((c_d + a_d * (j + 0.5)) - c_s) / a_s
        if not (0.0 <= u < n):
            runs.append((0, []))
            continue
        runs.append(taps(u, n, rho, method))
    T = max([len(w) for _, w in runs] + [1])
    start = np.zeros(m, np.int32)
    count = np.zeros(m, np.int32)
    weights = np.zeros((T, m), np.float64)
    for j, (x0, w) in enumerate(runs):
        if w:
            start[j], count[j] = x0, len(w)
            weights[:len(w), j] = w
    return start, count, weights


def default_fill(dtype):
    return np.nan if np.dtype(dtype).kind == 'f' else 0


def resample(src, table_y, table_x, fill=None, nearest=False):
    """src (..., ny, nx) -> (..., H, W).  Weighted: float32 / float64 stay, everything else is computed and
    returned as float64.  nearest: the element itself, of any type."""
    src = np.asarray(src)
    sy, cy, wy = table_y
    sx, cx, wx = table_x
    inside = (cy > 0)[:, None] & (cx > 0)[None, :]
    if nearest:
        out = src[..., np.where(cy > 0, sy, 0)[:, None], np.where(cx > 0, sx, 0)[None, :]]
        fill = default_fill(src.dtype) if fill is None else fill
        return np.where(inside, out, np.array(fill).astype(src.dtype)).astype(src.dtype)
    if src.dtype not in (np.float32, np.float64):
        src = src.astype(np.float64)
    ny, nx = src.shape[-2:]
    H, W = len(sy), len(sx)
    acc = np.zeros(src.shape[:-2] + (H, W), np.float64)
    with np.errstate(all='ignore'):
        for r in range(int(cy.max()) if H else 0):
            rows = np.clip(sy + r, 0, ny - 1)
            h = np.zeros_like(acc)
            for q in range(int(cx.max()) if W else 0):
                cols = np.clip(sx + q, 0, nx - 1)
                v = src[..., rows[:, None], cols[None, :]].astype(np.float64)
                h = np.where((q < cx)[None, :], h + wx[q][None, :] * v, h)
            acc = np.where((r < cy)[:, None], acc + wy[r][:, None] * h, acc)
        fill = np.nan if fill is None else fill
        out = np.where(inside, acc.astype(src.dtype), np.array(fill, np.float64).astype(src.dtype))
    return out.astype(src.dtype)


def axis_of(transform, axis):
    """(a, c) of the x axis or (e, f) of the y axis of a six-tuple (a, b, c, d, e, f)"""
    return (transform[0], transform[2]) if axis == 'x' else (transform[4], transform[5])


def regrid(src, src_transform, dst_transform, H, W, method, fill=None):
    """src (..., ny, nx) on src_transform -> (..., H, W) on dst_transform"""
    ny, nx = np.asarray(src).shape[-2:]
    ty = axis_table(ny, H, axis_of(src_transform, 'y'), axis_of(dst_transform, 'y'), method)
    tx = axis_table(nx, W, axis_of(src_transform, 'x'), axis_of(dst_transform, 'x'), method)
    return resample(src, ty, tx, fill=fill, nearest=method == 'nearest')
