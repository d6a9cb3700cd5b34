"""change_segments restated in numpy: the direction of every declared change and the segment means.

An explicit loop over the dates, vectorised over the pixels, float64 throughout, every operation in the order
the definition writes it (README.md, "Direction of change and segment means").  Per pixel:

    l = 0; s_p = 0.0; m = 0.0
    for t = 0 .. k-1:
        if t >= 1 and c[t] != 0:
            mean_p = s_p / m;  d_p = (double) x_p[t] - mean_p
            direction[t] = code(d);  means_p[l .. t-1] = (T) mean_p
            l = t; s_p = 0.0; m = 0.0
        else: direction[t] = 0
        s_p = s_p + (double) x_p[t]; m = m + 1.0
    means_p[l .. k-1] = (T)(s_p / m)

numpy only; nothing here knows how the kernel walks the data."""
import numpy as np

STRUCTURES = {'diag': (1, 2, 3), 'c2': (4,), 'c3': (9,)}


def code(d, structure):
    """d: the difference planes (float64 arrays of one shape).  1 positive definite, 2 negative definite, 3
    anything else -- a comparison with NaN is False, so every NaN lands in 3."""
    if structure == 'diag':
        pos = np.ones(d[0].shape, bool)
        neg = np.ones(d[0].shape, bool)
        for dp in d:
            pos &= dp > 0
            neg &= dp < 0
    elif structure == 'c2':
        d0, d1, d2, d3 = d
        a = d0
        det = (d0 * d3) - ((d1 * d1) + (d2 * d2))
        pos = (a > 0) & (det > 0)
        neg = (a < 0) & (det > 0)
    else:
        d11, d22, d33, r12, i12, r13, i13, r23, i23 = d
        n12 = r12 * r12 + i12 * i12
        n13 = r13 * r13 + i13 * i13
        n23 = r23 * r23 + i23 * i23
        m1 = d11
        m2 = (d11 * d22) - n12
        tr = ((r12 * r23) - (i12 * i23)) * r13 + ((r12 * i23) + (i12 * r23)) * i13
        m3 = (((d11 * d22) * d33) + (2.0 * tr)) - (((d11 * n23) + (d22 * n13)) + (d33 * n12))
        pos = (m1 > 0) & (m2 > 0) & (m3 > 0)
        neg = (m1 < 0) & (m2 > 0) & (m3 < 0)
    return np.where(pos, 1, np.where(neg, 2, 3)).astype(np.int8)


def change_segments(planes, change, structure):
    """planes: P arrays (k, ny, nx) of one float type T; change: (ny, nx, k), non-zero = date t opens a segment.
    Returns direction int8 (ny, nx, k) and the P mean planes (k, ny, nx) of type T."""
    assert len(planes) in STRUCTURES[structure]
    T = planes[0].dtype
    k, ny, nx = planes[0].shape
    c = np.moveaxis(np.asarray(change) != 0, -1, 0)              # (k, ny, nx)
    direction = np.zeros((k, ny, nx), np.int8)
    means = [np.empty((k, ny, nx), T) for _ in planes]
    start = np.zeros((ny, nx), np.int64)
    s = [np.zeros((ny, nx), np.float64) for _ in planes]
    m = np.zeros((ny, nx), np.float64)
    dates = np.arange(k)[:, None, None]
    with np.errstate(all='ignore'):
        for t in range(k):
            x = [p[t].astype(np.float64) for p in planes]
            if t >= 1 and c[t].any():
                f = c[t]
                mean = [sp / m for sp in s]
                d = [xp - mp for xp, mp in zip(x, mean)]
                direction[t] = np.where(f, code(d, structure), 0)
                lo = int(start[f].min())                                     # (only a shortcut: no closing segment starts earlier)
                fill = f[None] & (dates[lo:t] >= start[None])                # dates l .. t-1 of the closing pixels
                for p in range(len(planes)):
                    np.copyto(means[p][lo:t], np.broadcast_to(mean[p].astype(T)[None], fill.shape), where=fill)
                    s[p] = np.where(f, 0.0, s[p])
                start = np.where(f, t, start)
                m = np.where(f, 0.0, m)
            for p in range(len(planes)):
                s[p] = s[p] + x[p]
            m = m + 1.0
        lo = int(start.min())
        fill = dates[lo:] >= start[None]
        for p in range(len(planes)):
            np.copyto(means[p][lo:], np.broadcast_to((s[p] / m).astype(T)[None], fill.shape), where=fill)
    return np.ascontiguousarray(np.moveaxis(direction, 0, -1)), means
