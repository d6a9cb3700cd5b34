"""The numpy restatement of the speckle filters (README "Speckle filters", include/nd_amd.h): literal loops over the
taps, in the definition's order, float64 throughout, vectorised over the pixels only.  numpy adds and multiplies
element by element without fusing, so every bracket below is one rounding, as in the library.

    moments(x, w)             -> S1, S2 of every (y, x) plane of x (..., ny, nx)
    lee(x, w, looks, method)  -> the Lee / Kuan filter of every plane
    multitemporal(vars, w)    -> the Quegan & Yu filter of C variables of (k, ny, nx), jointly
"""
import numpy as np


def refl(i, n):
    """scipy's 'reflect' index map, periodic: p = i mod 2n; p if p < n else 2n - 1 - p"""
    p = np.mod(np.asarray(i, np.int64), 2 * n)
    return np.where(p < n, p, 2 * n - 1 - p)


def out_dtype(x):
    x = np.asarray(x)
    return x.dtype if x.dtype in (np.float32, np.float64) else np.dtype(np.float64)


def moments(x, w):
    """Window sums of x and x * x over w x w around every pixel of every plane: row sums with taps ascending, then
    the sum of the w row sums with rows ascending; each sum starts from 0."""
    assert w % 2 == 1 and w >= 1
    xd = np.asarray(x).astype(np.float64)
    ny, nx = xd.shape[-2:]
    R = w // 2
    jj, ii = np.arange(nx), np.arange(ny)
    with np.errstate(all='ignore'):
        h1 = np.zeros(xd.shape)
        h2 = np.zeros(xd.shape)
        for d in range(-R, R + 1):
            v = xd[..., :, refl(jj + d, nx)]
            h1 = h1 + v
            h2 = h2 + v * v
        s1 = np.zeros(xd.shape)
        s2 = np.zeros(xd.shape)
        for d in range(-R, R + 1):
            rows = refl(ii + d, ny)
            s1 = s1 + h1[..., rows, :]
            s2 = s2 + h2[..., rows, :]
    return s1, s2


def lee_weight(x, w, looks, method='lee'):
    """-> m, b of the Lee / Kuan filter (float64)"""
    assert method in ('lee', 'kuan')
    s1, s2 = moments(x, w)
    n = float(w * w)
    cu2 = 1.0 / float(looks)
    with np.errstate(all='ignore'):
        m = s1 / n
        v = s2 / n - m * m
        q = ((m * m) * cu2) / v
        b = 1.0 - q
        if method == 'kuan':
            b = b / (1.0 + cu2)
        b = np.where((v > 0) & (b > 0), b, 0.0)
    return m, b


def lee(x, w, looks, method='lee'):
    m, b = lee_weight(x, w, looks, method)
    xd = np.asarray(x).astype(np.float64)
    with np.errstate(all='ignore'):
        return (m + b * (xd - m)).astype(out_dtype(x))


def multitemporal(variables, w):
    """variables: a list of C arrays (k, ny, nx) of one shape and type (or one such array: C = 1) -> a list (or one
    array) of the filtered stacks.  r runs over the dates in order and, within a date, over the variables."""
    single = isinstance(variables, np.ndarray)
    vs = [variables] if single else list(variables)
    k = vs[0].shape[0]
    n = float(w * w)
    xd = [np.asarray(v).astype(np.float64) for v in vs]
    with np.errstate(all='ignore'):
        m = [moments(v, w)[0] / n for v in vs]
        r = np.zeros(xd[0].shape[1:])
        for t in range(k):
            for c in range(len(vs)):
                r = r + xd[c][t] / m[c][t]
        out = [((m[c] * r) / float(k * len(vs))).astype(out_dtype(vs[c])) for c in range(len(vs))]
    return out[0] if single else out


def multitemporal_looks(looks, k, w, variables=1):
    mm, n = float(k * variables), float(w * w)
    return mm * n * float(looks) / (mm + n - 1.0)
