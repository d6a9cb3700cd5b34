"""Vectorised numpy restatement of Coregistration (nd/warp.py:1104-1163) as scikit-image 0.18 computes
it: skimage.registration.phase_cross_correlation(C11[t], C11[ref], upsample_factor=u) for the shift,
skimage.transform.warp(v[t], AffineTransform(translation=(s_col, s_row)), order=3) for every variable.
Test infrastructure: the GPU path is checked against it where no recorded skimage output exists."""
import numpy as np

try:
    import scipy.fft as _fft          # keeps single precision, as skimage 0.18 calls it
except Exception:                     # pragma: no cover - numpy's FFT works in double precision
    _fft = np.fft

NAN_MESSAGE = ('NaN values found, please remove NaNs from your input data or use the '
               '`reference_mask`/`moving_mask` keywords, eg: phase_cross_correlation(reference_image, '
               'moving_image, reference_mask=~np.isnan(reference_image), '
               'moving_mask=~np.isnan(moving_image))')


# ------------------------------------------------------------------ shift
def upsampled_dft(data, region, u, offsets):
    """skimage.registration._phase_cross_correlation._upsampled_dft: last axis first."""
    for n, off in list(zip(data.shape, offsets))[::-1]:
        kernel = (np.arange(region) - off)[:, None] * np.fft.fftfreq(n, u)
        kernel = np.exp(-(1j * 2 * np.pi) * kernel)
        data = np.tensordot(kernel, data, axes=(1, -1))
    return data


def phase_shift(src, ref, u=1):
    """(row, col) shift of `src` against `ref`; raises ValueError(NAN_MESSAGE) where skimage does."""
    F_s = _fft.fftn(src)
    F_r = _fft.fftn(ref)
    P = F_s * F_r.conj()
    cc = _fft.ifftn(P)
    peak = np.unravel_index(np.argmax(np.abs(cc)), cc.shape)
    mid = np.array([np.fix(n / 2) for n in cc.shape])
    s = np.stack(peak).astype(np.float64)
    s[s > mid] -= np.array(cc.shape)[s > mid]
    if u == 1:
        ccmax = cc[peak]
    else:
        s = np.round(s * u) / u
        region = np.ceil(u * 1.5)
        d = np.fix(region / 2.0)
        uu = np.array(u, dtype=np.float64)
        CC = upsampled_dft(P.conj(), int(region), uu, d - s * uu).conj()
        peak = np.unravel_index(np.argmax(np.abs(CC)), CC.shape)
        ccmax = CC[peak]
        s = s + (np.stack(peak).astype(np.float64) - d) / uu
    for i, n in enumerate(cc.shape):
        if n == 1:
            s[i] = 0
    amp_s = np.sum(np.real(F_s * F_s.conj()))
    amp_r = np.sum(np.real(F_r * F_r.conj()))
    if np.isnan(ccmax) or np.isnan(amp_s) or np.isnan(amp_r):
        raise ValueError(NAN_MESSAGE)
    return s


# ------------------------------------------------------------------ warp
def cubic(x, f0, f1, f2, f3):
    """skimage's cubic_interpolation for the array type: double arithmetic for float64; for float32
    the two tap differences in float, the rest in double, the result rounded to float."""
    if np.asarray(f0).dtype == np.float32:
        d20 = (f2 - f0).astype(np.float64)
        d12 = (f1 - f2).astype(np.float64)
        x, f0, f1, f2, f3 = (np.asarray(v, np.float64) for v in (x, f0, f1, f2, f3))
        return (f1 + 0.5 * x * (d20 + x * (2.0 * f0 - 5.0 * f1 + 4.0 * f2 - f3
                                           + x * (3.0 * d12 + f3 - f0)))).astype(np.float32)
    return f1 + 0.5 * x * (f2 - f0 + x * (2.0 * f0 - 5.0 * f1 + 4.0 * f2 - f3 + x * (3.0 * (f1 - f2) + f3 - f0)))


def coordinates(n, shift, dtype):
    """floor and fraction of i + shift, formed in `dtype` (skimage casts its matrix to the image type)."""
    T = np.dtype(dtype).type
    v = np.arange(n, dtype=dtype) + (T(shift) if np.isfinite(shift) else T(0))
    v = np.minimum(np.maximum(v, T(-4)), T(n + 4))
    f = np.floor(v)
    return f.astype(np.int64), (v - f).astype(dtype)


def _taps(a, rows, cols):
    """a[rows[:, None], cols[None, :]] with 0 outside the plane."""
    nr, nc = a.shape
    ok = (rows[:, None] >= 0) & (rows[:, None] < nr) & (cols[None, :] >= 0) & (cols[None, :] < nc)
    v = a[np.clip(rows, 0, nr - 1)[:, None], np.clip(cols, 0, nc - 1)[None, :]]
    return np.where(ok, v, a.dtype.type(0))


def interpolate(a, s_row, s_col, rows=None, cols=None):
    """The bicubic samples of plane `a` at (r + s_row, c + s_col) for the output rows x cols given
    (all by default), before the clip."""
    nr, nc = a.shape
    ri, rf = coordinates(nr, s_row, a.dtype)
    ci, cf = coordinates(nc, s_col, a.dtype)
    rows = np.arange(nr) if rows is None else np.asarray(rows)
    cols = np.arange(nc) if cols is None else np.asarray(cols)
    r0, xr = ri[rows], rf[rows]
    c0, xc = ci[cols], cf[cols]
    h = []
    for i in range(4):
        tr = r0 - 1 + i
        f = [_taps(a, tr, c0 - 1 + j) for j in range(4)]
        h.append(cubic(xc[None, :], *f))
    return cubic(xr[:, None], *h)


def clip_preserve(out, lo, hi):
    """skimage's _clip_warp_output for mode 'constant', cval 0."""
    mask = out == 0
    preserve = not (lo <= 0 <= hi)
    with np.errstate(invalid='ignore'):
        out = np.clip(out, lo, hi)
    if preserve:
        out[mask] = 0
    return out


def warp_plane(a, s_row, s_col):
    return clip_preserve(interpolate(a, s_row, s_col), a.min(), a.max())


def warp_pixels(a, s_row, s_col, rows, cols):
    """warp_plane(a, ...)[rows][:, cols] without warping the whole plane."""
    return clip_preserve(interpolate(a, s_row, s_col, rows, cols), a.min(), a.max())


# ------------------------------------------------------------------ the algorithm
def shifts(c11, reference=0, upsampling=10):
    """(k, 2) shifts of the planar (time, y, x) C11 stack, 0 for the reference date."""
    out = np.zeros((c11.shape[0], 2))
    for t in range(c11.shape[0]):
        if t != reference:
            out[t] = phase_shift(c11[t], c11[reference], upsampling)
    return out


def warp_stack(stack, sh, reference):
    out = stack.copy()
    for t in range(stack.shape[0]):
        if t != reference:
            out[t] = warp_plane(stack[t], sh[t, 0], sh[t, 1])
    return out


def coregister(planes, reference=0, upsampling=10):
    """planes: {name: planar (time, y, x) array} including 'C11' -> ({name: warped}, shifts)."""
    sh = shifts(planes['C11'], reference, upsampling)
    return {n: warp_stack(a, sh, reference) for n, a in planes.items()}, sh
