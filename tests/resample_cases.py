"""What the resample GPU tests share: sources, the device call in each layout, the comparison, and the random cases of
tests/test_resample_fuzz_gpu.py.  The restatement is tests/resample_ref.py."""
import numpy as np

from tests import resample_ref as ref

WEIGHTED = ('bilinear', 'cubic', 'average')
LAYOUTS = ('planar', 'pixel')


def source(rng, shape, dtype=np.float32, nonfinite=0.0):
    """gamma-distributed intensities (the speckle of a SAR plane), with a share of NaN / +inf / -inf samples"""
    a = rng.gamma(2.0, 0.5, size=shape)
    if np.dtype(dtype).kind != 'f':
        return (a * 40).astype(dtype)
    a = a.astype(dtype)
    if nonfinite:
        bad = rng.random(shape) < nonfinite
        a[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype), size=int(bad.sum()))
    return a


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view('u%d' % a.dtype.itemsize) if a.dtype != np.bool_ else a.view(np.uint8)


def assert_same(got, want, payloads=False):
    """equal everywhere: the same shape and type, NaN at the same positions, the same bits at every other element
    (payloads: the bits of the NaNs too, as nearest must deliver them)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind == 'f' and not payloads:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), 'NaN at %d positions of the device, %d of the restatement' % (gn.sum(), wn.sum())
        same = bits(got)[~gn] == bits(want)[~wn]
        assert same.all(), '%d of %d elements differ' % ((~same).sum(), same.size)
    else:
        same = bits(got) == bits(want)
        assert same.all(), '%d of %d elements differ' % ((~same).sum(), same.size)


def device_regrid(K, src, tr_s, tr_d, H, W, method, layout='planar', fill=None, crop=False, strided_out=False,
                  tables=None):
    """src numpy (P, ny, nx) through kernels.resample in `layout` -> numpy (P, H, W).  crop: the source is a window of
    a larger tensor; strided_out: the result goes into every second element of a larger buffer."""
    import torch
    P, ny, nx = src.shape
    dev = torch.device('cuda', torch.cuda.current_device())
    if tables is None:
        tables = (K.resample_axis(ny, H, ref.axis_of(tr_s, 'y'), ref.axis_of(tr_d, 'y'), method),
                  K.resample_axis(nx, W, ref.axis_of(tr_s, 'x'), ref.axis_of(tr_d, 'x'), method))
    if layout == 'planar':
        dims, host, oshape, back = ('time', 'y', 'x'), src, (P, H, W), None
    elif layout == 'pixel':
        dims, host, oshape, back = ('y', 'x', 'time'), np.moveaxis(src, 0, -1), (H, W, P), (-1, 0)
    else:
        assert layout == '2d' and P == 1
        dims, host, oshape, back = ('y', 'x'), src[0], (H, W), None
    host = np.ascontiguousarray(host)
    if crop:
        big = np.zeros([n + 5 for n in host.shape], host.dtype)
        window = tuple(slice(2, 2 + n) for n in host.shape)
        big[window] = host
        t = torch.from_numpy(big).to(dev)[window]
        assert not t.is_contiguous() or t.numel() <= 1
    else:
        t = torch.from_numpy(host).to(dev)
    out = None
    if strided_out:
        odt = t.dtype if (method == 'nearest' or t.is_floating_point()) else torch.float64
        buf = torch.full([n + 3 for n in oshape[:-1]] + [2 * oshape[-1] + 1], 1, dtype=odt, device=dev)
        out = buf[tuple(slice(1, 1 + n) for n in oshape[:-1]) + (slice(1, 1 + 2 * oshape[-1], 2),)]
    got = K.resample(t, tables[0], tables[1], dims=dims, fill=fill, out=out)
    if strided_out:
        assert got is out
        untouched = buf.clone()
        untouched[tuple(slice(1, 1 + n) for n in oshape[:-1]) + (slice(1, 1 + 2 * oshape[-1], 2),)] = 1
        assert bool((untouched == 1).all()), 'elements outside the strided out were written'
    got = got.cpu().numpy()
    if back:
        got = np.moveaxis(got, *back)
    return got.reshape(P, H, W)


def check(K, src, tr_s, tr_d, H, W, method, layout='planar', fill=None, **kw):
    got = device_regrid(K, src, tr_s, tr_d, H, W, method, layout, fill=fill, **kw)
    want = ref.regrid(src, tr_s, tr_d, H, W, method, fill=fill)
    assert_same(got, want, payloads=method == 'nearest')
    return got


def whole_extent(ny, nx, H, W, a=10.0, e=-10.0, c=500.0, f=900.0):
    """source and destination transforms of a resize of the whole extent"""
    return (a, 0.0, c, 0.0, e, f), (a * nx / W, 0.0, c, 0.0, e * ny / H, f)


# ---- the random cases of the fuzz test ---------------------------------------------------------------------------
def random_case(rng):
    ny, nx = (int(v) for v in rng.integers(1, 201, size=2))
    while ny * nx > 6000:
        ny, nx = max(1, ny // 2), max(1, nx * 2 // 3)
    method = str(rng.choice(ref.METHODS))
    ratios = np.exp(rng.uniform(np.log(0.05), np.log(40.0), size=2))
    for d in range(2):
        if rng.random() < 0.3:
            ratios[d] = rng.choice([0.25, 0.5, 1.0, 2.0, 2.5, 4.0])
    a_s, e_s = rng.choice([10.0, -10.0, 0.3, -1.0], size=2)
    c_s, f_s = rng.uniform(-50, 50, size=2)
    a_d = a_s * ratios[1] * (-1.0 if rng.random() < 0.15 else 1.0)
    e_d = e_s * ratios[0] * (-1.0 if rng.random() < 0.15 else 1.0)
    # the destination starts within or a little outside the source; now and then on a source pixel's corner
    off = rng.uniform(-0.2, 0.7, size=2) * (nx, ny)
    if rng.random() < 0.3:
        off = np.round(off)
    c_d = c_s + a_s * off[0] + (a_s * nx * 0.9 if a_d * a_s < 0 else 0.0)
    f_d = f_s + e_s * off[1] + (e_s * ny * 0.9 if e_d * e_s < 0 else 0.0)
    W = int(np.clip(nx / ratios[1] * rng.uniform(0.3, 1.2), 1, 200))
    H = int(np.clip(ny / ratios[0] * rng.uniform(0.3, 1.2), 1, 200))
    while H * W > 6000:
        H, W = max(1, H // 2), max(1, W * 2 // 3)
    if method == 'nearest':
        dtype = rng.choice([np.uint8, np.bool_, np.int16, np.int32, np.int64, np.float32, np.float64])
    else:
        dtype = rng.choice([np.float32, np.float64, np.float32, np.float64, np.int32, np.uint8])
    P = int(rng.choice([1, 1, 2, 3, 5]))
    layout = str(rng.choice(LAYOUTS + (('2d',) if P == 1 else ())))
    src = source(rng, (P, ny, nx), dtype, nonfinite=float(rng.choice([0.0, 0.0, 0.02])))
    fill = None if rng.random() < 0.7 else (float(rng.integers(-3, 4)) if np.dtype(dtype).kind == 'f' or
                                            method != 'nearest' else int(rng.integers(0, 2)))
    return dict(src=src, tr_s=(a_s, 0.0, c_s, 0.0, e_s, f_s), tr_d=(a_d, 0.0, c_d, 0.0, e_d, f_d), H=H, W=W,
                method=method, layout=layout, fill=fill, crop=bool(rng.random() < 0.3),
                strided_out=bool(rng.random() < 0.3))


def describe(case):
    return {k: (v if k != 'src' else (v.shape, str(v.dtype))) for k, v in case.items()}
