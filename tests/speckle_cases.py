"""What the speckle GPU tests share: sources with planted corner values, the device call in each layout, the
comparison, the case tables and the random cases of tests/test_speckle_fuzz_gpu.py.  The restatement is
tests/speckle_ref.py."""
import numpy as np

from tests import speckle_ref as ref

WIDTHS = (1, 3, 5, 7, 9, 11, 13, 31)            # every unrolled instantiation, the loop form, both ends
LAYOUTS = ('planar', 'pixel', 'crop')
SENTINEL = -777.25                              # what outputs hold before the call: an unwritten element shows


def tiles():
    """(TY, TX) of the kernels as built, and of the one-launch multitemporal form"""
    from nd_amd import kernels as K
    return K.SPECKLE_TILE, K.SPECKLE_HOT_TILE


def plane_shapes(ty, tx, w=7):
    """the smallest planes at which a tiled kernel can go wrong: windows larger than the plane, one short of a
    tile, a tile, one more, several tiles with a ragged edge"""
    return [(1, 1), (1, 2), (2, 5), (3, 3), (ty - 1, tx - 1), (ty, tx), (ty + 1, tx + 1),
            (2 * ty + 3, tx + w // 2)]


def speckle(rng, shape, dtype=np.float32, looks=4.0):
    """gamma(L, 1 / L) speckle of mean 1 on a smooth backscatter pattern"""
    a = rng.gamma(looks, 1.0 / looks, size=shape)
    if np.dtype(dtype).kind != 'f':
        return (a * 40).astype(dtype)
    return a.astype(dtype)


def plant(a, rng, seams=()):
    """NaN, +inf, -inf, 0, a negative and a subnormal sample into the float stack `a` (k, ny, nx): on the border and
    around the (row, column) positions of `seams`, each on a plane of its own where the stack has enough"""
    if a.dtype.kind != 'f':
        return a
    k, ny, nx = a.shape
    tiny = np.finfo(a.dtype).tiny
    values = [np.nan, np.inf, -np.inf, 0.0, -3.5, tiny / 4]
    spots = [(0, 0), (ny - 1, nx - 1), (0, nx // 2), (ny // 2, 0)]
    for (y, x) in seams:
        spots += [(y - 1, x - 1), (y, x), (y, x - 1), (y - 1, x)]
    spots = [(y, x) for y, x in spots if 0 <= y < ny and 0 <= x < nx]
    for i, (y, x) in enumerate(spots):
        a[(i * 5) % k, y, x] = values[int(rng.integers(len(values)))]
    return a


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view('u%d' % a.dtype.itemsize)


def assert_same(got, want):
    """equal everywhere: the same shape and type, NaN at the same positions, the same bits at every other element"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), 'NaN at %d positions of the device, %d of the restatement' % (gn.sum(), wn.sum())
    same = bits(got)[~gn] == bits(want)[~wn]
    assert same.all(), '%d of %d elements differ' % ((~same).sum(), same.size)


def _upload(torch, dev, src, layout):
    """src numpy (k, ny, nx) -> (device tensor, dims, back) in `layout`; `back` brings a result to (k, ny, nx)"""
    if layout == 'pixel':
        dims, host, back = ('y', 'x', 'time'), np.ascontiguousarray(np.moveaxis(src, 0, -1)), (-1, 0)
    else:
        dims, host, back = ('time', 'y', 'x'), np.ascontiguousarray(src), None
    if layout == 'crop':
        # a window of a larger tensor: not contiguous, and it starts at a storage offset
        big = np.full([n + 5 for n in host.shape], 3.0, host.dtype)
        window = tuple(slice(2, 2 + n) for n in host.shape)
        big[window] = host
        t = torch.from_numpy(big).to(dev)[window]
        assert t.storage_offset() > 0
    else:
        t = torch.from_numpy(host).to(dev)
    return t, dims, back


def _out_dtype(torch, t):
    return t.dtype if t.is_floating_point() else torch.float64


def _output(torch, t, strided):
    """-> (out, check): a sentinel-filled output of t's shape, contiguous or every second element of the last axis of
    a larger buffer; check() asserts that nothing outside `out` was written"""
    dt = _out_dtype(torch, t)
    shape = list(t.shape)
    if not strided:
        out = torch.full(shape, SENTINEL, dtype=dt, device=t.device)
        return out, lambda: None
    buf = torch.full([n + 3 for n in shape[:-1]] + [2 * shape[-1] + 1], SENTINEL, dtype=dt, device=t.device)
    window = tuple(slice(1, 1 + n) for n in shape[:-1]) + (slice(1, 1 + 2 * shape[-1], 2),)
    out = buf[window]

    def check():
        rest = buf.clone()
        rest[window] = SENTINEL
        assert bool((rest == SENTINEL).all()), 'elements outside the strided out were written'
    return out, check


def _download(got, back, shape):
    got = got.cpu().numpy()
    if back:
        got = np.moveaxis(got, *back)
    return np.ascontiguousarray(got).reshape(shape)


def device_lee(K, src, w, looks, method, layout='planar', strided_out=False):
    """src numpy (k, ny, nx) through kernels.speckle_lee -> numpy (k, ny, nx)"""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    t, dims, back = _upload(torch, dev, src, layout)
    out, check = _output(torch, t, strided_out)
    got = K.speckle_lee(t, w, looks, method, out=out, dims=dims)
    assert got is out
    check()
    return _download(got, back, src.shape)


def device_multitemporal(K, variables, w, layout='planar', strided_out=False):
    """a list of numpy (k, ny, nx) through kernels.speckle_multitemporal, jointly -> a list of numpy (k, ny, nx)"""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    ups = [_upload(torch, dev, v, layout) for v in variables]
    outs = [_output(torch, u[0], strided_out) for u in ups]
    got = K.speckle_multitemporal([u[0] for u in ups], w, dims=ups[0][1], out=[o[0] for o in outs])
    for g, (o, check) in zip(got, outs):
        assert g is o
        check()
    return [_download(g, ups[0][2], variables[0].shape) for g in got]


def check_lee(K, src, w, looks=1.0, method='lee', **kw):
    got = device_lee(K, src, w, looks, method, **kw)
    assert_same(got, ref.lee(src, w, looks, method))
    return got


def check_multitemporal(K, variables, w, **kw):
    got = device_multitemporal(K, variables, w, **kw)
    want = ref.multitemporal(list(variables), w)
    for g, v in zip(got, want):
        assert_same(g, v)
    return got


# ---- the random cases of the fuzz test ---------------------------------------------------------------------------
def random_case(rng):
    ny, nx = (int(v) for v in rng.integers(1, 151, size=2))
    while ny * nx > 5000:
        ny, nx = max(1, ny // 2), max(1, nx * 2 // 3)
    filt = str(rng.choice(['lee', 'multitemporal']))
    w = int(rng.choice(WIDTHS + tuple(range(1, 32, 2))))
    dtype = np.dtype(rng.choice(['float32', 'float32', 'float64', 'int16']))
    case = {'filter': filt, 'w': w, 'dtype': dtype, 'layout': str(rng.choice(LAYOUTS)),
            'strided_out': bool(rng.random() < 0.3)}
    if filt == 'lee':
        k = int(rng.integers(1, 4))
        nvar = 1
        case['looks'] = float(rng.choice([1.0, 4.4, 0.7, 16.0]))
        case['method'] = str(rng.choice(['lee', 'kuan']))
    else:
        nvar = int(rng.choice([1, 1, 2, 3, 4]))
        # around the limit of the one-launch form now and then
        k = int(rng.integers(1, 7)) if rng.random() < 0.8 else int(rng.integers(30, 36)) // nvar + int(rng.integers(0, 2))
        k = max(k, 1)
        while k * nvar * ny * nx > 40000:
            ny, nx = max(1, ny * 2 // 3), max(1, nx * 2 // 3)
    seams = [(int(rng.integers(0, ny + 1)), int(rng.integers(0, nx + 1))), (8, 64), (32, 64)]
    case['variables'] = []
    for _ in range(nvar):
        a = speckle(rng, (k, ny, nx), dtype, looks=float(rng.choice([1.0, 4.0])))
        if rng.random() < 0.5:
            a = plant(a, rng, seams)
        case['variables'].append(a)
    return case


def describe(case):
    v = case['variables']
    return {key: val for key, val in case.items() if key != 'variables'} | {'shape': v[0].shape, 'nvar': len(v)}


def run_case(K, case):
    """the device result and the restatement of a random case, as lists of arrays"""
    v = case['variables']
    if case['filter'] == 'lee':
        got = [device_lee(K, v[0], case['w'], case['looks'], case['method'], case['layout'], case['strided_out'])]
        want = [ref.lee(v[0], case['w'], case['looks'], case['method'])]
    else:
        got = device_multitemporal(K, v, case['w'], case['layout'], case['strided_out'])
        want = ref.multitemporal(list(v), case['w'])
    return got, want
