"""What the region GPU tests share: the planes a tiled union-find can go wrong on, the device call in each layout with
strided outputs, the comparison (equal everywhere, no tolerance) and the random cases of
tests/test_regions_fuzz_gpu.py.  The restatement is tests/regions_ref.py."""
import numpy as np

from tests import regions_ref as ref

SHAPES = ((1, 1), (1, 200), (200, 1), (2, 2), (63, 65), (64, 64), (65, 129), (131, 257))
DENSITIES = (0.1, 0.41, 0.59, 0.9)              # 0.41 and 0.59: site percolation at 8 and 4, the longest regions
LAYOUTS = ('planar', 'pixel', 'crop')
DTYPES = ('bool', 'uint8', 'int32', 'int64', 'float32', 'float64')
SENTINEL = -77


def mask(rng, shape, density, dtype='uint8'):
    return (rng.random(shape) < density).astype(dtype)


# ---- adversarial planes ------------------------------------------------------------------------------------------
def serpentine(ny=131, nx=129):
    """every other row full, the full rows joined alternately at the right and left ends: one region whose parent
    chain runs through every tile"""
    a = np.zeros((ny, nx), np.uint8)
    a[0::2] = 1
    for i, y in enumerate(range(1, ny - 1, 2)):
        a[y, nx - 1 if i % 2 == 0 else 0] = 1
    return a


def spiral(n=101):
    """a square spiral of width 1 with gaps of 1"""
    a = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1
    while True:
        moved = False
        while True:
            ny_, nx_ = y + dy, x + dx
            ay, ax = ny_ + dy, nx_ + dx          # the cell behind the next one must be free: keeps a gap of 1
            if not (0 <= ny_ < n and 0 <= nx_ < n) or a[ny_, nx_]:
                break
            if 0 <= ay < n and 0 <= ax < n and a[ay, ax]:
                break
            y, x = ny_, nx_
            a[y, x] = 1
            moved = True
        if not moved:
            return a
        dy, dx = dx, -dy


def checkerboard(ny=70, nx=150):
    yy, xx = np.mgrid[:ny, :nx]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def stripes(ny=67, nx=131):
    """vertical stripes on every other column joined only along the last row, and its three other orientations:
    they separate a region's first pixel from where its merge happens"""
    a = np.zeros((ny, nx), np.uint8)
    a[:, 0::2] = 1
    a[ny - 1, :] = 1
    return {'last_row': a, 'first_row': a[::-1].copy(), 'last_col': a.T.copy(), 'first_col': a.T[:, ::-1].copy()}


def frames(n=133):
    """concentric square frames"""
    yy, xx = np.mgrid[:n, :n]
    ring = np.minimum(np.minimum(yy, xx), np.minimum(n - 1 - yy, n - 1 - xx))
    return (ring % 2 == 0).astype(np.uint8)


def antidiagonal(n=130):
    return np.eye(n, dtype=np.uint8)[:, ::-1].copy()


def adversarial():
    out = {'serpentine': serpentine(), 'serpentine_complement': (1 - serpentine()).astype(np.uint8),
           'spiral': spiral(), 'checkerboard': checkerboard(), 'full': np.ones((70, 150), np.uint8),
           'empty': np.zeros((70, 150), np.uint8), 'frames': frames(), 'antidiagonal': antidiagonal()}
    for k, v in stripes().items():
        out['stripes_' + k] = v
    return out


def class_map(rng, shape, nclass, dtype):
    """a random map of `nclass` classes in patches, 0 among them; floats carry NaN patches and -0.0, int64 two values
    above 2^53 that differ in the last bit"""
    dt = np.dtype(dtype)
    coarse = rng.integers(0, nclass, size=[max(1, -(-n // 3)) for n in shape])
    a = np.kron(coarse, np.ones((3, 3), np.int64))[:shape[0], :shape[1]]
    flip = rng.random(shape) < 0.2
    a = np.where(flip, rng.integers(0, nclass, size=shape), a)
    if dt == np.int64:
        table = np.array([0, 2 ** 53, 2 ** 53 + 1, -5, 7], np.int64)
        return table[a % 5]
    if dt.kind == 'f':
        table = np.array([0.0, 1.5, 1.5 + 2.0 ** -20, -2.0, 3.0], dt)
        v = table[a % 5]
        v[(rng.random(shape) < 0.05) & (v == 0)] = -0.0
        v[rng.random(shape) < 0.05] = np.nan
        return v
    return (a % 5).astype(dt)


# ---- the device calls --------------------------------------------------------------------------------------------
def _upload(torch, dev, stack, layout):
    """stack numpy (k, ny, nx) -> (device tensor, dims, back); `back` brings a result to (k, ny, nx)"""
    if layout == 'pixel':
        dims, host, back = ('y', 'x', 'time'), np.ascontiguousarray(np.moveaxis(stack, 0, -1)), (-1, 0)
    else:
        dims, host, back = ('time', 'y', 'x'), np.ascontiguousarray(stack), None
    if layout == 'crop':
        big = np.full([n + 5 for n in host.shape], 1, host.dtype)
        window = tuple(slice(2, 2 + n) for n in host.shape)
        big[window] = host
        t = torch.from_numpy(big).to(dev)[window]
    else:
        t = torch.from_numpy(host).to(dev)
    return t, dims, back


def _output(torch, t, dtype, strided):
    """-> (out, check): a sentinel-filled output of t's shape and `dtype`, packed, or every second element of the last
    axis of a larger buffer; check() asserts that nothing around `out` was written"""
    shape = list(t.shape)
    fillv = True if dtype == torch.bool else SENTINEL % 251 if dtype == torch.uint8 else SENTINEL
    if not strided:
        return torch.full(shape, fillv, dtype=dtype, device=t.device), lambda: None
    buf = torch.full([n + 3 for n in shape[:-1]] + [2 * shape[-1] + 1], fillv, dtype=dtype, device=t.device)
    window = tuple(slice(1, 1 + n) for n in shape[:-1]) + (slice(1, 1 + 2 * shape[-1], 2),)
    out = buf[window]

    def check():
        rest = buf.clone()
        rest[window] = fillv
        assert bool((rest == fillv).all()), 'elements around the strided output were written'
    return out, check


def _download(got, back, shape):
    got = got.cpu().numpy()
    if back:
        got = np.moveaxis(got, *back)
    return np.ascontiguousarray(got).reshape(shape)


def device_label(K, stack, connectivity=4, background=0, by_value=False, layout='planar', strided=False,
                 area=False):
    """stack numpy (k, ny, nx) through kernels.label_regions -> (labels (k, ny, nx), counts (k,), area or None)"""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    t, dims, back = _upload(torch, dev, stack, layout)
    lab, check_l = _output(torch, t, torch.int32, strided)
    ar, check_a = _output(torch, t, torch.int32, strided) if area else (None, lambda: None)
    res = K.label_regions(t, connectivity, background, by_value, dims=dims, labels=lab, area=ar)
    assert res[0] is lab and (not area or res[2] is ar)
    check_l()
    check_a()
    counts = res[1].cpu().numpy()
    assert counts.dtype == np.int64 and counts.shape == (stack.shape[0],)
    return (_download(lab, back, stack.shape), counts, _download(ar, back, stack.shape) if area else None)


def device_sizes(K, stack, connectivity=4, background=0, by_value=False, layout='planar'):
    """-> a list of int64 arrays, one per plane, through kernels.label_regions and kernels.region_sizes"""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    t, dims, back = _upload(torch, dev, stack, layout)
    labels, counts = K.label_regions(t, connectivity, background, by_value, dims=dims)
    sizes, offsets = K.region_sizes(labels, counts, dims=dims)
    sizes = sizes.cpu().numpy()
    assert sizes.dtype == np.int32
    return [sizes[a:b].astype(np.int64) for a, b in zip(offsets[:-1], offsets[1:])]


def device_sieve(K, stack, min_size, connectivity=4, background=0, by_value=False, fill=None, layout='planar',
                 strided=False):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    t, dims, back = _upload(torch, dev, stack, layout)
    out, check = _output(torch, t, t.dtype, strided)
    got = K.sieve_regions(t, min_size, connectivity, background, by_value, fill, dims=dims, out=out)
    assert got is out
    check()
    return _download(out, back, stack.shape)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view('u%d' % a.dtype.itemsize)


def assert_same(got, want):
    """the same shape, type and bits everywhere (NaN payloads and the sign of zero included)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    same = bits(got) == bits(want)
    assert same.all(), '%d of %d elements differ, first at %s' % ((~same).sum(), same.size,
                                                                  tuple(np.argwhere(~same)[0]))


def want_label(stack, connectivity=4, background=0, by_value=False):
    """the restatement per plane -> (labels (k, ny, nx) int32, counts (k,) int64)"""
    res = ref.planes(ref.label, stack, connectivity, background, by_value)
    labels = np.stack([r[0] for r in res]) if len(res) else np.zeros(stack.shape, np.int32)
    return labels.astype(np.int32), np.array([r[1] for r in res], np.int64)


def check_label(K, stack, connectivity=4, background=0, by_value=False, area=False, **kw):
    lab, counts, ar = device_label(K, stack, connectivity, background, by_value, area=area, **kw)
    wl, wc = want_label(stack, connectivity, background, by_value)
    assert np.array_equal(counts, wc), (counts, wc)
    assert_same(lab, wl)
    if area:
        assert_same(ar, np.stack([ref.area(l, n) for l, n in zip(wl, wc)]))
    return lab, counts


def check_sieve(K, stack, min_size, connectivity=4, background=0, by_value=False, fill=None, **kw):
    got = device_sieve(K, stack, min_size, connectivity, background, by_value, fill, **kw)
    want = np.stack(ref.planes(ref.sieve, stack, min_size, connectivity, background, by_value, fill))
    assert_same(got, want)
    return got


# ---- the random cases of the fuzz test ---------------------------------------------------------------------------
def random_case(rng):
    ny, nx = (int(v) for v in rng.integers(1, 151, size=2))
    k = int(rng.integers(1, 7))
    dtype = str(rng.choice(DTYPES))
    by_value = bool(rng.random() < 0.5)
    density = float(rng.choice(DENSITIES + (0.5, 1.0)))
    if by_value and dtype != 'bool':
        stack = np.stack([class_map(rng, (ny, nx), int(rng.integers(2, 6)), dtype) for _ in range(k)])
        background = [0, 3, 7][int(rng.integers(3))]
    else:
        stack = np.stack([mask(rng, (ny, nx), density) for _ in range(k)])
        background = 0
        if dtype != 'bool':
            background = int(rng.choice([0, 1, 3]))
            stack = stack * 2 + 1                   # values 1 and 3
        stack = stack.astype(dtype)
        if np.dtype(dtype).kind == 'f' and rng.random() < 0.5:
            stack[rng.random(stack.shape) < 0.1] = np.nan
    entry = str(rng.choice(['label', 'label_area', 'sizes', 'sieve']))
    case = {'entry': entry, 'connectivity': int(rng.choice([4, 8])), 'by_value': by_value, 'background': background,
            'layout': str(rng.choice(LAYOUTS)), 'strided': bool(rng.random() < 0.4), 'stack': stack}
    if entry == 'sieve':
        case['min_size'] = int(rng.choice([0, 1, 2, 3, 5, 20, 10 ** 6]))
        case['fill'] = None if rng.random() < 0.5 or dtype == 'bool' else 2
    return case


def describe(case):
    return {key: val for key, val in case.items() if key != 'stack'} | {'shape': case['stack'].shape,
                                                                         'dtype': str(case['stack'].dtype)}


def run_case(K, case):
    """the device result and the restatement of a random case, as lists of arrays"""
    s, c, bg, bv = case['stack'], case['connectivity'], case['background'], case['by_value']
    wl, wc = want_label(s, c, bg, bv)
    if case['entry'] in ('label', 'label_area'):
        area = case['entry'] == 'label_area'
        lab, counts, ar = device_label(K, s, c, bg, bv, case['layout'], case['strided'], area)
        got, want = [lab, counts], [wl, wc]
        if area:
            got.append(ar)
            want.append(np.stack([ref.area(l, n) for l, n in zip(wl, wc)]))
        return got, want
    if case['entry'] == 'sizes':
        return device_sizes(K, s, c, bg, bv, case['layout']), [ref.sizes(l, n) for l, n in zip(wl, wc)]
    got = device_sieve(K, s, case['min_size'], c, bg, bv, case['fill'], case['layout'], case['strided'])
    return [got], [np.stack(ref.planes(ref.sieve, s, case['min_size'], c, bg, bv, case['fill']))]
