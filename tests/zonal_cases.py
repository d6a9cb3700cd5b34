"""What the zonal GPU tests share: label planes with zones of chosen sizes, the data a sum can go wrong on, the device
calls in each layout, the comparison with the restatement (tests/zonal_ref.py: bit for bit) and the random cases of
tests/test_zonal_fuzz_gpu.py."""
import numpy as np

from tests import regions_cases as rcases
from tests import zonal_ref as ref

LAYOUTS = rcases.LAYOUTS                        # 'planar', 'pixel', 'crop'
LABEL_DTYPES = rcases.DTYPES                    # bool, uint8, int32, int64, float32, float64
ALL = ('count', 'nan_count', 'sum', 'min', 'max', 'm2', 'mean')
# one below, at and one above every group size of the tree: the 8-lane group, the chunk, the segment, two segments
ZONE_SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097, 8193)


def sized_zones(rng, shape, sizes, dtype='int32', scattered=True):
    """a label plane whose zone z + 1 has sizes[z] pixels, scattered over the plane (or in raster runs), 0 elsewhere"""
    npix = shape[0] * shape[1]
    assert sum(sizes) <= npix, (sum(sizes), npix)
    order = rng.permutation(npix) if scattered else np.arange(npix)
    lab = np.zeros(npix, np.int64)
    at = 0
    for z, m in enumerate(sizes):
        lab[order[at:at + m]] = z + 1
        at += m
    return lab.reshape(shape).astype(dtype)


def speckle(rng, shape, dtype='float32', nan=0.01):
    """gamma speckle of 4 looks with a share of NaN"""
    x = rng.gamma(4.0, 0.25, size=shape).astype(dtype)
    if nan:
        x[rng.random(shape) < nan] = np.nan
    return x


def blobs(rng, shape, density=0.59):
    """a labelling like label_regions': the 4-connected regions of a random mask, numbered in raster order"""
    from tests import regions_ref
    return regions_ref.label((rng.random(shape) < density).astype(np.uint8), 4)[0]


# ---- the device calls ----------------------------------------------------------------------------------------------
def _device():
    import torch
    return torch, torch.device('cuda', torch.cuda.current_device())


def upload_labels(labels, strided=False):
    """a label plane on the device: packed, or every second element of every second row of a larger buffer"""
    torch, dev = _device()
    labels = np.asarray(labels)
    if not strided:
        return torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    big = np.full((2 * labels.shape[0] + 1, 2 * labels.shape[1] + 3), 1, labels.dtype)
    big[1::2, 1:1 + 2 * labels.shape[1]:2] = labels
    return torch.from_numpy(big).to(dev)[1::2, 1:1 + 2 * labels.shape[1]:2]


def device_index(K, labels, ids=None, strided=False):
    return K.zonal_index(upload_labels(labels, strided), ids)


def device_stats(K, stack, index, layout='planar', stats=ALL):
    """stack numpy (k, ny, nx) through kernels.zonal_stats -> a dict of numpy (k, n)"""
    torch, dev = _device()
    t, dims, _ = rcases._upload(torch, dev, np.asarray(stack), layout)
    got = K.zonal_stats(t, index, dims=dims, stats=stats)
    return {s: v.cpu().numpy() for s, v in got.items()}


def want_stats(stack, labels, ids=None):
    st, ids = ref.zonal_stats(np.asarray(stack), np.asarray(labels), ids)
    st['mean'] = ref.mean(st)
    return st


def check_index(index, labels, ids=None):
    k, n, wids = ref.keys(labels, ids)
    perm, offsets = ref.index(k, n)
    assert index.n == n and np.array_equal(index.ids, wids)
    rcases.assert_same(index.keys.cpu().numpy(), k)
    rcases.assert_same(index.perm.cpu().numpy(), perm)
    rcases.assert_same(index.offsets.cpu().numpy(), offsets)


def check_stats(K, stack, labels, ids=None, layout='planar', strided=False, stats=ALL):
    index = device_index(K, labels, ids, strided)
    check_index(index, labels, ids)
    got = device_stats(K, stack, index, layout, stats)
    want = want_stats(stack, labels, ids)
    assert set(got) == set(stats)
    ref.same_stats(got, {s: want[s] for s in stats})
    return got, index


def device_paint(K, table, index, stack, layout='planar', strided=False, keep=False, fill=None):
    """table numpy (k, n) painted over the planes of `stack` (k, ny, nx: the type, and the values kept) -> (k, ny, nx)"""
    torch, dev = _device()
    t, dims, back = rcases._upload(torch, dev, np.asarray(stack), layout)
    out, check = rcases._output(torch, t, t.dtype, strided)
    tab = torch.from_numpy(np.ascontiguousarray(table, np.float64)).to(dev)
    got = K.zonal_paint(tab, index, like=t, out=out, keep=keep, fill=fill, dims=dims)
    assert got is out
    check()
    return rcases._download(out, back, np.asarray(stack).shape)


def check_paint(K, table, index, labels, stack, ids=None, **kw):
    got = device_paint(K, table, index, stack, **kw)
    k = ref.keys(labels, ids)[0]
    fill = kw.get('fill')
    want = ref.paint(table, k, np.asarray(stack).dtype, np.asarray(stack) if kw.get('keep') else None,
                     np.nan if fill is None else fill)
    ref.same(got, want)
    return got


# ---- the random cases of the fuzz test -----------------------------------------------------------------------------
def random_case(rng):
    ny, nx = (int(v) for v in rng.integers(1, 151, size=2))
    k = int(rng.integers(1, 7))
    kind = str(rng.choice(['classes', 'blobs', 'sparse']))
    ldtype = str(rng.choice(LABEL_DTYPES))
    ids = None
    if kind == 'classes':
        labels = rcases.class_map(rng, (ny, nx), int(rng.integers(2, 6)), ldtype if ldtype != 'bool' else 'uint8')
        if ldtype == 'bool':
            labels = labels != 0
        if np.dtype(ldtype) == np.int64:                # its labels pass 2^53: no 1 .. n
            ids = [-5, 7, 2 ** 53, 2 ** 53 + 1]
        elif rng.random() < 0.3:
            ids = [1, 3, 7]
    elif kind == 'blobs':
        labels = blobs(rng, (ny, nx), float(rng.choice([0.3, 0.59, 0.9])))
        ldtype = str(rng.choice(['int32', 'int64', 'float32', 'float64']))
        labels = labels.astype(ldtype)
    else:
        pool = np.unique(np.concatenate([rng.integers(-50, 5000, size=20), [3, 100234, 2 ** 40 + 1]]))
        ids = [int(v) for v in np.sort(rng.choice(pool, size=int(rng.integers(1, 12)), replace=False))]
        ldtype = 'int64'
        labels = rng.choice(pool, size=(ny, nx)).astype(np.int64)
    dtype = str(rng.choice(['float32', 'float64', 'int32']))
    if dtype == 'int32':
        stack = rng.integers(-1000, 1000, size=(k, ny, nx)).astype(np.int32)
    else:
        stack = speckle(rng, (k, ny, nx), dtype, float(rng.choice([0.0, 0.01, 0.3])))
        if rng.random() < 0.2:
            stack[rng.random(stack.shape) < 0.01] = np.inf
    return {'entry': str(rng.choice(['stats', 'paint_fill', 'paint_keep'])), 'labels': labels, 'ids': ids, 'stack': stack,
            'layout': str(rng.choice(LAYOUTS)), 'strided': bool(rng.random() < 0.4), 'kind': kind}


def describe(case):
    return {key: val for key, val in case.items() if key not in ('stack', 'labels')} | {
        'shape': case['stack'].shape, 'dtype': str(case['stack'].dtype), 'labels': str(case['labels'].dtype)}


def run_case(K, case):
    """runs the three kernel-level calls of a random case and compares with the restatement (AssertionError)"""
    labels, ids, stack = case['labels'], case['ids'], case['stack']
    got, index = check_stats(K, stack, labels, ids, case['layout'], case['strided'])
    if case['entry'] == 'stats':
        return
    if stack.dtype.kind != 'f':
        stack = stack.astype(np.float64)
    check_paint(K, got['mean'], index, labels, stack, ids, layout=case['layout'], strided=case['strided'],
                keep=case['entry'] == 'paint_keep', fill=None if case['entry'] == 'paint_keep' else -1.5)
