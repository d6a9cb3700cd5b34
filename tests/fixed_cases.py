"""Fixed cases, with references written inline, for the entries no seeded generator reaches: the three relayout
entries in every staging class of relayout.hip, split_complex / merge_complex, coregister_shifts, classify_gather,
class_stats, class_fill, feature_moments, gather_rows, rgb_limits, resample_check_table and region_sizes.

tests/test_canary_gpu.py runs them on poisoned, guard-banded memory, tests/test_streams_gpu.py on a held-back side
stream.  Every body takes `c`, the canary or the held_stream block it runs in: c.check() after each group of calls,
c.is_poison(t) where the contract leaves memory unwritten.  AssertionError is the verdict."""
import numpy as np
import pytest


def up(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- relayout ------------------------------------------------------------------------------------------------------
def pixels_per_block(row_elems, elem):
    """relayout_impl (nd_amd/csrc/relayout.hip): `int pb = 256; while (pb > 1 && pb * row_elems * sizeof(T) > 48 * 1024)
    pb >>= 1;` with row_elems = k | 1 for one plane stack and (2 k) | 1 for both halves of a complex source.  float32:
    256 pixels up to k = 47, 128 from 48, 64 from 96, 32 from 192, 16 from 384, 8 from 768, 4 from 1536, 2 from 3072,
    1 from 6144 to the wrappers' limit of (k | 1) * 4 <= 48 KiB, k = 12287; float64 and both halves: at half of each."""
    pb = 256
    while pb > 1 and pb * row_elems * elem > 48 * 1024:
        pb >>= 1
    return pb


def first_of_each_class(elem, both):
    """the shortest series of every staging class -> {pixels per block: k}"""
    out = {}
    k = 1
    while ((2 * k if both else k) | 1) * elem <= 48 * 1024:
        out.setdefault(pixels_per_block((2 * k if both else k) | 1, elem), k)
        k += 1
    return out


RELAYOUT_RASTER = (3, 67)           # 201 pixels: no multiple of any block's pixel count but 1


def relayout(K, device, dtype, c):
    """relayout_planar, relayout_planar_complex and relayout_pixel_major are copies: every destination element equals
    its source element bit for bit (numpy's moveaxis is the reference), for real sources and for the .real / .imag
    halves of a complex one.  Destination planes have a pitch of ny * nx + 5: the padding keeps the pattern.  A
    complex destination of relayout_pixel_major keeps the pattern in the half that was not written.  One series
    length per staging class (pixels_per_block), the first of each."""
    import torch
    ny, nx = RELAYOUT_RASTER
    npix, pitch = ny * nx, ny * nx + 5
    elem = np.dtype(dtype).itemsize
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    cdt = torch.complex64 if dtype == np.float32 else torch.complex128
    single, both = first_of_each_class(elem, False), first_of_each_class(elem, True)
    assert sorted(single) == sorted(both) == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert single == ({256: 1, 128: 48, 64: 96, 32: 192, 16: 384, 8: 768, 4: 1536, 2: 3072, 1: 6144} if elem == 4 else
                      {256: 1, 128: 24, 64: 48, 32: 96, 16: 192, 8: 384, 4: 768, 2: 1536, 1: 3072})
    rng = np.random.default_rng(5)

    def planes(k):
        """a poisoned (k, ny, nx) view of planes `pitch` apart, and the poisoned allocation behind it"""
        base = torch.empty((k, pitch), dtype=tdt, device=device)
        return base[:, :npix].view(k, ny, nx), base

    for pb in sorted(single):
        for k in {single[pb], max(1, single[pb] - 1) if pb < 256 else 47 if elem == 4 else 23}:
            re = rng.normal(size=(ny, nx, k)).astype(dtype)
            im = rng.normal(size=(ny, nx, k)).astype(dtype)
            z = torch.complex(up(re, device), up(im, device))
            assert z.dtype == cdt
            # (y, x, time) -> planar: a real source, then each half of the complex one
            for src, host in ((up(re, device), re), (z.real, re), (z.imag, im)):
                dst, base = planes(k)
                assert K.relayout_planar(src, dst)
                assert np.array_equal(dst.cpu().numpy(), np.moveaxis(host, -1, 0)), ('planar', k)
                assert bool(c.is_poison(base[:, npix:]).all()), ('planar: the padding was written', k)
            # planar -> (y, x, time): a real destination, then one half of a complex one
            src, base = planes(k)
            src.copy_(up(np.moveaxis(re, -1, 0), device))
            out = torch.empty((ny, nx, k), dtype=tdt, device=device)
            assert K.relayout_pixel_major(src, out)
            assert np.array_equal(out.cpu().numpy(), re), ('pixel-major', k)
            zo = torch.empty((ny, nx, k), dtype=cdt, device=device)
            assert K.relayout_pixel_major(src, zo.imag)
            assert np.array_equal(zo.imag.cpu().numpy(), re), ('pixel-major, .imag', k)
            assert bool(c.is_poison(zo.real).all()), ('pixel-major, .imag: the real half was written', k)
            c.check()
    for pb in sorted(both):
        k = both[pb]
        re = rng.normal(size=(ny, nx, k)).astype(dtype)
        im = rng.normal(size=(ny, nx, k)).astype(dtype)
        z = torch.complex(up(re, device), up(im, device))
        (dre, bre), (dim_, bim) = planes(k), planes(k)
        assert K.relayout_planar_complex(z.real, z.imag, dre, dim_)
        assert np.array_equal(dre.cpu().numpy(), np.moveaxis(re, -1, 0)), ('both halves, real', k)
        assert np.array_equal(dim_.cpu().numpy(), np.moveaxis(im, -1, 0)), ('both halves, imaginary', k)
        assert bool(c.is_poison(bre[:, npix:]).all()) and bool(c.is_poison(bim[:, npix:]).all()), k
        c.check()


# ---- split_complex / merge_complex ---------------------------------------------------------------------------------
def split_and_merge_complex(K, device, c):
    """split_complex and merge_complex move values unchanged: numpy's .real / .imag are the reference, bit for bit.
    Lengths around the four values a thread moves and the 1024 a block moves."""
    import torch
    rng = np.random.default_rng(6)
    for dtype in (np.float32, np.float64):
        cdt = torch.complex64 if dtype == np.float32 else torch.complex128
        for n in (1, 3, 4, 5, 1023, 1025):
            re, im = rng.normal(size=n).astype(dtype), rng.normal(size=n).astype(dtype)
            z = torch.complex(up(re, device), up(im, device))
            got = K.split_complex(z.real, z.imag)
            assert got is not None
            assert np.array_equal(got[0].cpu().numpy(), re) and np.array_equal(got[1].cpu().numpy(), im), (dtype, n)
            out = torch.empty(n, dtype=cdt, device=device)
            assert K.merge_complex(up(re, device), up(im, device), out)
            h = out.cpu().numpy()
            assert np.array_equal(h.real, re) and np.array_equal(h.imag, im), (dtype, n)
            c.check()


# ---- coregister_shifts ---------------------------------------------------------------------------------------------
def coregister_shifts(K, device, c):
    """One small stack per type of tests/coreg_cases.py (31 x 37, u = 7: prime sizes) against tests/coreg_ref.py by the
    near-tie rule of that module."""
    from tests import coreg_cases as cases
    ny, nx, u = cases.CASES[0]
    for dtype in (np.float32, np.float64):
        want, ok = cases.case_reference(ny, nx, u, dtype)
        sh, status = K.coregister_shifts(up(np.array(cases.c11_stack(ny, nx, u, dtype)), device), 0, u)   # a copy
        got, status = sh.cpu().numpy(), status.cpu().numpy()
        assert (status == 0).all() and (got[0] == 0).all()
        cases.check_shifts(got, want, ok, u, (ny, nx))
        c.check()


# ---- the classifier's helpers --------------------------------------------------------------------------------------
def feature_planes(rng, dtype, ny, nx, nfeat):
    """nfeat (ny, nx) planes of multiples of 1 / 256 below 16 in magnitude (float64 sums of a few thousand of them are
    exact in any order), 3 % NaN -> (X (rows, nfeat), the planes)"""
    planes = [(rng.integers(-4095, 4096, (ny, nx)) / 256.0).astype(dtype) for _ in range(nfeat)]
    for p in planes:
        p[rng.random((ny, nx)) < 0.03] = np.nan
    return np.stack([p.reshape(-1) for p in planes], axis=1), planes


def classify_gather_class_stats_class_fill(K, device, c):
    """classify_gather against classify_ref.make_Xy (the kept rows in row order, bit for bit; mask = kept),
    class_stats against per-class numpy sums -- exact: the values are multiples of 1 / 256, so a float64 sum of them
    is the same in any order -- and class_fill against its definition in kernels.py restated with numpy.where.
    37 x 67 = 2479 rows: several blocks, the last one partial."""
    from tests import classify_ref as ref
    rng = np.random.default_rng(7)
    ny, nx = 37, 67
    for dtype in (np.float32, np.float64):
        X, planes = feature_planes(rng, dtype, ny, nx, 3)
        feats = [up(p, device) for p in planes]
        labels = rng.integers(0, 4, (ny, nx)).astype(np.float64)
        labels[rng.random((ny, nx)) < 0.05] = np.nan
        lab = up(labels, device)
        # classify_gather, with and without labels
        for with_labels in (True, False):
            wX, wy, keep = ref.make_Xy(X, labels.reshape(-1) if with_labels else None)
            gX, gy, mask = K.classify_gather(feats, (ny, nx), (nx, 1), lab if with_labels else None,
                                             (nx, 1) if with_labels else None)
            assert np.array_equal(mask.cpu().numpy(), keep.astype(np.uint8))
            assert gX.cpu().numpy().tobytes() == np.ascontiguousarray(wX).tobytes() and gX.shape == wX.shape
            assert (gy is None) == (wy is None)
            if wy is not None:
                assert np.array_equal(gy.cpu().numpy(), wy)
        # class_stats: classes 0 .. 3, labels broadcast over a leading axis of 2 (label stride 0)
        var = np.stack([planes[0], planes[1]])
        lab2 = np.broadcast_to(labels, var.shape)
        s, n, nn = (t.cpu().numpy() for t in K.class_stats(up(var, device), lab, (0, nx, 1), 4))
        for l in range(4):
            v = var[lab2 == l].astype(np.float64)
            assert s[l] == v[~np.isnan(v)].sum() and n[l] == (~np.isnan(v)).sum() and nn[l] == np.isnan(v).sum(), l
        assert s.dtype == np.float64 and n.dtype == np.int64 and nn.dtype == np.int64
        # class_fill: fill[l] where the label is l in 0 .. 2, elsewhere var, or fill[-1] where that is NaN
        fill = np.array([10.5, 20.5, 30.5, -1.25], dtype)
        got = K.class_fill(up(var, device), lab, (0, nx, 1), up(fill, device)).cpu().numpy()
        want = np.where(np.isnan(var), fill[-1], var)
        for l in range(3):
            want = np.where(lab2 == l, fill[l], want)
        assert got.dtype == var.dtype and got.tobytes() == want.astype(dtype).tobytes()
        c.check()


def feature_moments_and_gather_rows(K, device, c):
    """feature_moments against kmeans_fit_ref.moments by the rule of check_moments (tests/test_kmeans_fit_gpu.py, as
    tools/fuzz_parity.py restates it): the count equal, mean and variance within rows * 2^-52 of the magnitudes
    behind them.  gather_rows against numpy indexing, bit for bit: NaN rows and valid = 0 for indices outside."""
    from tests import classify_ref as ref, kmeans_fit_ref as kf
    rng = np.random.default_rng(8)
    ny, nx = 29, 70
    for dtype in (np.float32, np.float64):
        X, planes = feature_planes(rng, dtype, ny, nx, 5)
        feats = [up(p, device) for p in planes]
        mean, scale = rng.normal(size=5), rng.uniform(0.5, 2.0, 5)
        for m, s in ((None, None), (mean, scale)):
            count, fmean, fvar = (t.cpu().numpy() for t in K.feature_moments(feats, (ny, nx), (nx, 1), m, s))
            n, wm, wv = kf.moments(X, m, s)
            V, valid = kf.values(X, m, s)
            mag = np.abs(V[valid]).sum(axis=0) / n
            bound = X.shape[0] * 2.0 ** -52
            assert int(count) == n
            assert np.all(np.abs(fmean - wm) <= bound * mag)
            assert np.all(np.abs(fvar - wv) <= bound * (wv + 2 * mag * np.sqrt(wv)) + (bound * mag) ** 2)
            idx = np.concatenate([rng.integers(0, ny * nx, 300), [-1, ny * nx, 0, ny * nx - 1]]).astype(np.int64)
            gX, gvalid = (t.cpu().numpy() for t in K.gather_rows(feats, (ny, nx), (nx, 1), up(idx, device), m, s))
            inside = (idx >= 0) & (idx < ny * nx)
            rows = X[np.where(inside, idx, 0)]
            want = rows if m is None else ref.scale(rows, m, s)
            want = np.where(inside[:, None], want, np.nan).astype(dtype)
            assert np.array_equal(gvalid, (inside & ~np.isnan(rows).any(axis=1)).astype(np.uint8))
            assert np.array_equal(np.isnan(gX), np.isnan(want))
            assert np.where(np.isnan(want), 0, gX).tobytes() == np.where(np.isnan(want), 0, want).tobytes()
        c.check()


# ---- rgb_limits ----------------------------------------------------------------------------------------------------
def rgb_limits(K, device, c):
    """rgb_limits on three channels, one of them a quotient, against rgb_ref.limits by the rule of
    tests/test_to_rgb_cpu.py (equal values of the data type, NaN where NaN); the counts equal."""
    from tests import rgb_ref
    from tests.test_to_rgb_cpu import same
    rng = np.random.default_rng(9)
    for dtype in (np.float32, np.float64):
        stacks = [rng.exponential(size=(3, 33, 71)).astype(dtype) for _ in range(4)]
        stacks[1][rng.random(stacks[1].shape) < 0.2] = np.nan
        stacks[2][1] = np.nan                                       # a whole plane without a value
        stacks[3][rng.random(stacks[3].shape) < 0.1] = 0
        dev = [up(a, device) for a in stacks]
        limits, counts = K.rgb_limits([dev[0], dev[1], (dev[2], dev[3])], 2, 98)
        with np.errstate(all='ignore'):
            chans = [stacks[0], stacks[1], stacks[2] / stacks[3]]
            want = np.array([[rgb_ref.limits(ch[t], 2, 98) for ch in chans] for t in range(3)], dtype=dtype)
            wn = np.array([[np.count_nonzero(~np.isnan(ch[t])) for ch in chans] for t in range(3)], np.int64)
        assert same(limits.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), wn)
        c.check()


# ---- resample_check_table ------------------------------------------------------------------------------------------
def resample_check_table(K, device, c):
    """resample_check_table accepts what resample_axis builds and refuses a run that leaves its axis"""
    from nd_amd import _lib
    for method in K.RESAMPLE_METHODS:
        K.resample_check_table(K.resample_axis(67, 131, (10.0, 500.0), (5.1, 497.0), method), device)
    bad = K.resample_axis(67, 131, (10.0, 500.0), (5.1, 497.0), 'bilinear')
    bad.start = bad.start.copy()
    two = int(np.argmax(bad.count == 2))
    assert bad.count[two] == 2
    bad.start[two] = 66                                             # two taps from the last sample on
    with pytest.raises(_lib.NdAmdError):
        K.resample_check_table(bad, device)


# ---- region_sizes --------------------------------------------------------------------------------------------------
def region_sizes_case():
    """the four planes of the region_sizes cases, the restatement's labels and counts, and its sizes per plane"""
    from tests import regions_cases as cases, regions_ref as ref
    rng = np.random.default_rng(11)
    stack = np.stack([cases.mask(rng, (70, 133), d) for d in (0.59, 0.0, 0.41, 1.0)])
    wl, wc = cases.want_label(stack, 8)
    return stack, wl, wc, [ref.sizes(l, n) for l, n in zip(wl, wc)]


def region_sizes_counted(K, device, case, c):
    """region_sizes on labels uploaded from the restatement: regions_ref.sizes is the reference"""
    stack, wl, wc, want = case
    sizes, offsets = K.region_sizes(up(wl, device), up(wc, device))
    sizes = sizes.cpu().numpy()
    for p, w in enumerate(want):
        assert np.array_equal(sizes[offsets[p]:offsets[p + 1]], w), p


def region_sizes_labelled(K, device, case, c):
    """label_regions on the device first, region_sizes of those labels, in every layout"""
    from tests import regions_cases as cases
    stack, wl, wc, want = case
    for layout in cases.LAYOUTS:
        got = cases.device_sizes(K, stack, 8, layout=layout)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), layout
