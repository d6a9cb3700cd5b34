"""Randomised parity campaign: the HIP path (through the C ABI) against the CPU oracle on random
shapes, strides, parameters and corner values.  Not part of the pytest suite (run time is open
ended); what it finds is either fixed with a regression case in tests/ or recorded in DESIGN.md 9.

    python tools/fuzz_parity.py --seconds 120 --seed 1 [--what omnibus,omnibus_long,omnibus_ml,c3,nlmeans,correlate,
        gaussian,omnibus_diag,change_segments,to_rgb,forest,kmeans_predict,knn,linear,kmeans_step,warp,c3_more]

The families up to `gaussian` run against the CPU oracle; the ones after it (NEWER), merged later, against the numpy
restatements under tests/, each as gen_<name> / want_<name> / compare_<name> (numpy only) around a device step.

Prints one line per failure (with the parameters needed to replay it) and a summary; exit code 1
if anything differed, 2 if a case raised (the campaign ends there)."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import torch
from nd_amd import kernels
from oracle import oracle as O

DEV = torch.device('cuda:0')
ILL_POSED = [0]     # NaN <-> number swaps of the ill-posed n_eff corner (nlmeans)


def wishart(rng, k, ny, nx, looks, dtype, pol=2):
    s = (rng.normal(size=(pol, looks, k, ny, nx)) + 1j * rng.normal(size=(pol, looks, k, ny, nx))) / np.sqrt(2)
    out = {}
    for i in range(pol):
        out['C%d%d' % (i + 1, i + 1)] = (np.abs(s[i]) ** 2).mean(axis=0)
        for j in range(i + 1, pol):
            c = (s[i] * np.conj(s[j])).mean(axis=0)
            out['C%d%dre' % (i + 1, j + 1)] = c.real
            out['C%d%dim' % (i + 1, j + 1)] = c.imag
    return {n: v.astype(dtype) for n, v in out.items()}


def case_omnibus(rng):
    k = int(rng.choice([2, 3, 5, 8, 9, 12, 16, 17, 24, 25, 31, 32, 33, 40, 48, 49, 60, 63, 64, 65, 80, 96, 97, 128, 130, 160, 192]))
    ny, nx = int(rng.integers(1, 40)), int(rng.integers(1, 300))
    looks = int(rng.choice([1, 2, 4, 9, 20]))
    dtype = rng.choice([np.float32, np.float64])
    alpha = float(rng.choice([0.01, 0.05, 0.2, 0.5, 0.7, 0.9, 0.99, 0.999, 0.9999, 1e-4]))
    n = int(rng.choice([looks, 1, 3]))
    w = wishart(rng, k, ny, nx, looks, dtype)
    planes = [w['C11'], w['C12re'], w['C12im'], w['C22']]
    # magnitudes: the fast forms take determinants inside 2^+-36 (float32) and hand the rest to the exact pass
    scale = float(rng.choice([1.0, 1.0, 1.0, 1e-3, 1e-6, 1e4, 1e6]))
    if scale != 1.0:
        planes = [(p * scale).astype(dtype) for p in planes]
    # step changes, zeros, NaNs, infinities, negative determinants
    if rng.random() < 0.7:
        m = rng.random((ny, nx)) < 0.3
        t0 = rng.integers(1, k, (ny, nx)) if k > 1 else np.zeros((ny, nx), int)
        g = np.where((np.arange(k)[:, None, None] >= t0[None]) & m[None], rng.choice([0.1, 4.0, 30.0]), 1.0)
        planes = [(p * g).astype(dtype) for p in planes]
    if rng.random() < 0.3:
        bad = rng.random((k, ny, nx)) < 0.01
        val = rng.choice([0.0, np.nan, np.inf, -1.0])
        planes[int(rng.integers(0, 4))][bad] = val
    desc = dict(k=k, ny=ny, nx=nx, looks=looks, dtype=np.dtype(dtype).name, alpha=alpha, n=n)
    return omnibus_parity(rng, planes, alpha, n, desc)


def omnibus_parity(rng, planes, alpha, n, desc):
    """The planar (time, y, x) stack `planes` through the HIP path in a random layout (also the pixel-major
    kernel), workspace and with or without the rasters, against the oracle."""
    k, ny, nx = planes[0].shape
    layout = rng.choice(['tyx', 'yxt', 'pad', 'pm', 'pmc'])
    desc.update(layout=str(layout))
    with np.errstate(all='ignore'):
        want, zw, pw = O.change_detection_planes([np.moveaxis(p, 0, -1) for p in planes], alpha, n, njobs=8, stats=True)
    if layout in ('tyx', 'pm', 'pmc'):
        dev = [torch.from_numpy(p).to(DEV) for p in planes]
        dims = ('time', 'y', 'x')
    elif layout == 'yxt':
        dev = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(p, 0, -1))).to(DEV) for p in planes]
        dims = ('y', 'x', 'time')
    else:
        big = torch.zeros((4, k, ny + 2, nx + 5), dtype=torch.from_numpy(planes[0]).dtype, device=DEV)
        for v in range(4):
            big[v, :, 1:ny + 1, 3:nx + 3] = torch.from_numpy(planes[v]).to(DEV)
        dev = [big[v, :, 1:ny + 1, 3:nx + 3] for v in range(4)]
        dims = ('time', 'y', 'x')
    stats = bool(rng.random() < 0.5)
    ws = str(rng.choice(['recommended', 'minimal']))
    desc.update(stats=stats, workspace=ws)
    res = None
    if layout in ('pm', 'pmc'):
        # the reference's own layout through the pixel-major kernel (C12 interleaved for 'pmc')
        dev = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(p, 0, -1))).to(DEV) for p in planes]
        dims = ('y', 'x', 'time')
        if layout == 'pmc':
            c12 = torch.complex(dev[1], dev[2])
            dev = [dev[0], c12.real, c12.imag, dev[3]]
        res = kernels.change_detection_pixel_major(*dev, alpha=alpha, n=n, stats=stats)
        if res is None and layout == 'pmc':
            dev = [d.contiguous() for d in dev]
    if res is None:
        res = kernels.change_detection(*dev, alpha=alpha, n=n, dims=dims, stats=stats, workspace=ws)
    got = (res[0] if stats else res).cpu().numpy()
    ok = np.array_equal(got, want)
    if ok and stats:
        z, P = res[1].cpu().numpy(), res[2].cpu().numpy()
        with np.errstate(all='ignore'):
            ok = (np.allclose(z, zw, rtol=1e-5, atol=0, equal_nan=True) and
                  np.allclose(P, pw, rtol=1e-5, atol=1e-7, equal_nan=True))
    return ok, desc


def case_omnibus_long(rng):
    """193 - 4096 dates (the per-pixel sweep of pass B, the per-j table in device memory, MODE 1's screen
    constants past 64 KB of LDS) on small rasters of tests.synth.long_series_stack: running products of the
    determinants kept in range, random step dates, planted subnormal / underflowing / overflowing pixels."""
    from tests import synth
    k = int(np.exp(rng.uniform(np.log(193), np.log(4097))))
    ny, nx = int(rng.integers(1, 5)), int(rng.integers(1, 33))
    if k > 2048:
        nx = min(nx, 16)
    dtype = rng.choice([np.float32, np.float64])
    alpha = float(rng.choice([1e-4, 0.01, 0.2, 0.5, 0.9, 0.99, 0.9999]))
    plant = bool(nx >= 2 * len(synth.PLANT) and rng.random() < 0.5)
    planes, _ = synth.long_series_stack(int(rng.integers(1 << 30)), k, ny, nx, dtype=dtype,
                                        change_frac=float(rng.uniform(0.2, 0.8)), plant=plant)
    # whole-stack scales: mild ones, and ones that move every determinant far enough for the products to leave
    # the double range within a few hundred dates
    scale = float(rng.choice([1.0, 1.0, 1.0, 0.9, 1.1, 1e-3, 1e3]))
    if scale != 1.0:
        planes = [(p * scale).astype(dtype) for p in planes]
    if rng.random() < 0.3:
        bad = rng.random((k, ny, nx)) < 0.002
        planes[int(rng.integers(0, 4))][bad] = rng.choice([0.0, np.nan, np.inf, -1.0])
    desc = dict(k=k, ny=ny, nx=nx, dtype=np.dtype(dtype).name, alpha=alpha, n=9, plant=plant, scale=scale)
    return omnibus_parity(rng, planes, alpha, 9, desc)


def case_omnibus_ml(rng):
    """OmnibusTest(ml=w): the fused multilooking kernel (nd_amd_omnibus_c2_ml) against scipy's boxcar
    followed by the oracle's test with n = ml ** 2 (nd/change.py:61-69)."""
    import scipy.ndimage as ndi
    ml = int(rng.choice([3, 5]))
    k = int(rng.choice([3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 20, 23, 24]))
    ny, nx = int(rng.integers(ml, 60)), int(rng.integers(ml, 400))
    if rng.random() < 0.3:
        nx = int(rng.choice([64, 128, 192, 256, 68, 132]))        # whole tiles, 16-byte rows
    looks = int(rng.choice([1, 1, 2, 4]))
    alpha = float(rng.choice([0.01, 0.2, 0.7, 0.9, 0.95, 0.99, 0.999, 1e-4]))
    w = wishart(rng, k, ny, nx, looks, np.float32)
    planes = [w['C11'], w['C12re'], w['C12im'], w['C22']]
    scale = float(rng.choice([1.0, 1.0, 1.0, 1e-3, 1e-6, 1e4]))
    if scale != 1.0:
        planes = [(p * np.float32(scale)).astype(np.float32) for p in planes]
    if rng.random() < 0.7:
        m = rng.random((ny, nx)) < 0.3
        t0 = rng.integers(1, k, (ny, nx))
        g = np.where((np.arange(k)[:, None, None] >= t0[None]) & m[None], rng.choice([0.1, 4.0, 30.0]), 1.0)
        planes = [(p * g).astype(np.float32) for p in planes]
    if rng.random() < 0.3:
        bad = rng.random((k, ny, nx)) < 0.005
        planes[int(rng.integers(0, 4))][bad] = rng.choice([0.0, np.nan, np.inf, -1.0])
    if rng.random() < 0.2:                                          # a nodata margin
        for p in planes:
            p[:, :, : nx // 3] = 0
    stats = bool(rng.random() < 0.4)
    layout = str(rng.choice(['tyx', 'pad']))
    desc = dict(ml=ml, k=k, ny=ny, nx=nx, looks=looks, alpha=alpha, stats=stats, layout=layout, scale=scale)
    kern = (np.ones((ml, ml), dtype=np.float64) / ml ** 2).reshape(1, ml, ml)
    with np.errstate(all='ignore'):
        mlp = [ndi.convolve(p, kern) for p in planes]
        want, zw, pw = O.change_detection_planes([np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in mlp],
                                                 alpha, ml * ml, njobs=8, stats=True)
    if layout == 'tyx':
        dev = [torch.from_numpy(p).to(DEV) for p in planes]
    else:
        big = torch.zeros((4, k, ny + 2, nx + 8), dtype=torch.float32, device=DEV)
        for v in range(4):
            big[v, :, 1:ny + 1, 4:nx + 4] = torch.from_numpy(planes[v]).to(DEV)
        dev = [big[v, :, 1:ny + 1, 4:nx + 4] for v in range(4)]
    res = kernels.change_detection_multilooked(*dev, alpha=alpha, ml=ml, stats=stats)
    if res is None:
        return False, dict(desc, refused=True)
    got = (res[0] if stats else res).cpu().numpy()
    ok = np.array_equal(got, want)
    if ok and stats:
        z, P = res[1].cpu().numpy(), res[2].cpu().numpy()
        with np.errstate(all='ignore'):
            ok = (np.allclose(z, zw, rtol=1e-5, atol=0, equal_nan=True) and
                  np.allclose(P, pw, rtol=1e-5, atol=1e-7, equal_nan=True))
    return ok, desc


def case_nlmeans(rng):
    layout = str(rng.choice(['A', 'B', 'C']))
    nv = int(rng.choice([1, 1, 2, 4, 5]))
    pm = int(rng.choice([0, 1]))
    dtype = np.float32 if rng.random() < 0.8 else np.float64
    if layout == 'A':            # (y, x, time, var) view of planar memory, 2-D window
        shape = (int(rng.integers(12, 80)), int(rng.integers(12, 200)), int(rng.integers(1, 4)), nv)
        r = (int(rng.integers(0, 6)), int(rng.integers(0, 6)), 0)
        f = (int(rng.integers(0, 3)),) * 2 + (0,) if rng.random() < 0.7 else (int(rng.integers(0, 3)), int(rng.integers(0, 3)), 0)
        perm = (3, 2, 0, 1)
    elif layout == 'B':          # (time, y, x, var) view of planar memory, 3-D window
        shape = (int(rng.integers(3, 8)), int(rng.integers(12, 60)), int(rng.integers(12, 200)), nv)
        r = (int(rng.integers(0, 3)), int(rng.integers(0, 5)), int(rng.integers(0, 5)))
        f = tuple(int(v) for v in rng.integers(0, 2, 3))
        if rng.random() < 0.35:  # three-date square windows: the streaming window kernel (patch_mode 0)
            R = int(rng.integers(1, 6))
            shape = (int(rng.integers(2, 9)), int(rng.integers(2 * R + 2, 70)), int(rng.integers(2 * R + 2, 300)), nv)
            r, f, pm = (1, R, R), (int(rng.integers(0, 2)), 1, int(rng.integers(1, 3))), 0
        perm = (3, 0, 1, 2)
    else:                        # C-contiguous (a, b, c, var): generic kernel
        shape = (int(rng.integers(3, 12)), int(rng.integers(5, 30)), int(rng.integers(5, 40)), nv)
        r = tuple(int(v) for v in rng.integers(0, 3, 3))
        f = tuple(int(v) for v in rng.integers(0, 2, 3))
        perm = None
    for d in range(3):           # keep a single reflection inside the array
        reach = r[d] + f[d]
        if reach > shape[d] - 1:
            r = tuple(0 if i == d else r[i] for i in range(3)); f = tuple(0 if i == d else f[i] for i in range(3))
    sigma, h = float(rng.choice([0.3, 0.5, 1.0, 2.0])), float(rng.choice([0.3, 0.5, 1.0, 2.0]))
    ne = float(rng.choice([-1, -1, 3.0, 10.0, 50.0, 1.0]))
    nq = (2 * r[0] + 1) * (2 * r[1] + 1) * (2 * r[2] + 1) - 1
    if ne == nq + 1:
        # ill-posed corner of find_weight (nd/_filters.pyx:296-315): with n_eff - 1 equal to the
        # number of neighbours, equal weights put the discriminant at exactly 0 +- rounding noise,
        # and whether the reference returns a number or NaN depends on the last ulp of libm's exp
        ne = float(nq + 2)
    a = rng.gamma(4.0, 0.25, shape).astype(dtype)
    if rng.random() < 0.3:
        a -= a.mean().astype(dtype)
    nodata = 'none'
    if rng.random() < 0.3:       # nodata: a NaN margin, isolated NaNs, infinities of either sign (inf - inf)
        nodata = str(rng.choice(['margin', 'points', 'inf', 'mixed']))
        if nodata in ('margin', 'mixed'):
            ax = int(rng.integers(0, 3))
            sl = [slice(None)] * 4
            sl[ax] = slice(0, max(1, shape[ax] // 4))
            a[tuple(sl)] = np.nan
        if nodata in ('points', 'mixed'):
            a[rng.random(shape) < 0.003] = np.nan
        if nodata in ('inf', 'mixed'):
            m = rng.random(shape) < 0.004
            a[m] = np.where(rng.random(int(m.sum())) < 0.7, np.inf, -np.inf).astype(dtype)
    desc = dict(layout=layout, shape=shape, r=r, f=f, sigma=sigma, h=h, n_eff=ne, patch_mode=pm, dtype=np.dtype(dtype).name,
                nodata=nodata)
    want = np.empty_like(a)
    with np.errstate(all='ignore'):
        O.pixelwise_nlmeans_3d(a, want, r, f, sigma, h, ne, neff_policy=0, njobs=8, patch_mode=pm)
    t = torch.from_numpy(a).to(DEV)
    if perm is not None:
        inv = [perm.index(i) for i in range(4)]
        t = t.permute(*perm).contiguous().permute(*inv)
    out = torch.empty_like(t)
    kernels.pixelwise_nlmeans_3d(t, out, r, f, sigma, h, ne, patch_mode=pm, neff_policy=0)
    got = out.cpu().numpy()
    uniform = pm == 0 and max(f) > 0
    if uniform or dtype == np.float64 and False:
        ok = np.array_equal(got, want, equal_nan=True)
    else:
        fin = a[np.isfinite(a)]
        scale = float(np.abs(fin).max()) if fin.size else 1.0
        with np.errstate(all='ignore'):
            close = np.isclose(got, want, rtol=1e-5, atol=2e-6 * scale, equal_nan=True)
        ok = bool(close.all())
        if not ok and ne >= 0 and nodata != 'none':
            # Infinite data give weights of exactly 0, so the number of neighbours that carry weight
            # can equal n_eff - 1 anywhere (the generator only avoids that for the whole window), e.g.
            # a sample and its own reflection at the raster's edge: W^2 / W2 = n_eff - 1 +- rounding
            # noise decides between find_weight's error branch and a number.  The pixels where the
            # ORACLE ITSELF changes when n_eff moves by 1e-9 are that corner, not comparable.
            lo, hi = np.empty_like(a), np.empty_like(a)
            with np.errstate(all='ignore'):
                O.pixelwise_nlmeans_3d(a, lo, r, f, sigma, h, ne * (1 - 1e-9), neff_policy=0, njobs=8, patch_mode=pm)
                O.pixelwise_nlmeans_3d(a, hi, r, f, sigma, h, ne * (1 + 1e-9), neff_policy=0, njobs=8, patch_mode=pm)
                unstable = ~np.isclose(lo, hi, rtol=1e-6, atol=2e-7 * scale, equal_nan=True)
            if (close | unstable).all() and unstable.sum() <= max(16, got.size // 5):
                ILL_POSED[0] += int((unstable & ~close).sum())
                ok = True
        if not ok and ne >= 0:
            # find_weight's discriminant n tw^2 - n (n - 1) tsq is exactly 0 +- rounding noise when
            # n_eff - 1 neighbours share all the weight (e.g. a sample and its own reflection at the
            # raster's edge): NaN or a number, decided by the last ulp of libm's exp in the
            # reference itself.  Such NaN <-> number swaps are counted, not failed.
            swaps = np.isnan(got) != np.isnan(want)
            if (close | swaps).all() and swaps.sum() <= max(4, got.size // 200):
                ILL_POSED[0] += int(swaps.sum())
                ok = True
    return ok, desc


def case_correlate(rng):
    nd = int(rng.choice([2, 3]))
    dtype = np.float32 if rng.random() < 0.7 else np.float64
    shape = tuple(int(v) for v in (rng.integers(1, 6, nd - 2).tolist() + [rng.integers(1, 70), rng.integers(1, 300)]))
    ksh = tuple(int(v) for v in ([1] * (nd - 2) if rng.random() < 0.7 else rng.integers(1, 4, nd - 2).tolist()) +
                rng.integers(1, 8, 2).tolist())
    kind = str(rng.choice(['box', 'rand', 'sparse']))
    origin = 0
    if rng.random() < 0.35:      # square 3 / 5 / 7 windows on float32 planes: the register-window kernel
        w = int(rng.choice([3, 5, 7]))
        dtype = np.float32
        shape = shape[:-2] + (int(rng.integers(1, 90)), int(rng.integers(8, 900)))
        ksh = (1,) * (nd - 2) + (w, w)
        kind = str(rng.choice(['box', 'rand']))
        if rng.random() < 0.3:
            origin = (0,) * (nd - 2) + (int(rng.integers(-(w // 2), w // 2 + 1)), 0)
    if kind == 'box':
        kern = np.ones(ksh) / np.prod(ksh)
    else:
        kern = rng.normal(size=ksh)
        if kind == 'sparse':
            kern[rng.random(ksh) < 0.4] = 0.0
            if not kern.any():
                kern.flat[0] = 1.0
    mode = str(rng.choice(['reflect', 'constant', 'nearest', 'mirror', 'wrap']))
    cval = float(rng.choice([0.0, 1.5]))
    a = rng.normal(size=shape).astype(dtype)
    desc = dict(shape=shape, kernel=ksh, kind=kind, mode=mode, cval=cval, origin=origin, dtype=np.dtype(dtype).name)
    want = O.convolve(a, kern, mode=mode, cval=cval, origin=origin)
    t = torch.from_numpy(a).to(DEV)
    if rng.random() < 0.3 and nd == 3:          # (y, x, time)-style memory: window axes are not the fastest
        t = t.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        desc['strided'] = True
    got = kernels.convolve(t, kern, mode=mode, cval=cval, origin=origin).cpu().numpy()
    return np.array_equal(got, want, equal_nan=True), desc


def case_gaussian(rng):
    import scipy.ndimage as snf
    nd = int(rng.choice([2, 3]))
    dtype = np.float32 if rng.random() < 0.6 else np.float64
    shape = tuple(int(v) for v in rng.integers(1, 60, nd))
    sigma = tuple(float(v) for v in rng.choice([0.0, 0.5, 1.0, 2.5, 7.0], nd))
    mode = str(rng.choice(['reflect', 'constant', 'nearest', 'mirror', 'wrap']))
    fused = rng.random() < 0.45  # (y, x) passes of one radius on float32 planes: the fused kernel
    if fused:
        dtype = np.float32
        sg = float(rng.choice([0.3, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0]))
        shape = (int(rng.integers(1, 4)), int(rng.integers(1, 90)), int(rng.integers(8, 800)))
        sigma = (0.0, sg, sg if rng.random() < 0.8 else sg * 1.05)
        mode = str(rng.choice(['reflect', 'nearest', 'mirror', 'wrap']))
    a = rng.normal(size=shape).astype(dtype)
    if fused and rng.random() < 0.3:
        a[rng.random(shape) < 0.002] = rng.choice([np.inf, -np.inf, np.nan, 0.0])
    desc = dict(shape=shape, sigma=sigma, mode=mode, dtype=np.dtype(dtype).name)
    with np.errstate(all='ignore'):
        want = snf.gaussian_filter(a, sigma=sigma, mode=mode)
    got = kernels.gaussian_filter(torch.from_numpy(a).to(DEV), sigma, mode=mode).cpu().numpy()
    return np.array_equal(got, want, equal_nan=True), desc


# ---------------------------------------------------------------------------
# The families merged after round 6.  Each is three numpy-only functions -- gen_<name>(rng) -> (inputs, desc),
# want_<name>(inputs), which calls the restatement under tests/, and compare_<name>(got, want, inputs) -> bool --
# and a device step run_<name>(inputs) -> got that draws nothing: tests/test_fuzz_cases_cpu.py runs gen, want
# and compare over the seeds of the GPU test without a GPU.  got / want are dicts of numpy arrays.
# ---------------------------------------------------------------------------
LAST = {}                    # name / got / want of the newest case, for tools/fuzz_replay.py
EDGES = (1, 63, 64, 65, 255, 256, 257)
SCALES = (1.0, 1e-6, 1e-3, 1e4, 1e6)
CORNERS = (0.0, np.nan, np.inf, -np.inf, -1.0)
STACK_LAYOUTS = ('tyx', 'yxt', 'pad', 'off')


def draw_extent(rng, hi):
    """1 .. hi, half of the draws on the wave and block edges"""
    if rng.random() < 0.5:
        return int(rng.choice([n for n in EDGES if n <= hi]))
    return int(rng.integers(1, hi + 1))


def draw_raster(rng, max_pixels):
    nx = draw_extent(rng, max(1, min(300, max_pixels)))
    return int(rng.integers(1, max(1, min(8, max_pixels // nx)) + 1)), nx


def plant_corners(rng, arrays, values=CORNERS, share=0.3):
    """in `share` of the cases 1 % of the samples of one array, or of all, become one corner value"""
    if rng.random() >= share:
        return 'none'
    val = float(rng.choice(values))
    which = range(len(arrays)) if rng.random() < 0.5 else [int(rng.integers(0, len(arrays)))]
    for i in which:
        arrays[i][rng.random(arrays[i].shape) < 0.01] = val
    return repr(val)


def same_bits(got, want):
    """same type and shape, NaN where `want` has NaN, elsewhere the same bits"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.where(nan, 0, got).tobytes() == np.where(nan, 0, want).tobytes())


def device_planes(planes, layout, single=False):
    """the (time, y, x) numpy planes on the device: 'tyx' and 'yxt' (time fastest) as separate allocations or as
    one, 'pad' a view of a larger allocation, 'off' every base pointer one element off the 16-byte grid
    -> (views, dims, back), back(a) turning an output shaped like a view into (time, y, x) again"""
    k, ny, nx = planes[0].shape
    n = len(planes)
    tyx, same = ('time', 'y', 'x'), lambda a: a
    if layout == 'tyx':
        one = [torch.from_numpy(p).to(DEV) for p in planes]
        return (list(torch.stack(one)) if single else one), tyx, same
    if layout == 'yxt':
        one = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(p, 0, -1))).to(DEV) for p in planes]
        return (list(torch.stack(one)) if single else one), ('y', 'x', 'time'), lambda a: np.moveaxis(a, -1, 0)
    dt = torch.from_numpy(planes[0]).dtype
    if layout == 'pad':
        big = torch.zeros((n, k, ny + 2, nx + 5), dtype=dt, device=DEV)
        views = [big[v, :, 1:ny + 1, 3:nx + 3] for v in range(n)]
    else:
        step = k * ny * nx + (-(k * ny * nx)) % 4 + 4          # a multiple of 16 bytes in either type
        flat = torch.zeros(n * step + 1, dtype=dt, device=DEV)
        views = [flat[v * step + 1:][:k * ny * nx].view(k, ny, nx) for v in range(n)]
        assert all(v.data_ptr() % 16 == v.element_size() for v in views)
    for v, p in zip(views, planes):
        v.copy_(torch.from_numpy(p).to(DEV))
    return views, tyx, same


def host(t):
    return None if t is None else t.cpu().numpy()


# ---- omnibus_diag: kernels.change_detection_diag against tests/omnibus_diag_ref.py -------------------------
DIAG_ALPHAS = (1e-4, 0.01, 0.2, 0.5, 0.74, 0.75, 0.76, 0.9, 0.99, 0.9999)
DIAG_WORK = 250000            # pixels * dates^2 of one case: the restatement stays well under a second


def gen_omnibus_diag(rng):
    from tests import omnibus_diag_cases as C
    q = int(rng.integers(1, 4))
    dtype = str(rng.choice(['float32', 'float64']))
    if rng.random() < 0.6:
        k = C.FUSED_MAX_K[(q, dtype)] + int(rng.integers(-1, 2))
    else:
        k = int(rng.choice([1, 2, 3, 5, 10, 33, 64, 65, 97, 130, 200]))
    n = float(rng.choice([1, 2.5, 4.4, 9]))
    alpha = float(rng.choice(DIAG_ALPHAS))
    ny, nx = draw_raster(rng, max(1, min(2000, DIAG_WORK // (k * k))))
    planes = C.gamma_stack(int(rng.integers(1 << 30)), q, k, ny, nx, n, dtype)
    scale = float(rng.choice(SCALES))
    if scale != 1.0:
        planes = [(p * scale).astype(dtype) for p in planes]
    corner = plant_corners(rng, planes)
    stats = bool(rng.random() < 0.5)
    layout = str(rng.choice(STACK_LAYOUTS))
    desc = dict(q=q, dtype=dtype, k=k, ny=ny, nx=nx, n=n, alpha=alpha, scale=scale, corner=corner, stats=stats,
                layout=layout)
    return dict(planes=planes, q=q, dtype=dtype, n=n, alpha=alpha, stats=stats, layout=layout), desc


def want_omnibus_diag(inp):
    from tests import omnibus_diag_ref as R
    structure = (1,) * inp['q']
    with np.errstate(all='ignore'):
        S = R.Series(inp['planes'], structure, inp['n'])
        m, z, P = R.change_detection(inp['planes'], structure, inp['alpha'], inp['n'], series=S)
    return dict(map=m, z=z, P=P, closest=np.float64(S.closest))


def run_omnibus_diag(inp):
    views, dims, _ = device_planes(inp['planes'], inp['layout'])
    res = kernels.change_detection_diag(views, alpha=inp['alpha'], n=inp['n'], dims=dims, stats=inp['stats'])
    if inp['stats']:
        return dict(map=host(res[0]), z=host(res[1]), P=host(res[2]))
    return dict(map=host(res))


def compare_omnibus_diag(got, want, inp):
    """tests/omnibus_diag_cases.py: compare, unchanged, with the series' closest decision"""
    from tests import omnibus_diag_cases as C
    if got['map'].shape != want['map'].shape or got['map'].dtype != np.uint8:
        return False
    try:
        with np.errstate(all='ignore'):
            C.compare(got['map'], got.get('z'), got.get('P'), want['map'], want['z'], want['P'],
                      float(want['closest']), inp['alpha'], inp['dtype'])
    except AssertionError:
        return False
    return True


# ---- change_segments: kernels.change_segments against tests/change_segments_ref.py ---------------------------
def gen_change_segments(rng):
    from tests import change_segments_cases as cases
    structure, nplanes = cases.STRUCTURES[int(rng.integers(0, len(cases.STRUCTURES)))]
    dtype = str(rng.choice(['float32', 'float64']))
    k = 1000 if rng.random() < 0.02 else int(rng.choice([1, 2, 3, 10, 25, 33, 63, 64, 65, 130, 200]))
    ny, nx = draw_raster(rng, max(1, min(2000, 40000 // k)))
    planes, _ = cases.make(structure, nplanes, np.dtype(dtype), k, ny, nx, int(rng.integers(1 << 30)))
    p = float(rng.choice([0, 0.02, 0.25, 0.9, 1]))
    change = np.where(rng.random((ny, nx, k)) < p, rng.choice([1, 2, 255], (ny, nx, k)), 0).astype(np.uint8)
    first = bool(rng.random() < 0.5)
    change[..., 0] = 1 if first else 0
    scale = float(rng.choice(SCALES))
    if scale != 1.0:
        planes = [(a * scale).astype(dtype) for a in planes]
    corner = plant_corners(rng, planes)
    outputs = str(rng.choice(['both', 'direction', 'means']))
    layout, single = str(rng.choice(STACK_LAYOUTS)), bool(rng.random() < 0.5)
    desc = dict(structure=structure, planes=nplanes, dtype=dtype, k=k, ny=ny, nx=nx, p=p, first=first, scale=scale,
                corner=corner, outputs=outputs, layout=layout, single=single)
    return dict(planes=planes, change=change, structure=structure, outputs=outputs, layout=layout,
                single=single), desc


def want_change_segments(inp):
    from tests import change_segments_ref as R
    d, m = R.change_segments(inp['planes'], inp['change'], inp['structure'])
    return dict(direction=d, **{'mean%d' % i: a for i, a in enumerate(m)})


def run_change_segments(inp):
    views, dims, back = device_planes(inp['planes'], inp['layout'], inp['single'])
    direction, means = inp['outputs'] != 'means', inp['outputs'] != 'direction'
    res = kernels.change_segments(views, torch.from_numpy(inp['change']).to(DEV), inp['structure'], dims=dims,
                                  direction=direction, means=means)
    d, m = res if (direction and means) else ((res, None) if direction else (None, res))
    got = {}
    if d is not None:
        got['direction'] = host(d)
    if m is not None:
        got.update({'mean%d' % i: np.ascontiguousarray(back(host(a))) for i, a in enumerate(m)})
    return got


def compare_change_segments(got, want, inp):
    """direction equal everywhere, means bit for bit with equal NaN positions (assert_bit_equal): whatever was
    asked for must be there"""
    from tests.change_segments_cases import assert_bit_equal
    asked = [key for key in want if inp['outputs'] == 'both' or (key == 'direction') == (inp['outputs'] == 'direction')]
    try:
        for key in asked:
            if key == 'direction':
                assert got[key].dtype == np.int8
                np.testing.assert_array_equal(got[key], want[key])
            else:
                assert_bit_equal(got[key], want[key], key)
    except (AssertionError, KeyError):
        return False
    return True


# ---- the classifiers' feature table: views into one buffer, any sizes / strides of up to four dimensions -----
FEATURE_FORMS = ((1, 2, 3, 4), (5, 7, 8), (9, 12, 16, 33))      # registers for <= 4, for <= 8, memory reads beyond
ROW_LAYOUTS = ('contiguous', 'padded', 'permuted', 'zero', 'interleaved')
CLASS_COUNTS = (1, 2, 3, 4, 5, 8, 9, 11, 17)


def draw_features(rng, rare=(128, 200)):
    """a feature form, then a count inside it; rarely k-NN's limit or more than any form holds"""
    if rng.random() < 0.04:
        return int(rng.choice(rare))
    return int(rng.choice(FEATURE_FORMS[int(rng.integers(0, 3))]))


def gen_rows(rng, nfeat, dtype, max_rows=3000, integers=False, corners=(0.0, -1.0)):
    """-> dict(buf, offsets, sizes, strides, X, ...): feature f's row (i0, ..) is buf[offsets[f] + i . strides],
    X the (rows, nfeat) matrix numpy reads through exactly that rule.  A stride-0 dimension is a broadcast."""
    nd = int(rng.integers(1, 5))
    main = int(rng.integers(0, nd))
    sizes = [1] * nd
    if rng.random() < 0.45:                      # a row count on a wave or block edge: the other dimensions have size 1
        sizes[main] = int(rng.choice([n for n in (1, 63, 65, 255, 256, 257) if n <= max_rows]))
    else:
        sizes[main] = int(rng.integers(1, max(1, min(300, max_rows)) + 1))
        for d in range(nd):
            n = int(rng.choice([1, 1, 2, 3, 5]))
            if d != main and int(np.prod(sizes)) * n <= max_rows:
                sizes[d] = n
    layout = str(rng.choice(ROW_LAYOUTS))
    order = [int(i) for i in rng.permutation(nd)] if layout == 'permuted' else list(range(nd))   # slowest first
    ext = [n + int(rng.integers(0, 4)) for n in sizes] if layout == 'padded' else list(sizes)
    zero = -1
    if layout == 'zero':
        wide = [d for d in range(nd) if sizes[d] > 1]
        zero = int(rng.choice(wide)) if wide else int(rng.integers(0, nd))
        ext[zero] = 1
    strides, step = [0] * nd, 1
    for d in reversed(order):
        strides[d] = 0 if d == zero else step
        step *= ext[d]
    base = int(rng.integers(0, 4))                                       # 1 .. 3: off the 16-byte grid
    if layout == 'interleaved':                                          # the features are the fastest axis
        strides = [s * nfeat for s in strides]
        offsets, total = base + np.arange(nfeat), base + step * nfeat
    else:
        pitch = step + int(rng.integers(0, 3))
        offsets, total = base + rng.permutation(nfeat) * pitch, base + nfeat * pitch
    if integers:
        buf = rng.integers(0, 6, total).astype(np.float64)
    else:
        buf = rng.gamma(4.0, 0.5, total) * 2
    scale = float(rng.choice(SCALES))
    buf = (buf * scale).astype(dtype)
    u, corner = rng.random(), 'none'
    if u < 1 / 3:
        corner = 'nan'
        buf[rng.random(total) < (0.01 if nfeat < 64 else 0.001)] = np.nan
    elif u < 0.5:
        corner = repr(float(rng.choice(corners)))
        buf[rng.random(total) < 0.01] = float(corner)
    rowoff = np.zeros(sizes, np.int64)
    for d, idx in enumerate(np.indices(sizes)):
        rowoff += idx * strides[d]
    rowoff = rowoff.reshape(-1)
    assert rowoff.min() >= 0 and offsets.min() >= 0 and int(rowoff.max()) + int(offsets.max()) < total     # in bounds
    table = dict(buf=buf, offsets=[int(o) for o in offsets], sizes=sizes, strides=[int(s) for s in strides],
                 rowoff=rowoff)
    table['X'] = read_rows(table)
    X = table['X']
    desc = dict(features=nfeat, dtype=np.dtype(dtype).name, sizes=sizes, strides=table['strides'], rows=X.shape[0],
                layout=layout, base=base, scale=scale, corner=corner)
    return table, desc


def read_rows(table):
    return table['buf'][np.asarray(table['offsets'])[None, :] + table['rowoff'][:, None]]


def draw_scaler(rng, X):
    """in half of the cases mean_ / scale_ of the finite values (scale_ 1 for a constant feature)"""
    if rng.random() < 0.5:
        return None, None
    with np.errstate(all='ignore'):
        fin = np.where(np.isfinite(X), X, 0).astype(np.float64)
        mean, scale = fin.mean(axis=0), fin.std(axis=0)
    scale[~(scale > 0) | ~np.isfinite(scale)] = 1.0
    return mean, scale


def model_rows(inp):
    """-> (keep, the kept rows as the model sees them: scaled where the case has a scaler)"""
    from tests import classify_ref as ref
    X = inp['X']
    keep = ~np.isnan(X).any(axis=1)
    with np.errstate(all='ignore'):
        return keep, (X[keep] if inp['mean'] is None else ref.scale(X[keep], inp['mean'], inp['scale']))


def device_table(inp):
    t = torch.from_numpy(inp['buf']).to(DEV)
    return [t[o:] for o in inp['offsets']], inp['sizes'], inp['strides']


def rows_of(t, inp):
    """a device output over `sizes` (+ a trailing axis) as (rows[, n])"""
    if t is None:
        return None
    a = t.cpu().numpy()
    assert a.shape[:len(inp['sizes'])] == tuple(inp['sizes'])
    return a.reshape((inp['X'].shape[0],) + a.shape[len(inp['sizes']):])


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def labels_and_proba(got, want, inp):
    """what was asked for is there; labels equal with NaN on the masked rows; probabilities bit for bit"""
    for key in ('labels', 'proba'):
        if inp['outputs'] in ('both', key):
            if key not in got or not same_bits(got[key], want[key]):
                return False
    return True


# ---- forest: kernels.classify_forest against classify_ref.forest_proba / forest_predict -------------------
def draw_tree(rng, nfeat, values, max_depth, pool):
    """one unbalanced tree as scikit-learn's arrays (children follow their parent); thresholds are the data's
    own values, their float64 neighbours (no float32 numbers) or points between"""
    feature, threshold, left, right = [], [], [], []

    def grow(depth):
        i = len(feature)
        feature.append(-2)
        threshold.append(-2.0)
        left.append(-1)
        right.append(-1)
        if depth < max_depth and rng.random() < (1.0 if depth == 0 and max_depth else 0.7):
            f = int(rng.integers(0, nfeat))
            v = float(values[int(rng.integers(0, values.shape[0])), f]) if values.shape[0] else 0.0
            v = v if np.isfinite(v) else 0.0
            how = rng.random()
            if how < 0.3:
                v = float(np.nextafter(v, np.inf if rng.random() < 0.5 else -np.inf))
            elif how < 0.5:
                v = v * float(rng.uniform(0.5, 1.5))
            feature[i], threshold[i] = f, v
            left[i] = grow(depth + 1)
            right[i] = grow(depth + 1)
        return i
    grow(0)
    value = pool[rng.integers(0, pool.shape[0], len(feature))]
    return feature, threshold, left, right, value


def gen_forest(rng):
    nfeat = draw_features(rng)
    dtype = str(rng.choice(['float32', 'float64']))
    table, desc = gen_rows(rng, nfeat, dtype, max_rows=3000 if nfeat < 64 else 600, corners=(0.0, -1.0, np.inf, -np.inf))
    mean, scale = draw_scaler(rng, table['X'])
    inp = dict(table, mean=mean, scale=scale)
    _, Xs = model_rows(inp)
    ncls = int(rng.choice(CLASS_COUNTS))
    ntrees, depth = int(rng.integers(1, 21)), int(rng.integers(0, 9))
    # few leaf distributions, half of them eighths: leaves share rows and class totals tie exactly
    pool = np.concatenate([rng.integers(0, 5, (3, ncls)) / 8.0, rng.random((2, ncls))])
    parts = [draw_tree(rng, nfeat, Xs.astype(np.float32), depth, pool) for _ in range(ntrees)]
    cat = lambda j, dt: np.concatenate([np.asarray(p[j], dt) for p in parts])       # noqa: E731
    inp.update(feature=cat(0, np.int64), threshold=cat(1, np.float64), left=cat(2, np.int64), right=cat(3, np.int64),
               value=np.concatenate([p[4] for p in parts]).astype(np.float64),
               tree_offsets=np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64),
               classes=np.sort(rng.normal(size=ncls) * 100), outputs=str(rng.choice(['both', 'labels', 'proba'])))
    desc.update(scaler=mean is not None, classes=ncls, trees=ntrees, depth=depth, nodes=int(inp['feature'].size),
                outputs=inp['outputs'])
    return inp, desc


def want_forest(inp):
    from tests import classify_ref as ref
    keep, Xp = model_rows(inp)
    proba = ref.forest_proba(Xp, inp['feature'], inp['threshold'], inp['left'], inp['right'], inp['value'],
                             inp['tree_offsets'])
    return dict(proba=ref.masked(proba, keep), labels=ref.masked(ref.forest_predict(proba, inp['classes']), keep))


def run_forest(inp):
    from nd_amd import classify
    nodes, roots = classify.pack_forest(inp['feature'], inp['threshold'], inp['left'], inp['right'], inp['tree_offsets'])
    feats, sizes, strides = device_table(inp)
    labels, proba = kernels.classify_forest(
        feats, sizes, strides, up(nodes.view(np.uint8).reshape(-1)), up(inp['value']), up(roots), up(inp['classes']),
        inp['mean'], inp['scale'], want_labels=inp['outputs'] != 'proba', want_proba=inp['outputs'] != 'labels')
    got = dict(labels=rows_of(labels, inp), proba=rows_of(proba, inp))
    return {key: a for key, a in got.items() if a is not None}


compare_forest = labels_and_proba


# ---- kmeans_predict: kernels.classify_kmeans against classify_ref.kmeans_labels -----------------------------
def draw_centres(rng, Xs, k, nfeat):
    """k distinct valid rows x 1.0625 (fewer where there are fewer; normal draws where there is none)"""
    rows = np.unique(Xs[np.isfinite(Xs).all(axis=1)].astype(np.float64), axis=0)
    if not rows.shape[0]:
        return rng.normal(size=(k, nfeat))
    return rows[rng.choice(rows.shape[0], size=min(k, rows.shape[0]), replace=False)] * 1.0625


def gen_kmeans_predict(rng):
    nfeat = draw_features(rng)
    dtype = str(rng.choice(['float32', 'float64']))
    table, desc = gen_rows(rng, nfeat, dtype, max_rows=3000 if nfeat < 64 else 600)
    mean, scale = draw_scaler(rng, table['X'])
    inp = dict(table, mean=mean, scale=scale)
    centers = draw_centres(rng, model_rows(inp)[1], int(rng.integers(1, 41)), nfeat)
    planted = bool(rng.random() < 0.2 and centers.shape[0] >= 2)
    if planted:                                                   # duplicates: the lower index wins
        for _ in range(int(rng.integers(1, 4))):
            i, j = rng.integers(0, centers.shape[0], 2)
            centers[int(j)] = centers[int(i)]
    inp.update(centers=centers, planted=planted)
    desc.update(scaler=mean is not None, k=int(centers.shape[0]), planted=planted)
    return inp, desc


def want_kmeans_predict(inp):
    from tests import classify_ref as ref
    keep, Xp = model_rows(inp)
    with np.errstate(all='ignore'):
        labels, gap = ref.kmeans_labels(Xp, inp['centers']), ref.kmeans_gap(Xp, inp['centers'])
    return dict(labels=ref.masked(labels, keep), gap=ref.masked(gap, keep))


def run_kmeans_predict(inp):
    feats, sizes, strides = device_table(inp)
    return dict(labels=rows_of(kernels.classify_kmeans(feats, sizes, strides, up(inp['centers']), inp['mean'],
                                                       inp['scale']), inp))


def compared_rows(want, inp):
    """the rows kmeans_predict compares: every valid row of a planted-duplicate case, else those whose two
    nearest centres are 1e-12 apart in relative squared distance (the rule of test_kmeans_labels)"""
    keep = ~np.isnan(want['labels'])
    return keep if inp['planted'] else keep & (np.nan_to_num(want['gap']) >= 1e-12)


def compare_kmeans_predict(got, want, inp):
    g, w = got['labels'], want['labels']
    if g.shape != w.shape or g.dtype != np.float64 or not np.array_equal(np.isnan(g), np.isnan(w)):
        return False
    ok = compared_rows(want, inp)
    return bool(np.array_equal(g[ok], w[ok]))


# ---- knn: kernels.classify_knn against classify_knn_linear_ref.knn_proba -------------------------------------
def gen_knn(rng):
    nfeat = draw_features(rng, rare=(128,))
    dtype = str(rng.choice(['float32', 'float64']))
    ntrain = int(rng.choice([1, 2, 7, 8, 9, 17, 64, 100, 257, 1000]))
    k = min(ntrain, int(rng.choice([1, 2, 3, 4, 5, 8, 9, 16, 17, 32])))
    integers = bool(rng.random() < 0.25)
    table, desc = gen_rows(rng, nfeat, dtype, max_rows=max(1, min(3000, 6000000 // (ntrain * nfeat))), integers=integers)
    mean, scale = draw_scaler(rng, table['X'])
    inp = dict(table, mean=mean, scale=scale)
    _, Xs = model_rows(inp)
    rows = Xs[np.isfinite(Xs).all(axis=1)].astype(np.float64)
    if rows.shape[0]:                       # samples among the queries (distance 0, exact ties), and near them
        train = rows[rng.integers(0, rows.shape[0], ntrain)]
        if not integers:
            train = train * np.where(rng.random((ntrain, 1)) < 0.5, 1.0, rng.uniform(0.5, 1.5, (ntrain, nfeat)))
    else:
        train = rng.normal(size=(ntrain, nfeat))
    ncls = int(rng.choice(CLASS_COUNTS))
    inp.update(train=np.ascontiguousarray(train), target=rng.integers(0, ncls, ntrain).astype(np.int32),
               classes=np.sort(rng.normal(size=ncls) * 100), k=k, outputs=str(rng.choice(['both', 'labels', 'proba'])))
    desc.update(scaler=mean is not None, ntrain=ntrain, k=k, classes=ncls, integers=integers, outputs=inp['outputs'])
    return inp, desc


def want_knn(inp):
    from tests import classify_knn_linear_ref as kl, classify_ref as ref
    keep, Xp = model_rows(inp)
    with np.errstate(all='ignore'):
        proba, _ = kl.knn_proba(Xp, inp['train'], inp['target'], inp['k'], inp['classes'].size)
    return dict(proba=ref.masked(proba, keep), labels=ref.masked(kl.first_max(proba, inp['classes']), keep))


def run_knn(inp):
    feats, sizes, strides = device_table(inp)
    labels, proba = kernels.classify_knn(
        feats, sizes, strides, up(inp['train']), up(inp['target']), up(inp['classes']), inp['k'], inp['mean'],
        inp['scale'], want_labels=inp['outputs'] != 'proba', want_proba=inp['outputs'] != 'labels')
    got = dict(labels=rows_of(labels, inp), proba=rows_of(proba, inp))
    return {key: a for key, a in got.items() if a is not None}


compare_knn = labels_and_proba              # knn_check: bit for bit on every row


# ---- linear: kernels.classify_linear against classify_knn_linear_ref.linear_decision ------------------------
def gen_linear(rng):
    nfeat = draw_features(rng)
    dtype = str(rng.choice(['float32', 'float64']))
    table, desc = gen_rows(rng, nfeat, dtype, max_rows=3000 if nfeat < 64 else 600)
    mean, scale = draw_scaler(rng, table['X'])
    ncoef = int(rng.choice([1, 2, 3, 8, 9, 11, 17]))
    spread = 1.0 / max(float(np.nanmax(np.abs(np.where(np.isfinite(table['X']), table['X'], 0)))), 1e-30) \
        if mean is None else 1.0
    coef, intercept = rng.normal(size=(ncoef, nfeat)) * spread, rng.normal(size=ncoef)
    special = bool(rng.random() < 0.1)
    if special:
        coef[int(rng.integers(0, ncoef))] = 0.0
        if ncoef >= 3:
            coef[2], intercept[2] = coef[1], intercept[1]
    link = str(rng.choice(['none', 'softmax', 'ovr']))
    inp = dict(table, mean=mean, scale=scale, coef=coef, intercept=intercept, link=link,
               classes=np.sort(rng.normal(size=2 if ncoef == 1 else ncoef) * 100))
    desc.update(scaler=mean is not None, ncoef=ncoef, link=link, special=special)
    return inp, desc


def want_linear(inp):
    from tests import classify_knn_linear_ref as kl, classify_ref as ref
    keep, Xp = model_rows(inp)
    with np.errstate(all='ignore'):
        s, _ = kl.linear_decision(Xp, inp['coef'], inp['intercept'])
        want = dict(decision=ref.masked(s, keep), labels=ref.masked(kl.linear_predict(s, inp['classes']), keep))
        if inp['link'] != 'none':
            want['proba'] = ref.masked(kl.linear_proba(s, inp['link']), keep)
    return want


def run_linear(inp):
    feats, sizes, strides = device_table(inp)
    args = (up(inp['coef']), up(inp['intercept']), up(inp['classes']), inp['link'])
    funcs = dict(decision='decision_function', labels='predict', **({} if inp['link'] == 'none' else {'proba': 'predict_proba'}))
    return {key: rows_of(kernels.classify_linear(feats, sizes, strides, *args, func, inp['mean'], inp['scale']), inp)
            for key, func in funcs.items()}


def compare_linear(got, want, inp):
    """linear_check: decision values bit for bit, labels equal, probabilities within 4 (n + 4) 2^-53"""
    if set(got) != set(want) or not same_bits(got['decision'], want['decision']) \
            or not same_bits(got['labels'], want['labels']):
        return False
    if 'proba' in want:
        g, w = got['proba'], want['proba']
        n = inp['classes'].size
        if g.shape != w.shape or not np.array_equal(np.isnan(g), np.isnan(w)):
            return False
        with np.errstate(all='ignore'):
            return bool(np.allclose(g, w, rtol=0, atol=4 * (n + 4) * 2.0 ** -53, equal_nan=True))
    return True


# ---- kmeans_step: kernels.kmeans_step and kernels.feature_moments against tests/kmeans_fit_ref.py -----------
KMEANS_FIT_MAX_ACC = 4096


def gen_kmeans_step(rng):
    nfeat = draw_features(rng)
    dtype = str(rng.choice(['float32', 'float64']))
    table, desc = gen_rows(rng, nfeat, dtype, max_rows=3000 if nfeat < 64 else 600)
    limit = KMEANS_FIT_MAX_ACC // (nfeat + 1)
    at_limit = bool(rng.random() < 0.1)
    k = limit - int(rng.integers(0, 2)) if at_limit else int(rng.integers(1, min(40, limit) + 1))
    empty = bool(rng.random() < 0.05)
    if empty:                                                       # no valid row: one feature is NaN throughout
        table['buf'][table['offsets'][int(rng.integers(0, nfeat))] + table['rowoff']] = np.nan
        table['X'] = read_rows(table)
    mean, scale = draw_scaler(rng, table['X'])
    inp = dict(table, mean=mean, scale=scale)
    _, Xs = model_rows(inp)
    centers = draw_centres(rng, Xs, k, nfeat)
    if centers.shape[0] < k:                                        # fewer distinct rows than centres: fill up
        centers = np.concatenate([centers, rng.normal(size=(k - centers.shape[0], nfeat)) * (np.abs(centers).max() + 1)])
    first = bool(rng.random() < 0.5)
    prev = np.full(table['X'].shape[0], -1, np.int32) if first else rng.integers(-1, k, table['X'].shape[0]).astype(np.int32)
    inp.update(centers=centers, prev=prev)
    desc.update(scaler=mean is not None, k=k, at_limit=at_limit, empty=empty, first=first)
    return inp, desc


def want_kmeans_step(inp):
    from tests import kmeans_fit_ref as kf
    with np.errstate(all='ignore'):
        labels, sums, counts, inertia, changed, mag = kf.step(inp['X'], inp['centers'], inp['prev'], inp['mean'], inp['scale'])
        n, m, var = kf.moments(inp['X'], inp['mean'], inp['scale'])
        V, valid = kf.values(inp['X'], inp['mean'], inp['scale'])
        mmag = np.abs(V[valid]).sum(axis=0) / n if n else np.full(V.shape[1], np.nan)
    return dict(labels=labels, sums=sums, counts=counts, inertia=np.float64(inertia), changed=np.int64(changed), mag=mag,
                count=np.int64(n), mean=m, var=var, mean_mag=mmag)


def run_kmeans_step(inp):
    feats, sizes, strides = device_table(inp)
    labels = up(inp['prev']).reshape(sizes).contiguous()
    sums, counts, inertia, changed = kernels.kmeans_step(feats, sizes, strides, up(inp['centers']), labels, inp['mean'],
                                                         inp['scale'])
    count, fmean, fvar = kernels.feature_moments(feats, sizes, strides, inp['mean'], inp['scale'])
    return dict(labels=host(labels).reshape(-1), sums=host(sums), counts=host(counts), inertia=host(inertia),
                changed=host(changed), count=host(count), mean=host(fmean), var=host(fvar))


def compare_kmeans_step(got, want, inp):
    """check_step and check_moments of tests/test_kmeans_fit_gpu.py: labels, counts, changed and the row count
    equal; float64 sums within rows * 2^-52 of the magnitudes behind them"""
    bound = inp['X'].shape[0] * 2.0 ** -52
    with np.errstate(all='ignore'):
        if not (np.array_equal(got['labels'], want['labels']) and np.array_equal(got['counts'], want['counts'])
                and int(got['changed']) == int(want['changed']) and int(got['count']) == int(want['count'])):
            return False
        if not np.all(np.abs(got['sums'] - want['sums']) - bound * want['mag'] <= 0):
            return False
        if not abs(float(got['inertia']) - float(want['inertia'])) <= bound * float(want['inertia']):
            return False
        if int(want['count']) == 0:
            return bool(np.isnan(got['mean']).all() and np.isnan(got['var']).all())
        mag, var = want['mean_mag'], want['var']
        slack = bound * (var + 2 * mag * np.sqrt(var)) + (bound * mag) ** 2
        return bool(np.all(np.abs(got['mean'] - want['mean']) <= bound * mag)
                    and np.all(np.abs(got['var'] - want['var']) <= slack))


# ---- to_rgb: kernels.rgb_limits and kernels.rgb_compose against tests/rgb_ref.py -------------------------------
RGB_RECIPES = ('exponential', 'some_nan', 'all_nan', 'infinities', 'ties16', 'constant', 'denormal_zero',
               'one_binade', 'scaled')


def draw_rgb_stack(rng, recipe, shape, dtype):
    """the value recipes of tests/rgb_cases.py: planes, on a (frames, y, x) stack"""
    T = np.dtype(dtype).type
    if recipe == 'all_nan':
        return np.full(shape, np.nan, dtype)
    if recipe == 'ties16':
        return rng.integers(0, 16, shape).astype(dtype)
    if recipe == 'constant':
        return np.full(shape, 3.25, dtype)
    if recipe == 'one_binade':
        return (1 + rng.random(shape)).astype(dtype)
    if recipe == 'denormal_zero':
        a = rng.standard_normal(shape).astype(dtype) * T(np.finfo(dtype).tiny) * T(0.25)
        a[rng.random(shape) < 0.3] = 0.0
        a[rng.random(shape) < 0.3] = -0.0
        return a
    a = rng.exponential(size=shape).astype(dtype)
    if recipe == 'some_nan':
        a[rng.random(shape) < 0.2] = np.nan
    elif recipe == 'infinities':
        a[rng.random(shape) < 0.1] = np.inf
        a[rng.random(shape) < 0.1] = -np.inf
    elif recipe == 'scaled':
        a = a * T(rng.choice([1e-6, 1e-3, 1e4, 1e6]))
    return a


def gen_to_rgb(rng):
    from tests import rgb_cases
    dtype = str(rng.choice(['float32', 'float64']))
    nch, k = int(rng.choice([1, 3])), int(rng.integers(1, 5))
    nx = int(rng.integers(1, 10)) if rng.random() < 0.4 else draw_extent(rng, 300)                  # the store tails
    ny = int(rng.integers(1, max(1, min(40, 4000 // (nx * k))) + 1))
    shape = (k, ny, nx)
    stacks, channels, recipes = [], [], []
    for _ in range(nch):
        recipe = str(rng.choice(RGB_RECIPES))
        recipes.append(recipe)
        stacks.append(draw_rgb_stack(rng, recipe, shape, dtype))
        if rng.random() < 0.25:                      # a quotient channel: x / 0 is an infinity, 0 / 0 a NaN
            den = rng.exponential(size=shape).astype(dtype)
            den[rng.random(shape) < 0.1] = 0
            both = rng.random(shape) < 0.05
            den[both] = 0
            stacks[-1][both] = 0
            stacks.append(den)
            channels.append((len(stacks) - 2, len(stacks) - 1))
            recipes[-1] += '/quotient'
        else:
            channels.append((len(stacks) - 1, None))
    if rng.random() < 0.5:
        pmin, pmax = (float(v) for v in rng.choice(rgb_cases.PERCENTILES, 2))
    else:
        pmin, pmax = (float(v) for v in rng.uniform(0, 100, 2))
    vmin = vmax = None
    given = str(rng.choice(['vmin', 'vmax', 'both'])) if rng.random() < 1 / 3 else 'none'
    if given != 'none':
        fin = stacks[0][np.isfinite(stacks[0])].astype(np.float64)
        lo, hi = (np.quantile(fin, [0.1, 0.9]) if fin.size else (0.5, 1.5))
        per_channel = bool(rng.random() < 0.5)
        draw = lambda c: [float(c * rng.uniform(0.5, 1.5)) for _ in range(nch)] if per_channel else [float(c)] * nch  # noqa: E731
        vmin = draw(lo) if given in ('vmin', 'both') else None
        vmax = draw(hi) if given in ('vmax', 'both') else None
        if given == 'both' and rng.random() < 0.2:
            vmin, vmax = vmax, (vmin if rng.random() < 0.5 else vmax)                                 # reversed, or equal
    mask = (rng.random((ny, nx)) < 0.7) if rng.random() < 1 / 3 else None
    layout = str(rng.choice(STACK_LAYOUTS))
    desc = dict(dtype=dtype, channels=nch, frames=k, ny=ny, nx=nx, recipes=recipes, pmin=pmin, pmax=pmax, vmin=vmin,
                vmax=vmax, mask=mask is not None, layout=layout)
    return dict(stacks=stacks, channels=channels, pmin=pmin, pmax=pmax, vmin=vmin, vmax=vmax, mask=mask, layout=layout), desc


def want_to_rgb(inp):
    from tests import rgb_ref
    stacks = inp['stacks']
    with np.errstate(all='ignore'):
        chans = [stacks[a] if b is None else stacks[a] / stacks[b] for a, b in inp['channels']]
        k = chans[0].shape[0]
        limits = np.array([[rgb_ref.limits(ch[t], inp['pmin'], inp['pmax']) for ch in chans] for t in range(k)],
                          dtype=chans[0].dtype)
        counts = np.array([[np.count_nonzero(~np.isnan(ch[t])) for ch in chans] for t in range(k)], np.int64)
        rgb = np.stack([rgb_ref.composite([ch[t] for ch in chans], inp['vmin'], inp['vmax'], inp['pmin'], inp['pmax'],
                                          inp['mask']) for t in range(k)])
    return dict(limits=limits, counts=counts, rgb=rgb)


def run_to_rgb(inp):
    views, dims, _ = device_planes(inp['stacks'], inp['layout'])
    if dims[0] == 'y':
        views = [v.permute(2, 0, 1) for v in views]
    channels = [views[a] if b is None else (views[a], views[b]) for a, b in inp['channels']]
    limits, counts = kernels.rgb_limits(channels, inp['pmin'], inp['pmax'])
    mask = None if inp['mask'] is None else torch.from_numpy(inp['mask']).to(DEV)
    rgb = kernels.rgb_compose(channels, limits, inp['vmin'], inp['vmax'], mask)
    return dict(limits=host(limits), counts=host(counts), rgb=host(rgb))


def compare_to_rgb(got, want, inp):
    """limits same() as rgb_ref.nanpercentile (equal values of the data type, NaN where NaN), counts equal,
    composite bytes equal"""
    from tests.test_to_rgb_cpu import same
    return bool(same(got['limits'], want['limits']) and got['counts'].dtype == np.int64
                and np.array_equal(got['counts'], want['counts']) and got['rgb'].dtype == np.uint8
                and np.array_equal(got['rgb'], want['rgb']))


# ---- warp: kernels.warp_translate against coreg_ref.warp_stack ---------------------------------------------------
def gen_warp(rng):
    dtype = str(rng.choice(['float32', 'float64']))
    nv, k = int(rng.integers(1, 4)), int(rng.integers(1, 7))
    nr = int(rng.integers(1, 41))
    nc = draw_extent(rng, 130) if rng.random() < 0.5 else int(rng.integers(1, 41))
    kinds = [str(rng.choice(['positive', 'mixed', 'negative'])) for _ in range(nv)]
    scale = float(rng.choice(SCALES))
    planes = []
    for kind in kinds:
        a = rng.gamma(4.0, 0.25, (k, nr, nc)) + 0.5 if kind != 'mixed' else rng.normal(size=(k, nr, nc))
        planes.append(((-a if kind == 'negative' else a) * scale).astype(dtype))
    corner = plant_corners(rng, planes, values=(0.0, -1.0))
    sh = np.stack([rng.uniform(-(nr + 2), nr + 2, k), rng.uniform(-(nc + 2), nc + 2, k)], axis=1)
    how = rng.random((k, 2))
    sh = np.where(how < 0.3, np.round(sh), np.where(how < 0.6, np.round(sh * 2) / 2, sh))          # integers, halves
    reference = int(rng.integers(-1, k))
    layout = str(rng.choice(['planar', 'pixel_major']))
    desc = dict(dtype=dtype, variables=kinds, k=k, rows=nr, cols=nc, scale=scale, corner=corner, shifts=sh.tolist(),
                reference=reference, layout=layout)
    return dict(planes=planes, shifts=sh, reference=reference, layout=layout, dtype=dtype), desc


def want_warp(inp):
    from tests import coreg_ref
    with np.errstate(all='ignore'):
        return {'v%d' % i: coreg_ref.warp_stack(a, inp['shifts'], inp['reference']) for i, a in enumerate(inp['planes'])}


def run_warp(inp):
    pm = inp['layout'] == 'pixel_major'
    tens = [up(np.moveaxis(a, 0, -1) if pm else a) for a in inp['planes']]
    res = kernels.warp_translate(tens, up(inp['shifts']), inp['reference'], inp['layout'])
    return {'v%d' % i: np.ascontiguousarray(np.moveaxis(host(r), -1, 0) if pm else host(r)) for i, r in enumerate(res)}


def compare_warp(got, want, inp):
    """float64 bit-equal; float32 within 1e-6 max |want| (_check_out of tests/test_coregister_gpu.py)"""
    for key, w in want.items():
        g = got.get(key)
        if g is None or g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(np.isnan(g), np.isnan(w)):
            return False
        if inp['dtype'] == 'float64':
            if not np.array_equal(g, w, equal_nan=True):
                return False
        elif not np.allclose(g, w, rtol=0, atol=1e-6 * float(np.nanmax(np.abs(w))), equal_nan=True):
            return False
    return True


# ---- c3: the full-pol test in every layout and through the pixel-major entry point, with its rasters -----------
C3_NAMES = ('C11', 'C22', 'C33', 'C12re', 'C12im', 'C13re', 'C13im', 'C23re', 'C23im')
C3_KS = (2, 3, 4, 7, 12, 24, 33, 48, 63, 64, 65)
C3_MORE_KS = (5, 8, 16, 32, 96)


def gen_c3(rng, ks=C3_KS):
    """(the draws up to the planes are those of the round-6 family, in their order: a seed gives the same planes)"""
    k = int(rng.choice(list(ks)))
    ny, nx = int(rng.integers(1, 20)), int(rng.integers(1, 200))
    looks = int(rng.choice([3, 9, 16]))
    dtype = rng.choice([np.float32, np.float64])
    alpha = float(rng.choice([1e-4, 0.01, 0.1, 0.5, 0.9, 0.99, 0.9999]))
    w = wishart(rng, k, ny, nx, looks, dtype, pol=3)
    planes = [w[n] for n in C3_NAMES]
    if rng.random() < 0.7:
        m = rng.random((ny, nx)) < 0.3
        t0 = rng.integers(1, k, (ny, nx))
        g = np.where((np.arange(k)[:, None, None] >= t0[None]) & m[None], 5.0, 1.0)
        planes = [(p * g).astype(dtype) for p in planes]
    corner = False
    if rng.random() < 0.3:       # zeros, NaNs, infinities, negative entries, a global scale
        corner = True
        bad = rng.random((k, ny, nx)) < 0.01
        planes[int(rng.integers(0, 9))][bad] = rng.choice([0.0, np.nan, np.inf, -1.0])
        planes = [(p * rng.choice([1.0, 1e-6, 1e5])).astype(dtype) for p in planes]
    layout = str(rng.choice(['tyx', 'yxt', 'pad', 'pm', 'pmc']))
    stats = bool(rng.random() < 0.5)
    desc = dict(k=k, ny=ny, nx=nx, looks=looks, dtype=np.dtype(dtype).name, alpha=alpha, corner=corner, layout=layout,
                stats=stats)
    return dict(planes=planes, alpha=alpha, looks=looks, layout=layout, stats=stats), desc


def gen_c3_more(rng):
    return gen_c3(rng, C3_MORE_KS)


def want_c3(inp):
    with np.errstate(all='ignore'):
        m, z, P = O.change_detection_pol([np.moveaxis(p, 0, -1) for p in inp['planes']], 3, inp['alpha'], inp['looks'],
                                         njobs=8, stats=True)
    return dict(map=m, z=z, P=P)


def run_c3(inp):
    layout, kw = inp['layout'], dict(alpha=inp['alpha'], n=inp['looks'], stats=inp['stats'])
    res = None
    if layout in ('pm', 'pmc'):
        # the reference's own layout through the pixel-major kernel (complex off-diagonals for 'pmc'); where the
        # entry point declines, the planar call on the same memory
        dev = [up(np.moveaxis(p, 0, -1)) for p in inp['planes']]
        if layout == 'pmc':
            for i in (3, 5, 7):
                c = torch.complex(dev[i], dev[i + 1])
                dev[i], dev[i + 1] = c.real, c.imag
        res = kernels.change_detection_c3_pixel_major(dev, **kw)
        if res is None:
            res = kernels.change_detection_c3([d.contiguous() for d in dev], dims=('y', 'x', 'time'), **kw)
    else:
        views, dims, _ = device_planes(inp['planes'], layout)
        res = kernels.change_detection_c3(views, dims=dims, **kw)
    if inp['stats']:
        return dict(map=host(res[0]), z=host(res[1]), P=host(res[2]))
    return dict(map=host(res))


def compare_c3(got, want, inp):
    """maps equal; z within 1e-5 relative, P within 1e-5 relative and 1e-30 (tests/test_omnibus_c3_gpu.py)"""
    if not (got['map'].dtype == np.uint8 and np.array_equal(got['map'], want['map'])):
        return False
    if 'z' in got:
        with np.errstate(all='ignore'):
            return bool(got['z'].shape == want['z'].shape and got['P'].shape == want['P'].shape
                        and np.allclose(got['z'], want['z'], rtol=1e-5, atol=0, equal_nan=True)
                        and np.allclose(got['P'], want['P'], rtol=1e-5, atol=1e-30, equal_nan=True))
    return True


# ---- rasterize: kernels.rasterize_polygons against tests/rasterize_ref.py ---------------------------------------------
RASTER_LAYOUTS = ('lyx', 'yxl', 'pad')


def gen_rasterize(rng):
    """random polygon sets (stars, holes, half-integer snaps, combs around the crossing list's capacity, polygons
    off the raster, empty ones), a random grid of either orientation, layers, value types and output strides"""
    from tests import rasterize_cases as cases
    ny, nx = draw_extent(rng, 70), draw_extent(rng, 130)
    n = int(rng.choice([0, 1, 2, 5, 20, 40]))
    polys = []
    for k in range(n):
        kind = rng.random()
        if kind < 0.06:
            crossings = int(rng.choice([cases.MAX_CROSSINGS - 2, cases.MAX_CROSSINGS, cases.MAX_CROSSINGS + 2,
                                        2 * cases.MAX_CROSSINGS + 2]))
            polys.append(cases.comb(crossings, x1=nx - 0.3 if (nx >= 40 and rng.random() < 0.5) else 39.7,
                                    ytop=float(rng.uniform(0.7, ny + 1))))
        elif kind < 0.1:
            polys.append([] if rng.random() < 0.5 else [rng.uniform(0, nx, (2, 2))])
        else:
            g = cases.random_polygon(rng, ny, nx, hole=bool(rng.random() < 0.4), m=int(rng.choice([3, 4, 7, 12, 64, 65, 130])))
            scale = float(rng.choice([0.1, 0.3, 1.0, 3.0]))
            c = g[0].mean(0)
            g = [c + (ring - c) * scale for ring in g]
            polys.append([cases.snap(ring) for ring in g] if rng.random() < 0.2 else g)
    # the grid: world = c + a * px, pixel coordinates come back through the bracketed division
    a = float(rng.choice([1.0, -1.0, 10.0, -0.25, 1 / 3]))
    e = float(rng.choice([1.0, -1.0, -10.0, 0.25, -1 / 3]))
    c, f = float(rng.choice([0.0, 5e5, -37.3])), float(rng.choice([0.0, 4.2e6, 11.1]))
    world = [[np.stack([c + a * r[:, 0], f + e * r[:, 1]], axis=1) for r in g] for g in polys]
    nlayers = int(rng.choice([1, 1, 2, 3]))
    layer = rng.integers(0, nlayers, n) if (nlayers > 1 or rng.random() < 0.3) else None
    floats = bool(rng.random() < 0.5)
    if floats:
        values = rng.choice([np.nan, -0.0, 1.5, -2.25, np.inf, 1e-310, 3.0], n).astype(np.float64)
        fill = float(rng.choice([0.0, -1.0, np.nan]))
    else:
        values = rng.choice([1, 2, 3, -7, 2 ** 53 + 1, -2 ** 62 - 1, 0], n).astype(np.int64)
        fill = int(rng.choice([0, -1, 2 ** 40]))
    layout = str(rng.choice(RASTER_LAYOUTS))
    table = bool(rng.random() < 0.5)
    desc = dict(ny=ny, nx=nx, n=n, a=a, e=e, c=c, f=f, nlayers=nlayers, layered=layer is not None, floats=floats,
                fill=fill, layout=layout, table=table)
    return dict(world=world, transform=(a, 0.0, c, 0.0, e, f), ny=ny, nx=nx, values=values, layer=layer,
                nlayers=nlayers, fill=fill, layout=layout, table=table), desc


def want_rasterize(inp):
    from tests import rasterize_ref as R
    polys = [[R.to_pixel(r, inp['transform']) for r in g] for g in inp['world']]
    return dict(out=R.burn(polys, inp['values'], inp['ny'], inp['nx'], layer=inp['layer'], nlayers=inp['nlayers'],
                           fill=inp['fill']))


def run_rasterize(inp):
    from nd_amd import vector
    from tests import rasterize_ref as R
    ny, nx, nl = inp['ny'], inp['nx'], inp['nlayers']
    polys = [[vector._to_pixel(r, inp['transform']) for r in g] for g in inp['world']]
    verts, ro, po = R.pack(polys)
    dt = torch.float64 if inp['values'].dtype.kind == 'f' else torch.int64
    if inp['layout'] == 'lyx':
        base, out = None, None
    elif inp['layout'] == 'yxl':
        base = torch.full((ny, nx, nl), 77, dtype=dt, device=DEV)
        out = base.permute(2, 0, 1)
    else:
        base = torch.full((nl, ny + 2, nx + 5), 77, dtype=dt, device=DEV)
        out = base[:, 1:ny + 1, 3:nx + 3]
    args = (kernels.PolygonTable(verts, ro, po, ny, nx, device=DEV), None, None) if inp['table'] else (verts, ro, po)
    res = kernels.rasterize_polygons(*args, inp['values'], ny, nx, layer=inp['layer'], nlayers=nl, fill=inp['fill'],
                                     out=out)
    got = dict(out=host(res))
    if inp['layout'] == 'pad':
        frame = base.clone()
        frame[:, 1:ny + 1, 3:nx + 3] = 77
        got['untouched'] = np.asarray(bool((frame == 77).all()))
    return got


def compare_rasterize(got, want, inp):
    """the same type, shape and bytes everywhere (no tolerance, no excluded pixels); nothing written around a view"""
    g, w = np.ascontiguousarray(got['out']), want['out']
    return bool(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
                and bool(got.get('untouched', True)))


want_c3_more, run_c3_more, compare_c3_more = want_c3, run_c3, compare_c3


def newer_case(name):
    gen, want_of, run, compare = (globals()[p + name] for p in ('gen_', 'want_', 'run_', 'compare_'))

    def case(rng):
        inputs, desc = gen(rng)
        want = want_of(inputs)
        got = run(inputs)
        LAST.clear()
        LAST.update(name=name, got=got, want=want)
        return bool(compare(got, want, inputs)), desc
    return case


NEWER = ('omnibus_diag', 'change_segments', 'to_rgb', 'forest', 'kmeans_predict', 'knn', 'linear', 'kmeans_step', 'warp',
         'c3_more', 'rasterize')


CASES = {'omnibus': case_omnibus, 'omnibus_long': case_omnibus_long, 'omnibus_ml': case_omnibus_ml, 'c3': newer_case('c3'),
         'nlmeans': case_nlmeans, 'correlate': case_correlate, 'gaussian': case_gaussian}
CASES.update({name: newer_case(name) for name in NEWER})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=60.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--what', default=','.join(CASES))
    a = ap.parse_args()
    names = a.what.split(',')
    O.build()
    count = {n: 0 for n in names}
    fails = 0
    t_end = time.time() + a.seconds
    i = 0
    t_say = time.time() + 60.0
    while time.time() < t_end:
        if time.time() > t_say:              # a heartbeat: silent runs are taken for hung ones
            print('progress', count, 'failures', fails, flush=True)
            t_say = time.time() + 60.0
        name = names[i % len(names)]
        rng = np.random.default_rng([a.seed, i])
        try:
            ok, desc = CASES[name](rng)
        except Exception as e:
            # an error is a failure too, and the last case: the device may have faulted, nothing more is run on it
            print('FAIL %s seed=(%d,%d) %s' % (name, a.seed, i, {'exception': repr(e)}), flush=True)
            print('cases', count, 'failures', fails + 1, 'stopped by the exception above')
            sys.exit(2)
        count[name] += 1
        if not ok:
            fails += 1
            print('FAIL %s seed=(%d,%d) %s' % (name, a.seed, i, desc), flush=True)
        i += 1
    print('cases', count, 'failures', fails, 'ill-posed n_eff swaps (not failures)', ILL_POSED[0])
    sys.exit(1 if fails else 0)


if __name__ == '__main__':
    main()
