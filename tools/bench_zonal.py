"""Secondary measurement: kernels.zonal_stats (count, nan_count, sum, min, max, m2) of 24 dates of 4096 x 4096 float32
gamma speckle with 1 % NaN, in (time, y, x) memory and in (y, x, time) memory, inside three zone maps:

    parcels   10 000 random parcels rasterized as in tools/bench_rasterize.py
    regions   the regions at connectivity 4 of OmnibusTest(n = 9, alpha = 0.99)'s change map for one date
    half      one zone of half the raster

For each: the index build (kernels.zonal_index: keys, torch's stable sort and search) timed on its own, then the minimum
of 7 kernels.zonal_stats calls, device events around the call, after 2 warm-up calls.  Next to each figure:

    the definition's own traffic at 8 TB/s: the data bytes of the zoned pixels once, and 4 index bytes per zoned pixel
        once per call
    torch on the device by hand: index_add_ (sum, count, and the squares around the mean in a second pass) and
        scatter_reduce (amin, amax) on the flattened (time, y, x) planes with float64 accumulators, one call after a
        warm-up call; this skips no NaN
    scipy.ndimage.mean + variance on the host for 2 of the planes (NaN replaced by 0), and that time for all the planes

Before timing, a band of rows of every zone map is compared with the restatement (tests/zonal_ref.py), bit for bit.
Writes profiles/zonal_bench.json (or the path given) and prints it.

    python tools/bench_zonal.py [--out PATH] [--size N] [--dates K] [--reps N] [--band ROWS]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                  # noqa: E402
import scipy.ndimage as ndi                         # noqa: E402
import torch                                        # noqa: E402
from nd_amd import kernels, synth                   # noqa: E402
from tests import rasterize_cases, rasterize_ref   # noqa: E402
from tests import zonal_ref as ref                 # noqa: E402

PEAK = 8.0e12                                       # HBM3E, bytes / s (datasheet)
STATS = ('count', 'nan_count', 'sum', 'min', 'max', 'm2')


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def min_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return [timed(fn) for _ in range(reps)]


def by_hand(planes, keys, n):
    """planes: k float32 tensors of npix elements each (views of either layout); float64 accumulators, n + 1 bins"""
    out = []
    cnt = torch.bincount(keys, minlength=n + 1).to(torch.float64)
    for x in planes:
        x = x.to(torch.float64)
        s = torch.zeros(n + 1, dtype=torch.float64, device=x.device).index_add_(0, keys, x)
        mean = s / cnt
        d = x - mean[keys]
        m2 = torch.zeros(n + 1, dtype=torch.float64, device=x.device).index_add_(0, keys, d * d)
        lo = torch.full((n + 1,), float('inf'), dtype=torch.float64, device=x.device).scatter_reduce_(0, keys, x, 'amin')
        hi = torch.full((n + 1,), float('-inf'), dtype=torch.float64, device=x.device).scatter_reduce_(0, keys, x, 'amax')
        out.append((s, m2, lo, hi))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'zonal_bench.json'))
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--dates', type=int, default=24)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--band', type=int, default=192)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_zonal needs a GPU')
    N, k, reps = args.size, args.dates, args.reps
    band = min(args.band, N)
    dev = torch.device('cuda:0')
    res = {'workload': 'zonal_stats %s of %d dates of %d x %d float32 gamma speckle with 1 %% NaN' % (STATS, k, N, N),
           'timing': 'min of %d calls after 2 warm-up calls, device events around kernels.zonal_stats; the index build '
                     '(kernels.zonal_index) on its own, min of 3' % reps,
           'traffic': '4 data bytes per zoned pixel and plane once, 4 index bytes per zoned pixel once per call, at %g '
                      'B/s' % PEAK, 'peak_bytes_per_s': PEAK, 'runs': []}

    # ---- the zone maps
    zone_maps = {}
    polys = rasterize_cases.parcels(np.random.default_rng(4096), max(1, int(10000 * (N / 4096.0) ** 2)), N, N)
    values = np.arange(1, len(polys) + 1)
    zone_maps['parcels'] = kernels.rasterize_polygons(*rasterize_ref.pack(polys), values, N, N)[0].contiguous()
    stack = synth.wishart_c2_stack(k, N, N, looks=9, device=dev)
    change = kernels.change_detection(stack[0], stack[1], stack[2], stack[3], alpha=0.99, n=9)      # (y, x, time)
    del stack
    one_date = change[:, :, k // 2].contiguous()
    del change
    torch.cuda.empty_cache()
    zone_maps['regions'] = kernels.label_regions(one_date, 4)[0]
    half = torch.zeros((N, N), dtype=torch.uint8, device=dev)
    half[:N // 2] = 1
    zone_maps['half'] = half

    # ---- the data, in both layouts
    gen = torch.Generator(device=dev)
    gen.manual_seed(2026)
    planar = torch.empty((k, N, N), dtype=torch.float32, device=dev)
    for t in range(k):
        u = torch.rand((4, N, N), generator=gen, device=dev).clamp_(min=1e-12)
        planar[t] = -torch.log(u).sum(0) * 0.25
        planar[t][torch.rand((N, N), generator=gen, device=dev) < 0.01] = float('nan')
        del u
    pixel = planar.permute(1, 2, 0).contiguous()                    # (y, x, time)
    layouts = (('(time, y, x)', planar, ('time', 'y', 'x')), ('(y, x, time)', pixel, ('y', 'x', 'time')))
    host2 = np.nan_to_num(planar[:2].cpu().numpy(), nan=0.0)

    for name, zones in zone_maps.items():
        # a band of rows against the restatement, both layouts
        zb = zones[:band].contiguous()
        ib = kernels.zonal_index(zb)
        want = ref.zonal_stats(planar[:, :band].cpu().numpy(), zb.cpu().numpy())[0]
        for tag, data, dims in layouts:
            sub = data[:, :band] if dims[0] == 'time' else data[:band]
            got = kernels.zonal_stats(sub, ib, dims=dims, stats=STATS)
            ref.same_stats({s: v.cpu().numpy() for s, v in got.items()}, want)
        del zb, ib, want

        build = min_ms(lambda: kernels.zonal_index(zones), 3, warm=1)
        index = kernels.zonal_index(zones)
        n = index.n
        sizes = (index.offsets[1:] - index.offsets[:-1])
        zoned = int(index.offsets[-1])
        floor_bytes = zoned * (4 * k + 4)
        keys64 = index.keys.reshape(-1).to(torch.int64)
        t0 = time.perf_counter()
        labels_host = zones.cpu().numpy()
        ids = np.arange(1, n + 1)
        for p in host2:
            ndi.mean(p, labels_host, ids)
            ndi.variance(p, labels_host, ids)
        scipy_s = time.perf_counter() - t0
        for tag, data, dims in layouts:
            first = kernels.zonal_stats(data, index, dims=dims, stats=STATS)
            again = kernels.zonal_stats(data, index, dims=dims, stats=STATS)
            for s in STATS:
                if first[s].cpu().numpy().tobytes() != again[s].cpu().numpy().tobytes():
                    raise SystemExit('%s %s: two runs differ in %s' % (name, tag, s))
            ms = min_ms(lambda: kernels.zonal_stats(data, index, dims=dims, stats=STATS), reps)
            views = ([data[t].reshape(-1) for t in range(k)] if dims[0] == 'time'
                     else [data[:, :, t].reshape(-1) for t in range(k)])
            if dims[0] == 'time':                   # (seconds a call: once per zone map, on the planar layout)
                hand = min_ms(lambda: by_hand(views, keys64, n), 1, warm=1)
            run = dict(name='%s, %s' % (name, tag), zones=n, zoned_pixels=zoned, layout=tag,
                       largest_zone=int(sizes.max()) if n else 0, median_zone=float(sizes.double().median()) if n else 0.0,
                       ms_min=min(ms), ms_all=ms, index_build_ms_min=min(build), index_build_ms_all=build,
                       traffic_bytes=floor_bytes, traffic_floor_ms=floor_bytes / PEAK * 1e3,
                       share_of_peak=floor_bytes / (min(ms) * 1e-3) / PEAK,
                       torch_by_hand_planar_ms=min(hand),
                       scipy_mean_variance_seconds_2_planes=scipy_s, scipy_mean_variance_seconds_all_planes=scipy_s * k / 2,
                       equal_to_restatement_on_a_band_of_rows=band, two_runs_identical=True)
            res['runs'].append(run)
            print(json.dumps(run), flush=True)
            del first, again, views
        del index, keys64
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
