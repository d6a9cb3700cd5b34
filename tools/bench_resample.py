"""Secondary measurement: kernels.resample on a 24-date stack of 4096 x 4096 float32 on the device, planar
(time, y, x) and pixel-major (y, x, time), the tables already on the device --

    average / 2, average / 2.5, cubic / 2.5        down-sampling (spatial multilooking with decimation)
    bilinear x 2 (from 24 x 2048^2)                up-sampling
    bilinear at equal size, half a pixel shifted
    nearest x 2 on one uint8 map (from 2048^2)

Each line reports the minimum of 7 calls (device events around kernels.resample, after 2 warm-up calls) and the share
of 8 TB/s that the definition's own traffic reaches at that time: the source bytes that lie under any tap, once, plus
the bytes written.  Before timing, a band of output rows of the first and last plane is compared with
tests/resample_ref.py and must be equal.  For scale, on the same device: F.interpolate(mode='bilinear',
antialias=True) and F.avg_pool2d on the same planar stacks, and a plain copy of the larger side of each workload.
Writes profiles/resample_bench.json (or the path given) and prints it.

    python tools/bench_resample.py [--out PATH] [--size N] [--dates K] [--reps N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                  # noqa: E402
import torch                                        # noqa: E402
import torch.nn.functional as F                     # noqa: E402
from nd_amd import kernels                          # noqa: E402
from tests import resample_cases as cases          # noqa: E402
from tests import resample_ref as ref              # noqa: E402

PEAK = 8.0e12                                       # HBM3E, bytes / s (datasheet)
BAND = 6                                            # output rows compared with the restatement


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def min_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return [timed(fn)[0] for _ in range(reps)]


def covered(table):
    """source samples that lie under any tap of the axis"""
    hit = np.zeros(table.n + 1, np.int64)
    live = table.count > 0
    np.add.at(hit, table.start[live], 1)
    np.add.at(hit, (table.start + table.count)[live], -1)
    return int((np.cumsum(hit)[:-1] > 0).sum())


def check_band(name, planar, out_planar, ty, tx, nearest):
    """BAND output rows from the middle of the first and the last plane against the restatement"""
    i0 = ty.m // 2
    rows = slice(i0, min(ty.m, i0 + BAND))
    sy, cy, wy = ty.start[rows], ty.count[rows], ty.weights[:, rows]
    live = cy > 0
    r0 = int(sy[live].min()) if live.any() else 0
    r1 = int((sy + cy)[live].max()) if live.any() else 1
    src = planar[[0, -1], r0:r1].cpu().numpy()
    want = ref.resample(src, (np.where(live, sy - r0, 0).astype(np.int32), cy, wy), (tx.start, tx.count, tx.weights),
                        nearest=nearest)
    got = out_planar[[0, -1], rows].cpu().numpy()
    try:
        cases.assert_same(got, want, payloads=nearest)
    except AssertionError as e:
        raise SystemExit('%s: the kernel differs from the restatement on output rows %d..%d: %s'
                         % (name, rows.start, rows.stop, e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_bench.json'))
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--dates', type=int, default=24)
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample needs a GPU')
    N, k = args.size, args.dates
    dev = torch.device('cuda:0')
    torch.manual_seed(4096)
    res = {'workload': 'kernels.resample, %d dates of %d x %d float32 (nearest: one uint8 map), tables on the device'
                       % (k, N, N),
           'timing': 'min of %d calls after 2 warm-up calls, device events' % args.reps,
           'traffic': 'source bytes under any tap, once, plus the bytes written; share of %g B/s' % PEAK,
           'peak_bytes_per_s': PEAK, 'runs': [], 'for_scale': []}
    # (name, method, source side, output side, shift in source pixels, dtype, planes)
    work = [('average / 2', 'average', N, N // 2, 0.0, torch.float32, k),
            ('average / 2.5', 'average', N, int(N / 2.5), 0.0, torch.float32, k),
            ('cubic / 2.5', 'cubic', N, int(N / 2.5), 0.0, torch.float32, k),
            ('bilinear x 2', 'bilinear', N // 2, N, 0.0, torch.float32, k),
            ('bilinear, half a pixel shifted', 'bilinear', N, N, 0.5, torch.float32, k),
            ('nearest x 2, uint8', 'nearest', N // 2, N, 0.0, torch.uint8, 1)]
    for name, method, n, m, shift, dtype, planes in work:
        ratio = {'average / 2.5': 2.5, 'cubic / 2.5': 2.5}.get(name, n / m)
        if dtype == torch.uint8:
            planar = torch.randint(0, 256, (planes, n, n), dtype=dtype, device=dev)
        else:
            planar = torch.empty((planes, n, n), dtype=dtype, device=dev).exponential_()
        ty = kernels.resample_axis(n, m, (-1.0, 0.0), (-ratio, -shift), method)
        tx = kernels.resample_axis(n, m, (1.0, 0.0), (ratio, shift), method)
        dty, dtx = ty.to(dev), tx.to(dev)
        item = planar.element_size()
        traffic = planes * item * (covered(ty) * covered(tx) + m * m)
        run = {'name': name, 'method': method, 'source': [planes, n, n], 'output': [planes, m, m],
               'taps': [ty.taps, tx.taps], 'traffic_bytes': traffic, 'traffic_floor_ms': traffic / PEAK * 1e3}
        for layout, dims in (('planar', ('time', 'y', 'x')), ('pixel_major', ('y', 'x', 'time'))):
            src = planar if layout == 'planar' else planar.permute(1, 2, 0).contiguous()
            shape = (planes, m, m) if layout == 'planar' else (m, m, planes)
            out = torch.empty(shape, dtype=dtype, device=dev)
            call = lambda: kernels.resample(src, dty, dtx, dims=dims, out=out)          # noqa: E731
            first = call().clone()
            if not torch.equal(first.view(torch.uint8), call().view(torch.uint8)):
                raise SystemExit('%s %s: two runs differ' % (name, layout))
            check_band('%s %s' % (name, layout), planar, first if layout == 'planar' else first.permute(2, 0, 1),
                       ty, tx, method == 'nearest')
            del first
            ms = min_ms(call, args.reps)
            run[layout] = {'ms_min': min(ms), 'ms_all': ms, 'share_of_peak': traffic / (min(ms) * 1e-3) / PEAK,
                           'equal_to_restatement_on_band': True}
            del src, out
        # a plain copy of the larger side, for scale
        big = planar if n >= m else torch.empty((planes, m, m), dtype=dtype, device=dev)
        dst = torch.empty_like(big)
        ms = min_ms(lambda: dst.copy_(big), args.reps)
        run['copy_of_larger_side_ms_min'] = min(ms)
        run['copy_of_larger_side_bytes'] = 2 * big.numel() * item
        del big, dst
        if name == 'average / 2':
            ms = min_ms(lambda: F.avg_pool2d(planar[None], 2), args.reps)
            res['for_scale'].append({'name': 'F.avg_pool2d(2) on the planar stack', 'ms_min': min(ms), 'ms_all': ms})
        if name in ('average / 2.5', 'bilinear x 2', 'bilinear, half a pixel shifted'):
            ms = min_ms(lambda: F.interpolate(planar[None], size=(m, m), mode='bilinear', antialias=True,
                                              align_corners=False), args.reps)
            res['for_scale'].append({'name': "F.interpolate(mode='bilinear', antialias=True), %d^2 -> %d^2, planar"
                                             % (n, m), 'ms_min': min(ms), 'ms_all': ms})
        res['runs'].append(run)
        del planar
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
