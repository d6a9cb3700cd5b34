"""Secondary measurement: change_segments (direction of change and segment means) on a 24 x 4096 x 4096 float32
dual-pol stack on the device, with the map of the omnibus test at alpha = 0.99 (few changes) and at
alpha = 0.01 (the dense map) -- direction only, means only and both, next to a plain device-side torch
version of the same definition in the same process (a loop over the dates with torch.where, float64
accumulators, the backward carry for the means), whose outputs are asserted equal to the kernel's before
anything is timed.  Each figure is the minimum over the timed calls after 2 warm-up calls, every call timed
with device events; kernel and torch calls alternate.  The floor a figure is a share of is the definition's own
traffic: reads P k sizeof(T) + k, writes k (direction) and P k sizeof(T) (means) bytes per pixel, over the
datasheet's HBM rate.  Writes profiles/change_segments_bench.json (or the path given) and prints it.

    python tools/bench_change_segments.py [--out PATH] [--size NY NX] [--reps N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                        # noqa: E402
from nd_amd import kernels, synth                   # noqa: E402

PEAK = 8.0e12                                       # HBM3E, bytes / s (datasheet)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_version(planes, change, direction=True, means=True):
    """The definition with torch on the device, C2 structure: planes four (k, ny, nx) tensors, change uint8
    (ny, nx, k).  Returns what kernels.change_segments returns."""
    k = planes[0].shape[0]
    T = planes[0].dtype
    opens = (change != 0).permute(2, 0, 1).contiguous()                     # (k, ny, nx)
    s = [torch.zeros(planes[0].shape[1:], dtype=torch.float64, device=planes[0].device) for _ in planes]
    m = torch.zeros_like(s[0])
    zero = torch.zeros_like(m)
    out_d = torch.zeros(opens.shape, dtype=torch.int8, device=opens.device) if direction else None
    out_m = [torch.empty_like(p) for p in planes] if means else None
    c1, c2, c3 = (torch.full(m.shape, v, dtype=torch.int8, device=m.device) for v in (1, 2, 3))
    for t in range(k):
        x = [p[t].double() for p in planes]
        if t >= 1:
            f = opens[t]
            if direction:
                d = [xp - sp / m for xp, sp in zip(x, s)]
                det = (d[0] * d[3]) - ((d[1] * d[1]) + (d[2] * d[2]))
                code = torch.where((d[0] > 0) & (det > 0), c1, torch.where((d[0] < 0) & (det > 0), c2, c3))
                out_d[t] = torch.where(f, code, torch.zeros_like(code))
            s = [torch.where(f, zero, sp) for sp in s]
            m = torch.where(f, zero, m)
        s = [sp + xp for sp, xp in zip(s, x)]
        m = m + 1.0
        if means:
            for p in range(len(planes)):
                out_m[p][t] = (s[p] / m).to(T)                               # the running mean ...
    if means:
        for t in range(k - 2, -1, -1):                                       # ... carried back from each segment's end
            for p in range(len(planes)):
                out_m[p][t] = torch.where(opens[t + 1], out_m[p][t], out_m[p][t + 1])
    if direction:
        out_d = out_d.permute(1, 2, 0).contiguous()
    return (out_d, out_m) if (direction and means) else (out_d if direction else out_m)


def same(a, b):
    if torch.is_tensor(a):
        return bool(torch.equal(a, b))
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'change_segments_bench.json'))
    ap.add_argument('--size', type=int, nargs=2, default=(4096, 4096))
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_change_segments needs a GPU')
    k, (ny, nx) = 24, args.size
    dev = torch.device('cuda:0')
    st = synth.wishart_c2_stack(k, ny, nx, looks=9, seed=11, device=dev)
    planes = list(st)
    P, esz = 4, 4
    npix = ny * nx
    floor = {'direction': npix * (P * k * esz + k + k), 'means': npix * (P * k * esz + k + P * k * esz),
             'both': npix * (P * k * esz + k + k + P * k * esz)}
    want = {'direction': (True, False), 'means': (False, True), 'both': (True, True)}
    res = {'workload': 'change_segments, c2, %dt x %d x %d float32 on the device' % (k, ny, nx),
           'timing': 'min of %d calls after 2 warm-up calls, device events; kernel and torch calls alternate' % args.reps,
           'baseline': 'device-side torch loop over the dates (this script, torch_version)',
           'floor': 'bytes the definition moves per call / %g B/s' % PEAK, 'peak_bytes_per_s': PEAK, 'runs': []}
    for alpha in (0.99, 0.01):
        change = kernels.change_detection(planes[0], planes[1], planes[2], planes[3], alpha=alpha, n=9)
        per_pixel = float(change[..., 1:].sum().item()) / npix
        for out, (direction, means) in want.items():
            hip = lambda: kernels.change_segments(planes, change, 'c2', direction=direction, means=means)   # noqa: E731
            tor = lambda: torch_version(planes, change, direction=direction, means=means)                  # noqa: E731
            if not same(hip(), tor()):
                raise SystemExit('alpha %g, %s: the kernel and the torch version differ' % (alpha, out))
            for _ in range(2):
                hip()
                tor()
            torch.cuda.synchronize()
            ms = {'hip': [], 'torch': []}
            for _ in range(args.reps):
                ms['hip'].append(timed(hip)[0])
                ms['torch'].append(timed(tor)[0])
            best = min(ms['hip'])
            res['runs'].append({'alpha': alpha, 'outputs': out, 'changes_per_pixel': per_pixel,
                                'ms_min': best, 'ms_all': ms['hip'],
                                'torch_ms_min': min(ms['torch']), 'torch_ms_all': ms['torch'],
                                'torch_over_kernel': min(ms['torch']) / best, 'equal_outputs': True,
                                'floor_bytes': floor[out], 'floor_ms': floor[out] / PEAK * 1e3,
                                'floor_bytes_per_s': floor[out] / (best * 1e-3),
                                'share_of_peak': floor[out] / (best * 1e-3) / PEAK})
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
