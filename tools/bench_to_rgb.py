"""to_rgb timing: ms per call of nd_amd.visualize.to_rgb_stack (default channels C11, C22, C11 / C22) on a
device-resident k x n x n stack, per kernel (KernelTimer: rgb_limits = every selection pass, rgb_compose),
for float32 and float64, planar (time, y, x) and (y, x, time), exponential / constant / uniform planes.

    python tools/bench_to_rgb.py [--k 24] [--n 4096] [--reps 5] [--json out.json] [--dtypes float32,float64]

Beside every case, measured in the same run:
  floor_gb       the bytes the method has to move: R reads of C11 and C22 (R = 3 selection passes for
                 float32, 6 for float64, plus the compose read) and the composite written once
  read_ms        a plain read of C11 and C22 (torch sum of both), the yardstick of one selection pass: a
                 pass fetches exactly those bytes from HBM, the quotient channel's second read of both
                 planes is served by the cache (tools/prof_to_rgb.py under rocprofv3 --pmc FETCH_SIZE;
                 per-pass times come from the same tool under --kernel-trace)
  torch_ms       baseline (a): the same composite written with torch on the device (one sort per plane, both
                 ranks indexed from it, element-wise stretch), what a user would write without this
                 module; min of the same number of calls as the feature
  numpy_scaled_s baseline (b): tests/rgb_ref.py on ONE plane on the host, times the plane count (scaled,
                 not measured in full)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return min(out), sorted(out)[len(out) // 2]


def torch_limits(ch, ps):
    """np.nanpercentile's arithmetic for every p of `ps` from ONE full device sort (NaNs sort last)"""
    import torch
    v = torch.sort(ch.flatten()).values
    n = int((~torch.isnan(v)).sum().item())
    out = []
    for p in ps:
        if n == 0:
            out.append(ch.new_tensor(float('nan')))
            continue
        vi = ch.new_tensor(n - 1) * (ch.new_tensor(p) / ch.new_tensor(100))
        lo = min(int(torch.floor(vi).item()), n - 1)
        hi = min(lo + 1, n - 1)
        g = vi - lo
        d = v[hi] - v[lo]
        out.append(v[hi] - d * (1 - g) if g >= 0.5 else v[lo] + d * g)
    return out


def torch_composite(c11, c22, out):
    """baseline (a): sort per plane, index, element-wise stretch.  c11, c22: (time, y, x) views"""
    import torch
    for t in range(c11.shape[0]):
        for c, ch in enumerate((c11[t], c22[t], c11[t] / c22[t])):
            lo, hi = torch_limits(ch, (2, 98))
            if hi > lo:
                ch = (ch - lo) / (hi - lo) * 255
            out[t, :, :, c] = torch.nan_to_num(ch.double(), nan=0.0).clamp_(0, 255).to(torch.uint8)
    return out


def main():
    import numpy as np
    import torch
    from nd_amd import _lib, visualize, xr_lite
    from tests import rgb_ref
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=24)
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    k, n = a.k, a.n
    rows = []
    for dt in [getattr(torch, d) for d in a.dtypes.split(',')]:
        esz = torch.empty((), dtype=dt).element_size()
        reads = (3 if dt == torch.float32 else 6) + 1
        floor = (reads * 2 * k * n * n * esz + 3 * k * n * n) / 1e9
        for data in ('exponential', 'constant', 'uniform'):
            g = torch.Generator(device=dev).manual_seed(1)
            if data == 'exponential':
                c11 = torch.empty((k, n, n), dtype=dt, device=dev).exponential_(1.0, generator=g)
                c22 = torch.empty((k, n, n), dtype=dt, device=dev).exponential_(2.0, generator=g)
            elif data == 'constant':
                c11 = torch.full((k, n, n), 0.75, dtype=dt, device=dev)
                c22 = torch.full((k, n, n), 0.5, dtype=dt, device=dev)
            else:
                c11 = torch.rand((k, n, n), dtype=dt, device=dev, generator=g)
                c22 = torch.rand((k, n, n), dtype=dt, device=dev, generator=g) + 0.5
            host_s = None
            if data == 'exponential':
                plane = c11[0].cpu().numpy()
                t0 = time.perf_counter()
                rgb_ref.composite([plane])
                host_s = (time.perf_counter() - t0) * 3 * k
            frames = None
            for layout in ('planar', 'pixel_major'):
                dims = ('time', 'y', 'x') if layout == 'planar' else ('y', 'x', 'time')
                v11 = c11 if layout == 'planar' else c11.permute(1, 2, 0).contiguous()
                v22 = c22 if layout == 'planar' else c22.permute(1, 2, 0).contiguous()
                ds = xr_lite.Dataset()
                ds['C11'] = (dims, v11)
                ds['C22'] = (dims, v22)
                ms = timed(lambda: visualize.to_rgb_stack(ds), a.reps)
                _lib.timing_enable(16)
                got = visualize.to_rgb_stack(ds)
                per = dict(_lib.timing_collect())
                _lib.timing_enable(0)
                read = timed(lambda: (v11.sum(), v22.sum()), a.reps)
                p11 = v11 if layout == 'planar' else v11.permute(2, 0, 1)
                p22 = v22 if layout == 'planar' else v22.permute(2, 0, 1)
                out = torch.empty((k, n, n, 3), dtype=torch.uint8, device=dev)
                base = timed(lambda: torch_composite(p11, p22, out), a.reps)
                if frames is None:
                    frames = got
                row = dict(dtype=str(dt)[6:], layout=layout, data=data, ms_min=ms[0], ms_median=ms[1],
                           limits_ms=per.get('rgb_limits'), compose_ms=per.get('rgb_compose'),
                           floor_gb=floor, floor_tb_per_s=floor / ms[0], peak_fraction=floor / ms[0] / 8.0,
                           read_ms=read[0], limits_over_read=per.get('rgb_limits') / read[0] / (reads - 1),
                           torch_ms=base[0], speedup_over_torch=base[0] / ms[0],
                           same_bytes_as_planar=bool(torch.equal(got, frames)),
                           torch_agrees=float((out == got).float().mean().item()))
                if host_s is not None:
                    row['numpy_scaled_s'] = host_s
                rows.append(row)
                print(json.dumps(row), flush=True)
                del v11, v22, ds, got, out, p11, p22
            del c11, c22, frames
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(dict(k=k, n=n, rows=rows), open(a.json, 'w'), indent=1)


if __name__ == '__main__':
    main()
