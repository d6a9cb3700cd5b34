"""Coregistration timing: ms per call of nd_amd_coregister_shifts and nd_amd_warp_translate on a
device-resident 24 x 4096 x 4096 stack of 4 variables, float32 and float64, both layouts, and of
the whole Coregistration.apply (float32, planar).  Plans and code objects are warmed up first.

    python tools/bench_coregister.py [--k 24] [--n 4096] [--reps 5] [--json out.json]

Bytes per warp call (the roofline figure): read + write of every plane once, 2 x 4 x k x n^2 x itemsize
(the min / max pass reads the planes once more: 3 passes in all).
"""
import argparse
import json
import os
import sys

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


def main():
    import torch
    from nd_amd import kernels, xr_lite
    from nd_amd.warp import Coregistration
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=24)
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    k, n = a.k, a.n
    rows = []
    for dt in (torch.float32, torch.float64):
        g = torch.Generator(device=dev).manual_seed(1)
        base = torch.rand((n // 64, n // 64), device=dev, generator=g, dtype=dt)
        base = torch.nn.functional.interpolate(base[None, None], size=(n, n), mode='bilinear')[0, 0]
        planar = []
        for v in range(4):
            st = torch.stack([torch.roll(base, (t % 7 - 3, t % 5 - 2), (0, 1)) for t in range(k)])
            planar.append((st + 0.05 * torch.rand((k, n, n), device=dev, generator=g, dtype=dt) + 1.0).contiguous())
            del st
        esz = planar[0].element_size()
        for layout in ('planar', 'pixel_major'):
            vs = planar if layout == 'planar' else [p.permute(1, 2, 0).contiguous() for p in planar]
            c11 = vs[0]
            dims = ('time', 'y', 'x') if layout == 'planar' else ('y', 'x', 'time')
            for u in (10, 50):
                ms = timed(lambda: kernels.coregister_shifts(c11, 0, u, dims=dims), a.reps)
                rows.append(dict(step='shifts', dtype=str(dt)[6:], layout=layout, upsampling=u,
                                 ms_min=ms[0], ms_median=ms[1]))
            sh, _ = kernels.coregister_shifts(c11, 0, 10, dims=dims)
            ms = timed(lambda: kernels.warp_translate(vs, sh, 0, layout), a.reps)
            nbytes = 2 * 4 * k * n * n * esz
            rows.append(dict(step='warp', dtype=str(dt)[6:], layout=layout, ms_min=ms[0], ms_median=ms[1],
                             read_write_gb=nbytes / 1e9, tb_per_s=nbytes / (ms[0] * 1e-3) / 1e12))
            if layout != 'planar':
                del vs
        if dt == torch.float32:
            ds = xr_lite.Dataset()
            for name, p in zip(('C11', 'C12__re', 'C12__im', 'C22'), planar):
                ds[name] = (('time', 'y', 'x'), p)
            ms = timed(lambda: Coregistration(upsampling=10).apply(ds), a.reps)
            rows.append(dict(step='apply', dtype='float32', layout='planar', upsampling=10,
                             ms_min=ms[0], ms_median=ms[1]))
        del planar
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    if a.json:
        json.dump(dict(k=k, n=n, rows=rows), open(a.json, 'w'), indent=1)


if __name__ == '__main__':
    main()
