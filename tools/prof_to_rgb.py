"""The workload of a rocprofv3 run over to_rgb_stack: the k x n x n float32 / float64 planar stack of
tools/bench_to_rgb.py (default channels C11, C22, C11 / C22), one warm-up call and `--calls` calls.

    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/prof_to_rgb.py
    rocprofv3 --kernel-trace --pmc FETCH_SIZE --kernel-include-regex rgb_ -d DIR -o p --output-format csv -- \\
        python tools/prof_to_rgb.py --calls 1            (counters in a run of their own; WRITE_SIZE likewise)

tools/summarize_to_rgb_prof.py turns the csv files into per-kernel milliseconds and bytes.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from nd_amd import visualize, xr_lite
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=24)
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--dtype', default='float32')
    ap.add_argument('--data', default='exponential', choices=('exponential', 'constant'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    dt = getattr(torch, a.dtype)
    shape = (a.k, a.n, a.n)
    if a.data == 'exponential':
        g = torch.Generator(device=dev).manual_seed(1)
        c11 = torch.empty(shape, dtype=dt, device=dev).exponential_(1.0, generator=g)
        c22 = torch.empty(shape, dtype=dt, device=dev).exponential_(2.0, generator=g)
    else:
        c11 = torch.full(shape, 0.75, dtype=dt, device=dev)
        c22 = torch.full(shape, 0.5, dtype=dt, device=dev)
    ds = xr_lite.Dataset()
    ds['C11'] = (('time', 'y', 'x'), c11)
    ds['C22'] = (('time', 'y', 'x'), c22)
    for _ in range(a.calls + 1):
        visualize.to_rgb_stack(ds)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
