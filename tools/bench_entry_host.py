#!/usr/bin/env python
"""tools/bench_entry_host.py -- host time per call of the change-detection entries.  Needs a GPU.

    [ND_AMD_LIB=/path/to/libnd_amd.so] python tools/bench_entry_host.py [--calls 2000] [--warmup 50]

One run: for change_detection at alpha = 0.01 and 0.99, change_detection_c3, change_detection_diag and
change_segments, `--calls` calls back to back on a raster small enough that a call is bound by the host (64 x 128
pixels, 8 dates, float32), timed with a host clock that ends in a synchronise.  Prints one JSON line, microseconds
per call.  Two builds are compared by alternating runs of this script, one process each, with ND_AMD_LIB naming
the library (profiles/omnibus_entry_bench.json).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch                                    # noqa: E402
from nd_amd import _lib, kernels                # noqa: E402

NY, NX, K, LOOKS = 64, 128, 8, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=50)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(7)
    # intensities of LOOKS looks around 1 with a step in a tenth of the pixels; small off-diagonal terms keep the
    # 2 x 2 and 3 x 3 matrices positive definite
    diag = [torch.empty((K, NY, NX), device=dev).exponential_(1.0, generator=g) / 4 + 0.75 for _ in range(3)]
    step = (torch.rand((NY, NX), device=dev, generator=g) < 0.1).float() * 3 + 1
    for d in diag:
        d[K // 2:] *= step
    off = [(torch.rand((K, NY, NX), device=dev, generator=g) - 0.5) * 0.1 for _ in range(6)]
    c2 = (diag[0], off[0], off[1], diag[1])
    c3 = diag + off
    change = kernels.change_detection(*c2, alpha=0.01, n=LOOKS)
    lines = {
        'change_detection_alpha_0.01': lambda: kernels.change_detection(*c2, alpha=0.01, n=LOOKS),
        'change_detection_alpha_0.99': lambda: kernels.change_detection(*c2, alpha=0.99, n=LOOKS),
        'change_detection_c3': lambda: kernels.change_detection_c3(c3, alpha=0.01, n=LOOKS),
        'change_detection_diag': lambda: kernels.change_detection_diag(diag[:2], alpha=0.01, n=LOOKS),
        'change_segments': lambda: kernels.change_segments(c2, change, 'c2'),
    }
    out = {'lib': os.path.abspath(_lib.LIB_PATH), 'calls': a.calls}
    for name, f in lines.items():
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            f()
        torch.cuda.synchronize(dev)
        out[name] = round((time.perf_counter() - t0) / a.calls * 1e6, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
