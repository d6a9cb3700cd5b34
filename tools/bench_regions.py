"""Secondary measurement: kernels.label_regions and kernels.sieve_regions on the change map of the headline workload
-- OmnibusTest on the synthetic dual-pol stack of 24 dates of 4096 x 4096, a uint8 map of 24 planes --

    at alpha = 0.99 (sparse) and alpha = 0.01 (dense)
    in (time, y, x) memory and in (y, x, time) memory, which is how the omnibus kernels leave it, read and written
    where it lies
    and on one 4096 x 4096 noise mask of density 0.59, the site-percolation threshold at 4: the longest regions

For each it times label_regions at connectivity 4 and 8 and sieve_regions(min_size=4): the minimum of 7 calls, device
events around the kernels.* call, after 2 warm-up calls.  Next to each figure: a plain device copy of the same bytes
(the map and an int32 plane per pixel for the labels, the map twice for the sieve), the definition's own traffic at
8 TB/s (1 byte read and 4 written per pixel; the map read and written), and scipy.ndimage.label on the host for the
same planes with the transfer of the map counted separately.  Before timing, two whole planes of every map are compared
with scipy.ndimage.label and must be equal.
Writes profiles/regions_bench.json (or the path given) and prints it.

    python tools/bench_regions.py [--out PATH] [--size N] [--dates K] [--reps N]
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
from tests import regions_ref as ref               # noqa: E402

PEAK = 8.0e12                                       # HBM3E, bytes / s (datasheet)
MIN_SIZE = 4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def min_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return [timed(fn) for _ in range(reps)]


def check_planes(name, planar, dims_map, dims, picks):
    """whole planes `picks` of the map against scipy.ndimage.label, both connectivities, and the sieve"""
    for conn in (4, 8):
        labels, counts = kernels.label_regions(dims_map, conn, dims=dims)
        sieved = kernels.sieve_regions(dims_map, MIN_SIZE, conn, dims=dims)
        at = dims.index('time')
        for p in picks:
            host = planar[p].cpu().numpy()
            want, n = ndi.label(host != 0, ref.structure(conn), output=np.int32)
            got = labels.select(at, p).cpu().numpy()
            if int(counts[p]) != n or not np.array_equal(got, want):
                raise SystemExit('%s: plane %d at connectivity %d differs from scipy.ndimage.label' % (name, p, conn))
            if not np.array_equal(sieved.select(at, p).cpu().numpy(), ref.sieve(host, MIN_SIZE, conn)):
                raise SystemExit('%s: plane %d at connectivity %d: the sieve differs' % (name, p, conn))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'regions_bench.json'))
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--dates', type=int, default=24)
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_regions needs a GPU')
    N, k, reps = args.size, args.dates, args.reps
    dev = torch.device('cuda:0')
    res = {'workload': 'regions of the uint8 change map of OmnibusTest (n = 9) on the synthetic dual-pol stack of %d '
                       'dates of %d x %d, and of one %d x %d noise mask of density 0.59' % (k, N, N, N, N),
           'timing': 'min of %d calls after 2 warm-up calls, device events around the kernels.* call; the calls wait '
                     'for the device themselves (the give-up word)' % reps,
           'traffic': 'labels: 1 byte read and 4 written per pixel; sieve: the map read and written; at %g B/s' % PEAK,
           'workspace_cap_bytes': kernels.REGIONS_WORKSPACE_CAP, 'peak_bytes_per_s': PEAK, 'runs': [], 'host': []}

    stack = synth.wishart_c2_stack(k, N, N, looks=9, device=dev)
    maps = {}
    for alpha in (0.99, 0.01):
        maps[alpha] = kernels.change_detection(stack[0], stack[1], stack[2], stack[3], alpha=alpha, n=9)
    del stack
    torch.cuda.empty_cache()
    gen = torch.Generator(device=dev)
    gen.manual_seed(59)
    noise = (torch.rand((1, N, N), generator=gen, device=dev) < 0.59).to(torch.uint8)

    def record(name, fn, nbytes, copy_fn, **extra):
        ms = min_ms(fn, reps)
        copy = min(min_ms(copy_fn, reps))
        run = dict(name=name, ms_min=min(ms), ms_all=ms, device_copy_ms=copy, traffic_bytes=nbytes,
                   traffic_floor_ms=nbytes / PEAK * 1e3, share_of_peak=nbytes / (min(ms) * 1e-3) / PEAK,
                   equal_to_scipy_on_two_planes=True, **extra)
        res['runs'].append(run)
        print(json.dumps(run), flush=True)

    def bench_map(name, m, dims, planar, **extra):
        npx = m.numel()
        labels = kernels.label_regions(m, 4, dims=dims)[0]
        labels2 = torch.empty_like(labels)
        out = torch.empty_like(m)

        def copy_labels():
            out.copy_(m)
            labels2.copy_(labels)

        for conn in (4, 8):
            record('%s: label_regions, connectivity %d' % (name, conn),
                   lambda conn=conn: kernels.label_regions(m, conn, dims=dims, labels=labels), 5 * npx, copy_labels,
                   connectivity=conn, regions=int(kernels.label_regions(m, conn, dims=dims)[1].sum()),
                   foreground=float((m != 0).float().mean()), **extra)
        record('%s: sieve_regions(min_size=%d), connectivity 4' % (name, MIN_SIZE),
               lambda: kernels.sieve_regions(m, MIN_SIZE, 4, dims=dims, out=out), 2 * npx, lambda: out.copy_(m),
               connectivity=4, **extra)
        del labels, labels2, out
        torch.cuda.empty_cache()

    def bench_host(name, planar):
        t0 = time.perf_counter()
        host = planar.cpu().numpy()
        transfer = time.perf_counter() - t0
        for conn in (4, 8):
            t0 = time.perf_counter()
            n = sum(ndi.label(p != 0, ref.structure(conn), output=np.int32)[1] for p in host)
            res['host'].append({'name': '%s: scipy.ndimage.label on the host, connectivity %d' % (name, conn),
                                'seconds': time.perf_counter() - t0, 'planes': len(host), 'regions': int(n),
                                'download_of_the_map_seconds': transfer})
            print(json.dumps(res['host'][-1]), flush=True)

    for alpha, pm in maps.items():
        planar = pm.permute(2, 0, 1).contiguous()
        tag = 'alpha = %g' % alpha
        check_planes(tag + ' (time, y, x)', planar, planar, ('time', 'y', 'x'), (0, k - 1))
        check_planes(tag + ' (y, x, time)', planar, pm, ('y', 'x', 'time'), (0, k - 1))
        bench_map(tag + ', (time, y, x)', planar, ('time', 'y', 'x'), planar, alpha=alpha, layout='(time, y, x)')
        bench_map(tag + ', (y, x, time) where it lies', pm, ('y', 'x', 'time'), planar, alpha=alpha,
                  layout='(y, x, time)')
        bench_host(tag, planar)
        del planar
    maps.clear()
    torch.cuda.empty_cache()
    check_planes('noise 0.59', noise, noise, ('time', 'y', 'x'), (0,))
    bench_map('noise mask of density 0.59, one plane', noise, ('time', 'y', 'x'), noise, layout='(time, y, x)')
    bench_host('noise mask of density 0.59, one plane', noise)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
