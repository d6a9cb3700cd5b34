"""Secondary measurement: kernels.rasterize_polygons on a 4096 x 4096 raster on the device, two workloads --

  parcels   10 000 random parcels of 4 to 12 vertices scattered over the raster
  ring      one 20 000-vertex ring spanning the raster (a lobed outline, a few dozen crossings a row at most)

Each line reports the whole call (owner clear, fill, resolve: device events around rasterize_polygons with the
polygon table already on the device, int64 values), the host's share that precedes it (boxes, prefix sums and the
upload: PolygonTable, wall clock), and the owner-clear plus resolve passes alone -- the same call with zero
polygons -- as the floor that pure memory traffic sets (4 bytes cleared + 4 read + 8 written per pixel).  Each
figure is the minimum over the timed calls after 2 warm-up calls.  Before anything is timed the kernel is compared
with tests/rasterize_ref.py on a 256 x 256 version of the workload, and two runs of the full size must give the
same bytes.  Writes profiles/rasterize_bench.json (or the path given) and prints it.

    python tools/bench_rasterize.py [--out PATH] [--size NY NX] [--reps N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                  # noqa: E402
import torch                                        # noqa: E402
from nd_amd import kernels                          # noqa: E402
from tests import rasterize_cases as cases         # noqa: E402
from tests import rasterize_ref as ref             # noqa: E402

PEAK = 8.0e12                                       # HBM3E, bytes / s (datasheet)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def lobed_ring(m, ny, nx):
    th = 2 * np.pi * np.arange(m) / m
    r = 0.75 + 0.2 * np.sin(5 * th) + 0.04 * np.sin(23 * th + 0.3)
    return [np.stack([nx / 2 + 0.499 * nx * r * np.cos(th), ny / 2 + 0.499 * ny * r * np.sin(th)], axis=1)]


def workload(name, ny, nx, scale=1.0):
    rng = np.random.default_rng(4096)
    if name == 'parcels':
        return cases.parcels(rng, max(1, int(10000 * scale * scale)), ny, nx)
    return [lobed_ring(max(3, int(20000 * scale)), ny, nx)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rasterize_bench.json'))
    ap.add_argument('--size', type=int, nargs=2, default=(4096, 4096))
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rasterize needs a GPU')
    ny, nx = args.size
    dev = torch.device('cuda:0')
    floor_bytes = ny * nx * (4 + 4 + 8)
    res = {'workload': 'rasterize_polygons, int64 values, one layer, %d x %d on the device' % (ny, nx),
           'timing': 'min of %d calls after 2 warm-up calls, device events' % args.reps,
           'floor': 'owner clear + resolve alone (the call with zero polygons); bytes: 4 cleared + 4 read + 8 written '
                    'per pixel over %g B/s' % PEAK, 'peak_bytes_per_s': PEAK, 'runs': []}
    empty = (np.zeros((0, 2)), np.zeros(1, np.int64), np.zeros(1, np.int64))
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    out = torch.empty((1, ny, nx), dtype=torch.int64, device=dev)
    for name in ('parcels', 'ring'):
        small = workload(name, 256, 256, scale=256.0 / max(ny, nx))
        v = np.arange(1, len(small) + 1)
        got = kernels.rasterize_polygons(*ref.pack(small), v, 256, 256).cpu().numpy()
        if got.tobytes() != ref.burn(small, v, 256, 256).tobytes():
            raise SystemExit('%s: the kernel differs from the restatement on the 256 x 256 version' % name)
        polys = workload(name, ny, nx)
        packed = ref.pack(polys)
        t0 = time.perf_counter()
        table = kernels.PolygonTable(*packed, ny, nx, device=dev)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        values = torch.arange(1, len(polys) + 1, dtype=torch.int64, device=dev)
        full = lambda: kernels.rasterize_polygons(table, None, None, values, ny, nx, out=out)      # noqa: E731
        bare = lambda: kernels.rasterize_polygons(*empty, none, ny, nx, out=out)                   # noqa: E731
        first = full().clone()
        if not torch.equal(first, full()):
            raise SystemExit('%s: two runs differ' % name)
        covered = float((first != 0).double().mean().item())
        for _ in range(2):
            full()
            bare()
        torch.cuda.synchronize()
        ms = {'full': [], 'bare': []}
        for _ in range(args.reps):
            ms['full'].append(timed(full)[0])
            ms['bare'].append(timed(bare)[0])
        res['runs'].append({'name': name, 'polygons': len(polys), 'vertices': int(packed[0].shape[0]),
                            'rows_of_work': table.items, 'covered_share': covered,
                            'ms_min': min(ms['full']), 'ms_all': ms['full'],
                            'clear_resolve_ms_min': min(ms['bare']), 'clear_resolve_ms_all': ms['bare'],
                            'host_table_ms': host_ms, 'equal_to_restatement_at_256': True,
                            'floor_bytes': floor_bytes, 'floor_ms': floor_bytes / PEAK * 1e3})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
