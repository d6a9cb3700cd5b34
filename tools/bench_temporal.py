"""Secondary measurement: kernels.temporal_stats on 4096 x 4096 float32 gamma speckle with 1 % NaN, in (time, y, x)
memory and in (y, x, time) memory, for 24 and 48 dates (the register form) and 100 dates (the LDS form; the moments alone
go through the streaming form there in (time, y, x) memory).  Four requests:

    mean_std      mean + std
    median        the median
    p2_p98        percentiles 2 and 98
    all           every statistic of kernels.TEMPORAL_STATS and both percentiles

For each: the minimum of 7 calls, device events around the kernels.* call, after 2 warm-up calls.  Next to each figure:

    the traffic floor: one read of the stack plus the outputs at the datasheet's 8 TB/s
    what a user would write in torch on the same device, minimum of 3 calls after one warm-up: torch.sort along the
        series plus gathers at the ranks for the order statistics (NaN sorts last, as here), nanmean and elementwise
        operations in the data's type for the moments, amin / amax / argmax over NaN-masked copies

Before timing, a band of rows is compared with the restatement (tests/temporal_ref.py): float64 outputs bit for bit,
order statistics by ==.  No time is fixed in advance.  Writes profiles/temporal_bench.json (or the path given) and
prints it.

    python tools/bench_temporal.py [--out PATH] [--size N] [--dates K K K] [--reps N] [--band ROWS]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                  # noqa: E402
import torch                                        # noqa: E402
from nd_amd import kernels                          # noqa: E402
from tests import temporal_ref as ref              # noqa: E402

PEAK = 8.0e12                                       # HBM3E, bytes / s (datasheet)
REQUESTS = (('mean_std', ('mean', 'std'), ()), ('median', ('median',), ()), ('p2_p98', (), (2.0, 98.0)),
            ('all', kernels.TEMPORAL_STATS, (2.0, 98.0)))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def min_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return min(timed(fn) for _ in range(reps))


def speckle(k, n, layout, dev):
    """gamma speckle of 4 looks (the sum of four exponentials) with 1 % NaN, made on the device"""
    gen = torch.Generator(device=dev).manual_seed(20261022)
    shape = (k, n, n) if layout == 'tyx' else (n, n, k)
    x = torch.zeros(shape, dtype=torch.float32, device=dev)
    for _ in range(4):
        x -= torch.rand(shape, generator=gen, dtype=torch.float32, device=dev).clamp_(min=1e-30).log_()
    x *= 0.25
    x[torch.rand(shape, generator=gen, device=dev) < 0.01] = float('nan')
    return x


def out_bytes(stats, q, npix):
    total = 0
    for s in stats:
        total += 4 if s in ('count', 'nan_count', 'argmin', 'argmax', 'min', 'max', 'median') else 8
    return (total + 4 * len(q)) * npix


# ---- torch by hand ---------------------------------------------------------------------------------------------------
def torch_moments(x, dim):
    mean = torch.nanmean(x, dim)
    d = x - mean.unsqueeze(dim)
    return mean, torch.nanmean(d * d, dim).sqrt_()


def torch_sorted(x, dim):
    s = torch.sort(x, dim=dim).values                # NaN last
    n = (~torch.isnan(x)).sum(dim)
    return s, n


def _at(s, r, dim):
    return torch.gather(s, dim, r.clamp(min=0).unsqueeze(dim)).squeeze(dim)


def torch_median(s, n, dim):
    return (_at(s, (n - 1) // 2, dim) + _at(s, n // 2, dim)) / 2


def torch_percentile(s, n, dim, p):
    vi = (n - 1).to(torch.float32) * (p / 100.0)
    lo = vi.floor().to(torch.int64)
    hi = torch.minimum(lo + 1, (n - 1).clamp(min=0))
    g = vi - lo
    a, b = _at(s, lo, dim), _at(s, hi, dim)
    return a + (b - a) * g


def torch_request(name, x, dim):
    if name == 'mean_std':
        return torch_moments(x, dim)
    if name == 'median':
        s, n = torch_sorted(x, dim)
        return torch_median(s, n, dim)
    if name == 'p2_p98':
        s, n = torch_sorted(x, dim)
        return torch_percentile(s, n, dim, 2.0), torch_percentile(s, n, dim, 98.0)
    s, n = torch_sorted(x, dim)
    nan = torch.isnan(x)
    mean, std = torch_moments(x, dim)
    lo = x.masked_fill(nan, float('inf'))
    hi = x.masked_fill(nan, float('-inf'))
    return (n, nan.sum(dim), torch.nansum(x, dim), mean, std, std / mean, std * std, lo.amin(dim), hi.amax(dim),
            lo.argmin(dim), hi.argmax(dim), torch_median(s, n, dim), torch_percentile(s, n, dim, 2.0),
            torch_percentile(s, n, dim, 98.0))


def check_band(x, axis, rows):
    """rows 0 .. rows - 1 against the restatement"""
    band = x[:, :rows] if axis == 0 else x[:rows]
    got = kernels.temporal_stats(band, kernels.TEMPORAL_STATS, (2.0, 98.0), axis=axis)
    host = np.moveaxis(band.cpu().numpy(), axis, 0)
    want = ref.stats(host, 0, True, 0, (2.0, 98.0))
    ref.same({s: v.cpu().numpy() for s, v in got.items()}, want, 'band')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'temporal_bench.json'))
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--dates', type=int, nargs='+', default=[24, 48, 100])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--band', type=int, default=8)
    args = ap.parse_args()
    dev = torch.device('cuda', torch.cuda.current_device())
    n, npix = args.size, args.size * args.size
    rows = []
    for k in args.dates:
        for layout in ('tyx', 'yxt'):
            axis = 0 if layout == 'tyx' else 2
            x = speckle(k, n, layout, dev)
            check_band(x, axis, min(args.band, n))
            for name, stats, q in REQUESTS:
                order = 'median' in stats or bool(q)
                tile = k <= kernels.TEMPORAL_LDS_MAX[x.dtype] and (order or layout == 'yxt')
                form = 'register' if k <= kernels.TEMPORAL_REG_MAX[x.dtype] else ('lds' if tile else 'stream')
                ms = min_ms(lambda: kernels.temporal_stats(x, stats, q, axis=axis), args.reps, 2)
                floor = 1e3 * (4.0 * k * npix + out_bytes(stats, q, npix)) / PEAK
                by_hand = min_ms(lambda: torch_request(name, x, axis), 3, 1)
                torch.cuda.empty_cache()
                rows.append({'dates': k, 'layout': layout, 'request': name, 'form': form, 'ms': round(ms, 3),
                             'floor_ms': round(floor, 3), 'times_floor': round(ms / floor, 2),
                             'torch_ms': round(by_hand, 3), 'torch_over_kernel': round(by_hand / ms, 2)})
                print(rows[-1], flush=True)
            del x
            torch.cuda.empty_cache()
    result = {'device': torch.cuda.get_device_name(dev), 'size': n, 'dtype': 'float32', 'reps': args.reps,
              'band_rows_checked': min(args.band, n), 'peak_bytes_per_s': PEAK, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
