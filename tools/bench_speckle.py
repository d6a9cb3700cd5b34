"""Secondary measurement: kernels.speckle_lee and kernels.speckle_multitemporal on a 24-date stack of 4096 x 4096
float32 on the device --

    Lee at w = 3, 7, 11
    multitemporal at w = 7 with k = 24 (one launch), k = 48 (two passes) and jointly on C = 2 variables of k = 12
    Lee and multitemporal at w = 7 on the same stack in (y, x, time) memory: through the planar layout, as the
    filter classes run it (transpose, kernel, transpose back), and the kernel on the strided view where it lies

Each line reports the minimum of 7 calls (device events around the kernels.* call, after 2 warm-up calls) and the
share of 8 TB/s that the definition's own traffic reaches at that time: one read and one write of the stack.  Before
timing, a band of rows of the first and last plane is compared with tests/speckle_ref.py and must be equal.
For scale, on the same device and stack: BoxcarFilter(w), and the composition a user would write without these
kernels for both filters -- BoxcarFilter on x and on x * x plus torch element-wise operations (float32).
Writes profiles/speckle_bench.json (or the path given) and prints it.

    python tools/bench_speckle.py [--out PATH] [--size N] [--dates K] [--reps N]
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
from nd_amd.filters import BoxcarFilter             # noqa: E402
from tests import speckle_cases as cases           # noqa: E402
from tests import speckle_ref as ref               # noqa: E402

PEAK = 8.0e12                                       # HBM3E, bytes / s (datasheet)
BAND = 6                                            # output rows compared with the restatement
LOOKS = 4.0


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


def band_rows(ny, w):
    """(source rows, rows of that window that are outputs free of its borders, output rows)"""
    i0 = ny // 2
    lo, hi = max(0, i0 - w // 2), min(ny, i0 + BAND + w // 2)
    return slice(lo, hi), slice(i0 - lo, i0 - lo + BAND), slice(i0, i0 + BAND)


def check_band(name, stacks, outs, w, restate):
    """BAND rows from the middle of every plane of the planar stacks against the restatement"""
    ny = stacks[0].shape[1]
    src_rows, inner, out_rows = band_rows(ny, w)
    if ny < BAND + w:
        raise SystemExit('the stack is too small for a band check')
    want = restate([s[:, src_rows].cpu().numpy() for s in stacks])
    for o, v in zip(outs, want):
        try:
            cases.assert_same(o[:, out_rows].cpu().numpy(), np.ascontiguousarray(v[:, inner]))
        except AssertionError as e:
            raise SystemExit('%s: the kernel differs from the restatement on rows %d..%d: %s'
                             % (name, out_rows.start, out_rows.stop, e))


def boxcar(stack, w, out):
    BoxcarFilter(dims=('y', 'x'), w=w)._filter(stack, (1, 2), out)
    return out


def lee_by_hand(x, w, looks):
    """what a user writes today: two boxcar passes and torch element-wise operations"""
    m = boxcar(x, w, torch.empty_like(x))
    m2 = boxcar(x * x, w, torch.empty_like(x))
    v = m2 - m * m
    b = 1.0 - (m * m) * (1.0 / looks) / v
    b = torch.where((v > 0) & (b > 0), b, torch.zeros_like(b))
    return m + b * (x - m)


def multitemporal_by_hand(x, w):
    m = boxcar(x, w, torch.empty_like(x))
    r = (x / m).sum(0)
    return m * r / x.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'speckle_bench.json'))
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--dates', type=int, default=24)
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_speckle needs a GPU')
    N, k, reps = args.size, args.dates, args.reps
    dev = torch.device('cuda:0')
    torch.manual_seed(4096)
    gamma = torch.distributions.Gamma(torch.tensor(LOOKS, device=dev), torch.tensor(LOOKS, device=dev))
    stack = gamma.sample((k, N, N)).to(torch.float32)
    res = {'workload': 'speckle filters, %d dates of %d x %d float32 on the device, gamma speckle of %g looks'
                       % (k, N, N, LOOKS),
           'timing': 'min of %d calls after 2 warm-up calls, device events around the kernels.* call' % reps,
           'traffic': 'one read and one write of the stack; share of %g B/s' % PEAK,
           'peak_bytes_per_s': PEAK, 'runs': [], 'for_scale': []}

    def record(name, fn, nbytes, **extra):
        ms = min_ms(fn, reps)
        run = dict(name=name, ms_min=min(ms), ms_all=ms, traffic_bytes=nbytes, traffic_floor_ms=nbytes / PEAK * 1e3,
                   share_of_peak=nbytes / (min(ms) * 1e-3) / PEAK, equal_to_restatement_on_band=True, **extra)
        res['runs'].append(run)
        print(json.dumps(run), flush=True)

    def scale(name, fn):
        ms = min_ms(fn, reps)
        res['for_scale'].append({'name': name, 'ms_min': min(ms), 'ms_all': ms})
        print(json.dumps(res['for_scale'][-1]), flush=True)

    nbytes = 2 * stack.numel() * stack.element_size()
    out = torch.empty_like(stack)
    for w in (3, 7, 11):
        kernels.speckle_lee(stack, w, LOOKS, 'lee', out=out)
        check_band('lee w=%d' % w, [stack], [out], w, lambda s, w=w: [ref.lee(s[0], w, LOOKS, 'lee')])
        record('lee, w = %d' % w, lambda w=w: kernels.speckle_lee(stack, w, LOOKS, 'lee', out=out), nbytes, w=w)
        scale('BoxcarFilter(w=%d) on the stack' % w, lambda w=w: boxcar(stack, w, out))
        scale('lee by hand: BoxcarFilter(w=%d) on x and x * x plus torch element-wise' % w,
              lambda w=w: lee_by_hand(stack, w, LOOKS))
    w = 7
    kernels.speckle_multitemporal(stack, w, out=out)
    check_band('multitemporal k=%d' % k, [stack], [out], w, lambda s: [ref.multitemporal(s[0], w)])
    record('multitemporal, w = 7, k = %d (one launch)' % k,
           lambda: kernels.speckle_multitemporal(stack, w, out=out), nbytes, w=w, k=k, variables=1)
    scale('multitemporal by hand: BoxcarFilter(w=7) plus torch element-wise, k = %d' % k,
          lambda: multitemporal_by_hand(stack, w))
    half = k // 2
    pair, pair_out = [stack[:half], stack[half:2 * half]], [out[:half], out[half:2 * half]]
    kernels.speckle_multitemporal(pair, w, out=pair_out)
    check_band('multitemporal joint', pair, pair_out, w, lambda s: ref.multitemporal(s, w))
    record('multitemporal jointly, w = 7, C = 2, k = %d (one launch)' % half,
           lambda: kernels.speckle_multitemporal(pair, w, out=pair_out), 2 * 2 * half * N * N * 4, w=w, k=half,
           variables=2)
    # (y, x, time) memory
    pm = stack.permute(1, 2, 0).contiguous()
    pm_out = torch.empty_like(pm)
    planar = torch.empty_like(stack)

    def through_planar(run):
        if not kernels.relayout_planar(pm, planar):
            raise SystemExit('relayout_planar does not take the stack')
        done = run(planar)
        if not kernels.relayout_pixel_major(done, pm_out):
            raise SystemExit('relayout_pixel_major does not take the stack')

    for name, run, restate in (
            ('lee, w = 7', lambda p, o=None, d=('time', 'y', 'x'): kernels.speckle_lee(p, w, LOOKS, 'lee', out=o, dims=d),
             lambda s: [ref.lee(s[0], w, LOOKS, 'lee')]),
            ('multitemporal, w = 7, k = %d' % k,
             lambda p, o=None, d=('time', 'y', 'x'): kernels.speckle_multitemporal(p, w, dims=d, out=o),
             lambda s: [ref.multitemporal(s[0], w)])):
        through_planar(run)
        check_band(name + ' (y, x, time)', [stack], [pm_out.permute(2, 0, 1)], w, restate)
        record(name + ', (y, x, time) through the planar layout', lambda run=run: through_planar(run), nbytes, w=w)
        pm_out.zero_()
        run(pm, pm_out, ('y', 'x', 'time'))
        check_band(name + ' (y, x, time) where it lies', [stack], [pm_out.permute(2, 0, 1)], w, restate)
        record(name + ', (y, x, time) read where it lies', lambda run=run: run(pm, pm_out, ('y', 'x', 'time')), nbytes,
               w=w)
    del pm, pm_out, planar, out
    torch.cuda.empty_cache()
    # twice the dates: the two-pass form
    long = torch.cat([stack, gamma.sample((k, N, N)).to(torch.float32)])
    long_out = torch.empty_like(long)
    kernels.speckle_multitemporal(long, w, out=long_out)
    check_band('multitemporal k=%d' % (2 * k), [long], [long_out], w, lambda s: [ref.multitemporal(s[0], w)])
    record('multitemporal, w = 7, k = %d (two passes)' % (2 * k),
           lambda: kernels.speckle_multitemporal(long, w, out=long_out), 2 * nbytes, w=w, k=2 * k, variables=1)
    scale('multitemporal by hand: BoxcarFilter(w=7) plus torch element-wise, k = %d' % (2 * k),
          lambda: multitemporal_by_hand(long, w))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
