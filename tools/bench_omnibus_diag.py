"""Secondary measurement: the intensity-only omnibus test (pol='diag') on a 24 x 4096 x 4096 float32
device-resident stack, q = 1 and 2, alpha = 0.99 and 0.01 -- and, for q = 2, the dual-pol call on the same
C11 / C22 with zero C12 planes (the workaround the test replaces, which reads twice the bytes) in the same
process.  Each figure is the minimum of 5 calls after 2 warm-up calls, every call timed with device events;
the two q = 2 forms alternate call by call so that clock and neighbours treat them alike.  Writes
profiles/omnibus_diag_bench.json (or the path given) and prints it.

    python tools/bench_omnibus_diag.py [--out PATH]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'omnibus_diag_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_omnibus_diag needs a GPU')
    k, ny, nx = 24, 4096, 4096
    looks = 4.4
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    st = synth.empty_stack(4, k, ny, nx, dev)
    # gamma(4.4, 1 / 4.4) speckle on two channels, 1 % of the pixels stepping up by 4 halfway
    conc = torch.full((ny, nx), looks, device=dev)
    mask = torch.rand((ny, nx), generator=gen, device=dev) < 0.01
    for t in range(k):
        for c in (0, 1):
            v = torch._standard_gamma(conc, generator=gen) / looks * (0.5 ** c)
            st[c, t] = torch.where(mask & (t >= k // 2), v * 4.0, v)
    st[2:] = 0.0
    vv, vh, zero_re, zero_im = st[0], st[1], st[2], st[3]
    forms = {
        'diag_q1': lambda alpha: kernels.change_detection_diag([vv], alpha=alpha, n=looks),
        'diag_q2': lambda alpha: kernels.change_detection_diag([vv, vh], alpha=alpha, n=looks),
        'dual_pol_zero_c12': lambda alpha: kernels.change_detection(vv, zero_re, zero_im, vh, alpha=alpha, n=4),
    }
    planes = {'diag_q1': 1, 'diag_q2': 2, 'dual_pol_zero_c12': 4}
    res = {'workload': 'omnibus, intensities only, %dt x %d x %d float32 on the device' % (k, ny, nx),
           'looks': looks, 'timing': 'min of 5 calls after 2 warm-up calls, device events; forms alternate',
           'peak_bytes_per_s': PEAK, 'runs': []}
    for alpha in (0.99, 0.01):
        for _ in range(2):
            for f in forms.values():
                f(alpha)
        torch.cuda.synchronize()
        ms = {name: [] for name in forms}
        changed = {}
        for _ in range(5):
            for name, f in forms.items():
                t, out = timed(lambda: f(alpha))
                ms[name].append(t)
                changed[name] = out
        for name in forms:
            best = min(ms[name])
            nbytes = planes[name] * k * ny * nx * 4
            res['runs'].append({'form': name, 'alpha': alpha, 'ms_min': best, 'ms_all': ms[name],
                                'input_bytes': nbytes, 'input_bytes_per_s': nbytes / (best * 1e-3),
                                'share_of_peak': nbytes / (best * 1e-3) / PEAK,
                                'changed_pixels': float((changed[name].sum(dim=2) > 0).float().mean().item())})
    t = {(r['form'], r['alpha']): r['ms_min'] for r in res['runs']}
    res['gate_q2_not_slower_than_dual_pol_at_0.99'] = bool(t[('diag_q2', 0.99)] <= t[('dual_pol_zero_c12', 0.99)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
