"""Records tests/golden/omnibus_diag.npz (+ omnibus_diag_f64.npz: the float64 z / P rasters, which would
take the first file past the size limit for a committed file) from the numpy restatement
tests/omnibus_diag_ref.py:

    python tests/golden/make_omnibus_diag_golden.py

Per case of tests/omnibus_diag_cases.py: the seed, per threshold the packed change map and the smallest
|P - alpha| the search met, and z / P of the whole-series test.  A seed is kept only if no test the search
asks has |P - alpha| <= 16 ulp(T) at any of the case's thresholds (the next seed is tried otherwise), so
that an implementation whose P differs in the last bits still decides every recorded test the same way.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import omnibus_diag_cases as C      # noqa: E402
from tests import omnibus_diag_ref as R        # noqa: E402


def record_case(case):
    """-> (seed, {alpha: (map, closest)}, z, P) for the first seed that keeps every decision clear of alpha."""
    for attempt in range(64):
        seed = case['seed'] + attempt
        planes = C.make_input(case, seed)
        S = R.Series(planes, (1,) * case['q'], case['n'])
        per_alpha, ok = {}, True
        for alpha in case['alphas']:
            m, z, P = R.change_detection(planes, (1,) * case['q'], alpha, case['n'], series=S)
            if S.closest <= 16 * C.ulp(alpha, case['dtype']):
                ok = False
                break
            per_alpha[alpha] = (m, S.closest)
        if ok:
            return seed, per_alpha, z, P
    raise RuntimeError('no seed found for %s' % case['name'])


def main():
    main_file, f64_file = {}, {}
    names, seeds = [], []
    for case in C.cases():
        seed, per_alpha, z, P = record_case(case)
        names.append(case['name'])
        seeds.append(seed)
        for alpha, (m, closest) in per_alpha.items():
            assert closest > 16 * C.ulp(alpha, case['dtype'])
            main_file['map/%s/%g' % (case['name'], alpha)] = np.packbits(m.ravel())
            main_file['closest/%s/%g' % (case['name'], alpha)] = np.float64(closest)
        dst = main_file if case['dtype'] == 'float32' else f64_file
        dst['z/' + case['name']] = z
        dst['P/' + case['name']] = P
        print(case['name'], 'seed', seed, 'changes', [int(m.sum()) for m, _ in per_alpha.values()])
    main_file['names'] = np.array(names)
    main_file['seeds'] = np.array(seeds, np.int64)
    np.savez_compressed(C.GOLDEN, **main_file)
    np.savez_compressed(C.GOLDEN_F64, **f64_file)
    for p in (C.GOLDEN, C.GOLDEN_F64):
        assert os.path.getsize(p) < 1024 * 1024, p
        print(p, os.path.getsize(p), 'bytes')


if __name__ == '__main__':
    main()
