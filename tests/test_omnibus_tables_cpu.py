"""The omnibus decision tables (nd_amd/csrc/omnibus_tables.hip) without a GPU: the unit and the dump program
tools/dump_omnibus_tables.cpp are compiled as plain C++ with ROCm's clang++, and what the bounds of every
entry promise is checked against the oracle's chi-square CDF -- with no tolerance: the bounds carry their own
margin (>= 1e-11 in P, omni_bounds), the oracle's CDF is pinned at 2e-13."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the grid of tools/dump_omnibus_tables.cpp, in its order
FAMILIES = [('c2', 2, 1), ('c3', 3, 1), ('diag', 1, 1), ('diag', 1, 2), ('diag', 1, 3)]
DTYPES = ['float32', 'float64']
ALPHAS = [1e-4, 0.01, 0.5, 0.9, 0.99]
LOOKS = [1.0, 4.0, 4.4, 9.0]
K = 48
J_DUMPED = list(range(1, K + 1)) + [97, 200]
J_CHECKED = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 25, 32, 48, 97, 200]

ENTRY = np.dtype([(f, '<f8') for f in ('m2rho', 'pklogk', 'omega2', 'lgam', 'zlo', 'zlo_a', 'zhi', 'zhi_a')])
DENSE = np.dtype([('re', '<i4'), ('rf', '<f4'), ('a', '<f4'), ('b', '<f4')])
STREAM = np.dtype([('e', [('re', '<i4'), ('rf', '<f4'), ('a', '<f4'), ('b', '<f4'), ('jf', '<f4'), ('cj', '<f4'),
                          ('mj', '<f4'), ('pad', '<f4')], (129,)),
                   ('ca', '<f4', (2,)), ('cb', '<f4', (2,)), ('dlo', '<f4'), ('dhi', '<f4')])


def _clangxx():
    from nd_amd import build
    cand = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), '..', 'lib', 'llvm', 'bin', 'clang++')
    for c in (os.environ.get('ND_AMD_CLANGXX'), cand, '/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++')):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("ROCm's clang++ not found (set ND_AMD_CLANGXX)")


@pytest.fixture(scope='module')
def records(tmp_path_factory):
    """[(family, p, q, dtype, alpha, n, entries[50], dense[131] or None, stream or None, entries_again[48])]"""
    exe = str(tmp_path_factory.mktemp('omnibus_tables') / 'dump_omnibus_tables')
    subprocess.check_call([_clangxx(), '-x', 'c++', '-std=c++17', '-O2', '-ffp-contract=off', '-fno-fast-math',
                           os.path.join(ROOT, 'tools', 'dump_omnibus_tables.cpp'),
                           os.path.join(ROOT, 'nd_amd', 'csrc', 'omnibus_tables.hip'), '-o', exe])
    raw = subprocess.run([exe, '--repeat'], check=True, stdout=subprocess.PIPE).stdout
    assert ENTRY.itemsize == 64 and DENSE.itemsize == 16 and STREAM.itemsize == 4152
    out, pos = [], 0

    def take(dtype, count):
        nonlocal pos
        a = np.frombuffer(raw, dtype, count, pos)
        pos += count * dtype.itemsize
        return a

    for fam, p, q in FAMILIES:
        for dt in DTYPES:
            for alpha in ALPHAS:
                for n in LOOKS:
                    whole = n == math.floor(n)
                    if not whole and p != 1:
                        continue
                    entries = take(ENTRY, len(J_DUMPED))
                    dense = take(DENSE, 129 + 2) if whole else None
                    stream = take(STREAM, 1)[0] if whole else None
                    again = take(ENTRY, K)
                    out.append((fam, p, q, dt, alpha, n, entries, dense, stream, again))
    assert pos == len(raw)
    return out


def _P(oracle, z, f, omega2):
    """P(z) = P1 + omega2 (P2 - P1) as the kernels combine it, in double"""
    p1 = oracle.cdf_chisq_P(z, f)
    p2 = oracle.cdf_chisq_P(z, f + 4)
    return p1 + omega2 * (p2 - p1)


def test_bounds_hold_against_the_oracle(oracle, records):
    """zlo_a <= zlo <= zhi <= zhi_a (or zlo = +inf: nothing fires), P(zlo) <= alpha and P(zhi) >= alpha for every
    finite bound -- and enough finite bounds in every family that the check cannot pass by skipping them
    (on the whole-number look counts 1, 4, 9: 2 400 entries, of which 1 830 carry finite bounds; 280 / 200 /
    1 350 in c2 / c3 / diag)."""
    total = {'all': 0, 'whole': 0}
    finite_lo = {'c2': 0, 'c3': 0, 'diag': 0}
    finite_hi = {'c2': 0, 'c3': 0, 'diag': 0}
    for fam, p, q, dt, alpha, n, entries, _, _, _ in records:
        whole = n == math.floor(n)
        for j in J_CHECKED:
            e = entries[J_DUMPED.index(j)]
            where = (fam, q, dt, alpha, n, j)
            total['all'] += 1
            total['whole'] += whole
            zlo, zhi, omega2 = float(e['zlo']), float(e['zhi']), float(e['omega2'])
            f = q * (j - 1) * p * p
            assert e['zlo_a'] <= zlo, where
            assert zhi <= e['zhi_a'], where
            assert zlo <= zhi or zlo == math.inf, where
            if math.isfinite(zlo):
                finite_lo[fam] += whole
                P = _P(oracle, zlo, f, omega2)
                print('P(zlo) - alpha = %.3e' % (P - alpha), where)
                assert P <= alpha, where
            if math.isfinite(zhi):
                finite_hi[fam] += whole
                P = _P(oracle, zhi, f, omega2)
                print('P(zhi) - alpha = %.3e' % (P - alpha), where)
                assert P >= alpha, where
    assert total == {'all': 2880, 'whole': 2400}
    for finite in (finite_lo, finite_hi):
        assert sum(finite.values()) >= 1800, finite
        assert all(v >= 180 for v in finite.values()), finite


def test_screens_are_ordered(records):
    """a <= b in every dense entry and ca <= cb for both marginal tests of the stream screen."""
    seen = 0
    for fam, p, q, dt, alpha, n, _, dense, stream, _ in records:
        if dense is None:
            continue
        assert (dense['a'] <= dense['b']).all(), (fam, q, dt, alpha, n)
        assert (stream['e']['a'] <= stream['e']['b']).all(), (fam, q, dt, alpha, n)
        assert (stream['ca'] <= stream['cb']).all(), (fam, q, dt, alpha, n)
        seen += 1
    assert seen == 150


def test_cached_table_equals_the_first(records):
    """A second get_table call with the same key returns the bytes of the first."""
    for fam, p, q, dt, alpha, n, entries, _, _, again in records:
        assert entries[:K].tobytes() == again.tobytes(), (fam, q, dt, alpha, n)
