"""The border index maps (nd_amd/csrc/borders.hpp) and align256 (entry_args.hpp) without a GPU:
tools/check_borders.cpp is compiled as plain C++ with ROCm's clang++ and run, plainly and with the address and
undefined-behaviour sanitizers (a stand-alone host program: nothing is preloaded).  For array lengths 1 to 9 and
indices from -4 len - 3 to 5 len + 2 it checks extend_line against the extended line built by tiling the pattern,
ml_reflect and reflect_line against its reflect case, the clamped 32-bit instantiations against the clamped 64-bit
results (also at len 2^30 - 1, where the sanitizers would see an overflow), extend_index against extend_line within
one length of the array, reflect_once and align256.

The tables the program prints are then compared with live scipy, whose maps are recovered with one-hot kernels:
2-D weights go through scipy.ndimage.correlate (the offset table, extend_index), 1-D weights through correlate1d
(the line extension, extend_line).  extend_line matches everywhere; extend_index matches everywhere except
reflect at cc = -4 len for len >= 2, where it says -1 (cval): recorded behaviour, asserted as exactly that set.
scipy is not asked at those eight positions.  Its own offset table holds the same -1 there (NI_InitFilterOffsets
runs the same arithmetic) and uses it as an index: it reads the 8 bytes in front of the array, the allocator's
block header, and returns them as a float64 (1.63e-322 for len 2 with scipy 1.15.3 and glibc, which rounds to the
"0" that index 0 of an array 0 .. n - 1 would give).  What scipy returns there is not a property of scipy's rule,
so the test pins this library's side: -1 on exactly that set, and scipy's map everywhere else."""
import os
import subprocess

import numpy as np
import pytest

from .test_omnibus_tables_cpu import ROOT, _clangxx

MODES = ['reflect', 'constant', 'nearest', 'mirror', 'wrap']
OK_LINES = ['ok extend_line', 'ok extend_index (8 positions differ from extend_line)', 'ok 32-bit limit',
            'ok reflect_once', 'ok align256']


def _run(tmp_path, sanitize):
    exe = str(tmp_path / 'check_borders')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g'] if sanitize else []
    subprocess.check_call([_clangxx(), '-std=c++17', '-O1', '-Wall', '-Werror'] + flags +
                          [os.path.join(ROOT, 'tools', 'check_borders.cpp'), '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    assert 'FAILED' not in run.stdout
    return run.stdout.splitlines()


def _table(lines, what):
    """{(mode, len, cc): value} of the program's `what` lines"""
    out = {}
    for ln in lines:
        f = ln.split()
        if f[0] == what:
            out[(f[1], int(f[2]), int(f[3]))] = int(f[4])
    return out


def _scipy_map(mode, n, cc, nd):
    """The index scipy reads for position cc of an array of n elements (-1: cval), through a one-hot kernel:
    the array holds 1 .. n, cval is 0, and the kernel's only tap lies cc to the right of output element 0."""
    import scipy.ndimage as ndi
    reach = 5 * n + 3
    w = np.zeros(2 * reach + 1)
    w[reach + cc] = 1.0
    x = np.arange(1.0, n + 1.0)
    if nd:
        got = ndi.correlate(x[None, :], w[None, :], mode=mode, cval=0.0)[0, 0]
    else:
        got = ndi.correlate1d(x, w, mode=mode, cval=0.0)[0]
    return int(round(got)) - 1


@pytest.mark.parametrize('sanitize', [False, True], ids=['plain', 'asan_ubsan'])
def test_border_maps(tmp_path, sanitize):
    lines = _run(tmp_path, sanitize)
    assert [ln for ln in lines if ln.startswith('ok ')] == OK_LINES
    # where the two rules differ from each other: the positions at which extend_index differs from scipy
    assert [ln for ln in lines if ln.startswith('differ ')] == ['differ reflect %d %d -1 0' % (n, -4 * n)
                                                                  for n in range(2, 10)]


def test_border_maps_against_scipy(tmp_path):
    lines = _run(tmp_path, False)
    line, index = _table(lines, 'line'), _table(lines, 'index')
    domain = {(m, n, cc) for m in MODES for n in range(1, 10) for cc in range(-4 * n - 3, 5 * n + 3)}
    assert set(line) == domain and set(index) == domain
    recorded = {('reflect', n, -4 * n) for n in range(2, 10)}
    line_off = {k for k in domain if line[k] != _scipy_map(k[0], k[1], k[2], nd=False)}
    assert line_off == set()
    index_off = {k for k in domain - recorded if index[k] != _scipy_map(k[0], k[1], k[2], nd=True)}
    assert index_off == set()
    # -1 in a mode that has no cval: nowhere but on the recorded set
    assert {k for k in domain if k[0] != 'constant' and index[k] == -1} == recorded
