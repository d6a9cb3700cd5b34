"""The dispatch helpers (nd_amd/csrc/dispatch.hpp) without a GPU: tools/check_dispatch.cpp is compiled as plain
C++ with ROCm's clang++ and run.  For every v from 0 to one past the last list value it checks that pick_le calls
its callback exactly once with the first V >= v (and not at all, returning false, beyond the list), that pick_eq
does the same for exact matches, and that pick forwards both values.  The program is built twice: plainly, and
with the address and undefined-behaviour sanitizers (a stand-alone host program: nothing is preloaded)."""
import os
import subprocess

import pytest

from .test_omnibus_tables_cpu import ROOT, _clangxx


@pytest.mark.parametrize('sanitize', [False, True], ids=['plain', 'asan_ubsan'])
def test_dispatch_helpers(tmp_path, sanitize):
    exe = str(tmp_path / 'check_dispatch')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g'] if sanitize else []
    subprocess.check_call([_clangxx(), '-std=c++17', '-O1', '-Wall', '-Werror'] + flags +
                          [os.path.join(ROOT, 'tools', 'check_dispatch.cpp'), '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert [ln for ln in run.stdout.splitlines() if ln.startswith('ok ')] == ['ok pick_le', 'ok pick_eq', 'ok pick',
                                                                               'ok nested']
    assert 'FAILED' not in run.stdout


@pytest.mark.parametrize('sanitize', [False, True], ids=['plain', 'asan_ubsan'])
def test_grid_helpers(tmp_path, sanitize):
    """shard_blocks and row_walk / row_blocks (nd_amd/csrc/entry_args.hpp) against the clamp and the row walk the
    launch sites used to write out (tools/check_entry_args.cpp): every (shards, entries per block, cap) of the
    library on both sides of every step up to 2^32 - 2 listed pixels; flat, strided and forced-flat rasters and
    the shapes around 2^31 - 1 blocks.  A stand-alone host program, as above."""
    exe = str(tmp_path / 'check_entry_args')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g'] if sanitize else []
    subprocess.check_call([_clangxx(), '-std=c++17', '-O1', '-Wall', '-Werror'] + flags +
                          [os.path.join(ROOT, 'tools', 'check_entry_args.cpp'), '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert [ln for ln in run.stdout.splitlines() if ln.startswith('ok ')] == ['ok shard_blocks', 'ok row_walk']
    assert 'FAILED' not in run.stdout
