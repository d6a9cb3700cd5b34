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


@pytest.mark.parametrize('sanitize', [False, True], ids=['plain', 'asan_ubsan'])
def test_lds_stage_pieces(tmp_path, sanitize):
    """lds_stage_piece / lds_stage_tail (nd_amd/csrc/memops.hpp, the plain part the staging loops of the pixel-major
    omnibus kernels run): for every run length up to 64 pixels x 48 dates x 2 x 8 bytes, multiples of 16 without and
    multiples of 4 with the 4-byte tail, the pieces of 64 lanes over all steps cover the run exactly once, stay inside
    it, land at the offset they came from and are the transfers of the loop as the kernels wrote it before
    (tools/check_memops.cpp).  A stand-alone host program, as above."""
    exe = str(tmp_path / 'check_memops')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g'] if sanitize else []
    subprocess.check_call([_clangxx(), '-std=c++17', '-O1', '-Wall', '-Werror'] + flags +
                          [os.path.join(ROOT, 'tools', 'check_memops.cpp'), '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert [ln for ln in run.stdout.splitlines() if ln.startswith('ok ')] == [
        'ok plain form: run lengths 0 .. 49152 in steps of 16', 'ok tail form: run lengths 0 .. 49152 in steps of 4']
    assert 'FAILED' not in run.stdout


def test_memory_idioms_are_named_in_one_place():
    """The buffer-descriptor builtin, the raw buffer loads and stores, the LDS-DMA builtin and the two bare waits
    occur in nd_amd/csrc/memops.hpp only; the waits also in omnibus_ml.hip, whose assembly transfers are waited for by
    count.  One recorded exception (profiles/memops_codeobj.txt): the scalar tail store of correlate_roll_kernel stays
    written out, because through the wrapper its 3 x 3 and 5 x 5 instantiations differ from the parent's."""
    import re
    csrc = os.path.join(ROOT, 'nd_amd', 'csrc')
    builtins = re.compile(r'make_buffer_rsrc|raw_buffer_load_\w+|raw_buffer_store_\w+|global_load_lds')
    waits = ('"s_waitcnt vmcnt(0)"', '"s_waitcnt lgkmcnt(0)"')
    named, waited = {}, set()
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(('.hip', '.hpp')):
            continue
        text = open(os.path.join(csrc, f)).read()
        code = re.sub(r'//[^\n]*', '', text)                       # (comments may speak of them)
        hits = builtins.findall(code)
        if hits:
            named[f] = sorted(hits)
        if any(w in text for w in waits):
            waited.add(f)
    assert set(named) == {'memops.hpp', 'correlate.hip'}, named
    assert named['correlate.hip'] == ['raw_buffer_store_b32'], named['correlate.hip']
    assert waited == {'memops.hpp', 'omnibus_ml.hip'}, waited
