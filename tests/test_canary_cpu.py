"""tests/canary.py can fail: on CPU tensors (device_types=('cpu',)) it poisons every call form the package uses,
passes through what it does not cover, restores torch's functions, reports a write one element before or behind a
tensor with the side and the offset, and lets clean use pass.  The last test reads nd_amd/*.py as text: no wrapper
may allocate uninitialised memory through a form the canary does not patch."""
import glob
import os
import re

import pytest
import torch

from tests.canary import PATCHED, PATTERNS, canary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = ('cpu',)


def all_bytes(t, pattern):
    """every byte of the (possibly strided) tensor's elements holds the pattern"""
    c = t.contiguous()
    return bool((c.reshape(-1).view(torch.uint8) == pattern).all())


@pytest.mark.parametrize('pattern', PATTERNS)
def test_poisons_every_call_form(pattern):
    like = torch.zeros(4, 6, dtype=torch.float64)
    perm = torch.zeros(4, 6, 5).permute(2, 0, 1)
    with canary(pattern, device_types=CPU) as c:
        made = [torch.empty(3, 5),
                torch.empty((3, 5)),
                torch.empty([2, 3, 4], dtype=torch.float64),
                torch.empty((7,), dtype=torch.uint8, device='cpu'),
                torch.empty(11, dtype=torch.uint8, device=torch.device('cpu')),
                torch.empty((), dtype=torch.int64, device='cpu'),
                torch.empty(like.shape, dtype=like.dtype, device=like.device),
                torch.empty((2, 2), dtype=torch.int8),
                torch.empty_like(like),
                torch.empty_like(perm, memory_format=torch.contiguous_format),
                torch.empty_strided((2, 3), (3, 1), dtype=torch.float32, device='cpu')]
        assert c.wrapped == len(made) == c.guarded
        strided = [torch.empty_like(perm),                                    # keeps the permuted strides
                   torch.empty_strided((3, 4), (1, 3), dtype=torch.float64),
                   torch.empty_strided((2, 3), (5, 1), dtype=torch.float32)]  # a pitch: the gaps are poisoned too
        assert c.wrapped == len(made) + 3 and c.guarded == len(made)
        for t in made:
            assert t.is_contiguous() and all_bytes(t, pattern), (t.shape, t.dtype)
        for t in strided:
            assert not t.is_contiguous() and all_bytes(t, pattern)
            assert bool((torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage()) == pattern).all())
        assert strided[0].stride() == perm.stride() and strided[0].shape == perm.shape
        assert made[0].shape == (3, 5) and made[0].dtype == torch.float32
        assert made[2].shape == (2, 3, 4) and made[2].dtype == torch.float64
        assert made[5].shape == () and made[5].dtype == torch.int64
        assert made[9].shape == perm.shape
        assert bool(c.is_poison(made[2]).all()) and bool(c.is_poison(strided[0]).all())
    if pattern == 0xFF:
        assert bool(torch.isnan(made[0]).all()) and bool(torch.isnan(made[2]).all()) and int(made[5]) == -1
    else:
        assert float(made[0][0, 0]) > 1e13 and int(made[5]) > 2 ** 62 and int(made[3][0]) == 85


def test_passes_through_what_it_does_not_cover():
    with canary(0xFF, device_types=('cuda',)) as c:           # CPU tensors are not covered here
        t = torch.empty(5)
        u = torch.empty_like(torch.zeros(3))
        assert c.wrapped == 0
    assert t.shape == (5,) and u.shape == (3,)
    with canary(0xFF, device_types=CPU) as c:
        e = [torch.empty(0), torch.empty((3, 0, 2)), torch.empty_like(torch.zeros(0, 4)),
             torch.empty_strided((0,), (1,))]
        m = torch.empty(4, device='meta')                      # another device type
        assert c.wrapped == 0
        assert [tuple(t.shape) for t in e] == [(0,), (3, 0, 2), (0, 4), (0,)] and m.device.type == 'meta'


def test_restores_after_exit_and_after_an_exception():
    before = {name: getattr(torch, name) for name in PATCHED}
    with canary(0x55, device_types=CPU):
        assert all(getattr(torch, name) is not before[name] for name in PATCHED)
    assert all(getattr(torch, name) is before[name] for name in PATCHED)
    with pytest.raises(KeyError):
        with canary(0x55, device_types=CPU):
            torch.empty(3)
            raise KeyError('inside')
    assert all(getattr(torch, name) is before[name] for name in PATCHED)
    with pytest.raises(AssertionError):                         # a touched guard: restored all the same
        with canary(0x55, device_types=CPU):
            t = torch.empty(3)
            torch.as_strided(t, (4,), (1,))[3] = 0.0
    assert all(getattr(torch, name) is before[name] for name in PATCHED)
    with pytest.raises(RuntimeError):
        with canary(0x55, device_types=CPU):
            with canary(0xFF, device_types=CPU):
                pass
    assert all(getattr(torch, name) is before[name] for name in PATCHED)


@pytest.mark.parametrize('pattern', PATTERNS)
def test_a_write_past_the_end_is_caught(pattern):
    with pytest.raises(AssertionError) as err:
        with canary(pattern, device_types=CPU):
            t = torch.empty((3, 5), dtype=torch.float32)
            torch.as_strided(t, (16,), (1,))[15] = 1.0          # one element past the end
    msg = str(err.value)
    assert 'after' in msg and 'offset 0 ' in msg and '(3, 5)' in msg and 'torch.float32' in msg
    assert 'test_canary_cpu.py' in msg and 'test_a_write_past_the_end_is_caught' in msg
    # an explicit check(), deeper into the guard, a second allocation untouched
    with canary(pattern, device_types=CPU) as c:
        ok = torch.empty(9, dtype=torch.uint8)
        ok[:] = 1
        t = torch.empty(10, dtype=torch.int64)
        torch.as_strided(t, (40,), (1,))[33] = 7                # 23 elements past the end: byte 184
        with pytest.raises(AssertionError) as err:
            c.check()
        assert 'after' in str(err.value) and 'offset 184 ' in str(err.value) and '(10,)' in str(err.value)
        c.check()                                               # the checked allocations were released


@pytest.mark.parametrize('pattern', PATTERNS)
def test_a_write_before_the_start_is_caught(pattern):
    with canary(pattern, device_types=CPU) as c:
        t = torch.empty(6, dtype=torch.float64)
        torch.as_strided(t, (1,), (1,), t.storage_offset() - 1)[0] = 2.0      # one element before the start
        with pytest.raises(AssertionError) as err:
            c.check()
    msg = str(err.value)
    assert 'before' in msg and 'offset -8 ' in msg and '(6,)' in msg and 'torch.float64' in msg


@pytest.mark.parametrize('pattern', PATTERNS)
def test_clean_use_passes(pattern):
    with canary(pattern, device_types=CPU) as c:
        a = torch.empty((4, 7), dtype=torch.float64)
        a[:] = torch.arange(28, dtype=torch.float64).view(4, 7)
        b = torch.empty(513, dtype=torch.uint8)
        b.fill_(0)
        d = torch.empty_like(a)
        d.copy_(a)
        c.check(release=False)
        assert c.wrapped == 3
    assert float(a.sum()) == 27 * 28 / 2 and torch.equal(a, d)


@pytest.mark.parametrize('pattern', PATTERNS)
def test_an_unwritten_part_still_shows_the_pattern(pattern):
    with canary(pattern, device_types=CPU) as c:
        out = torch.empty(10, dtype=torch.float32)
        out[:6] = 1.0
        left = c.is_poison(out)
        assert left.tolist() == [False] * 6 + [True] * 4
        flags = torch.empty((2, 5), dtype=torch.uint8)
        flags[0] = 0
        assert c.is_poison(flags).tolist() == [[False] * 5, [True] * 5]
    assert bool(torch.isnan(out[6:]).all()) if pattern == 0xFF else bool((out[6:] > 1e13).all())


def test_alignment_is_the_allocation_s():
    with canary(0xFF, device_types=CPU) as c:
        for n in (1, 3, 64, 1000):
            t = torch.empty(n, dtype=torch.float32)
            base = c._records[-1].base
            assert t.data_ptr() == base.data_ptr() + c.guard_bytes
            assert t.data_ptr() % 512 == base.data_ptr() % 512 and t.data_ptr() % 64 == 0
    with pytest.raises(ValueError):
        canary(0xFF, guard_bytes=100)


# every way to get uninitialised memory from torch that the canary does NOT patch
UNCOVERED = (r'\bempty_permuted\b', r'\bempty_quantized\b', r'\bnew_empty\b', r'\bnew_empty_strided\b', r'\bresize_\b',
             r'\bresize_as_\b', r'\.new\(', r'\bset_\(', r'torch\.\w*Tensor\(', r'torch\.\w*Storage\(',
             r'\bUntypedStorage\(', r'\b_empty_affine_quantized\b', r'\bfrom_file\b')
# the patch replaces attributes of the torch module: a name bound at import time would keep the original
ALIASES = (r'from\s+torch\s+import\s+[^\n]*\bempty', r'=\s*torch\.empty(_like|_strided)?\s*$',
           r'getattr\(\s*torch\s*,')


def test_the_package_allocates_through_covered_forms_only():
    files = sorted(glob.glob(os.path.join(ROOT, 'nd_amd', '*.py')))
    assert len(files) > 10
    seen = set()
    for path in files:
        text = open(path).read()
        name = os.path.relpath(path, ROOT)
        for rx in UNCOVERED + ALIASES:
            hit = re.search(rx, text, re.M)
            assert hit is None, '%s uses %r, which tests/canary.py does not poison' % (name, hit.group(0))
        # every torch.<something>empty<something> the package calls is a patched function
        for fn in re.findall(r'\btorch\.(\w*empty\w*)', text):
            assert fn in PATCHED, '%s calls torch.%s, which tests/canary.py does not patch' % (name, fn)
            seen.add(fn)
    assert seen == set(PATCHED), 'tests/canary.py patches %s, the package uses %s' % (sorted(PATCHED), sorted(seen))
