"""A poisoning, guard-banded allocator for tests.

nd_amd's wrappers hand the library memory nobody has initialised: outputs and workspaces come from torch.empty,
torch.empty_like and torch.empty_strided (PATCHED below; tests/test_canary_cpu.py reads the package's text and fails
when a wrapper starts to use another form).  In a pytest process that memory is usually zeros, or the correct result
of the previous, identically shaped case, so an output element no kernel writes, a counter nobody zeroes or a write
past the bytes a *_workspace_bytes entry reported changes no compared value.  Inside

    with canary(0xFF) as c:
        out = kernels.something(...)
        c.check()                        # also run on a clean exit from the block

every such allocation on a covered device type is filled with one byte value, and a contiguous one additionally lies
between two guard bands of `guard_bytes` bytes that must still hold the value afterwards:

    [ guard_bytes of pattern | nbytes of pattern, returned as the requested dtype and shape | guard_bytes of pattern ]

guard_bytes is a multiple of 512, so the returned pointer keeps the alignment the allocator gave the block and the
16-byte fast paths behind `data_ptr() % 16` checks run as they do in production.  A non-contiguous result (empty_like
of a permuted tensor, empty_strided with a pitch) stays torch's own tensor with its storage filled: no guard.  Empty
tensors, pinned host buffers and tensors on other device types pass through untouched.

The two patterns: 0xFF is NaN as float32 / float64, -1 as a signed integer, 255 as a change flag; 0x55 is about
1.5e13 as float32, 1.2e103 as float64, 1431655765 as int32, 85 as a change flag.  No kernel writes either as a flag, a
label or a count.

This is a plain helper: no conftest, no plugin, no pytest setting."""
import os
import sys

import torch

PATTERNS = (0xFF, 0x55)
PATCHED = ('empty', 'empty_like', 'empty_strided')       # the uninitialised-allocation functions nd_amd's Python uses
_HERE = os.path.abspath(__file__)
HELPERS = [_HERE]       # files whose frames are no call site: a helper that wraps the patched functions adds itself
_ACTIVE = []


def _call_site():
    """file:line (function) of the innermost frame outside this module (and outside every file of HELPERS)"""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) in HELPERS:
        f = f.f_back
    if f is None:
        return '?'
    return '%s:%d (%s)' % (os.path.relpath(f.f_code.co_filename, os.path.dirname(os.path.dirname(_HERE))),
                           f.f_lineno, f.f_code.co_name)


class _Record(object):
    __slots__ = ('base', 'nbytes', 'shape', 'dtype', 'site')

    def __init__(self, base, nbytes, shape, dtype, site):
        self.base, self.nbytes, self.shape, self.dtype, self.site = base, nbytes, shape, dtype, site

    def describe(self):
        return 'shape %s, %s, allocated at %s' % (tuple(self.shape), self.dtype, self.site)


class canary(object):
    """Context manager; see the module's docstring.  `wrapped`: how many allocations were poisoned since entry
    (guarded or not), `guarded`: how many of them lie between guard bands."""

    def __init__(self, pattern, guard_bytes=4096, device_types=('cuda',)):
        if not 0 <= int(pattern) <= 255:
            raise ValueError('pattern is one byte value')
        if guard_bytes <= 0 or guard_bytes % 512:
            raise ValueError('guard_bytes must be a positive multiple of 512: the pointer keeps its alignment')
        self.pattern = int(pattern)
        self.guard_bytes = int(guard_bytes)
        self.device_types = tuple(device_types)
        self.wrapped = 0
        self.guarded = 0
        self._records = []
        self._unguarded = []
        self._orig = None

    def allocations(self):
        """[(every byte of the allocation as a flat uint8 tensor, its description)] for what was poisoned since the last
        check(release=True): a guarded allocation with both guard bands, an unguarded one as its whole storage.  For
        helpers that watch the memory the library was handed (tests/held_stream.py)."""
        return [(r.base, r.describe()) for r in self._records] + list(self._unguarded)

    # ---- patching ------------------------------------------------------------------------------------------
    def __enter__(self):
        if _ACTIVE:
            raise RuntimeError('canary blocks do not nest')
        self._orig = {name: getattr(torch, name) for name in PATCHED}
        _ACTIVE.append(self)
        for name in PATCHED:
            setattr(torch, name, self._wrapper(name))
        return self

    def __exit__(self, exc_type, exc, tb):
        for name, fn in self._orig.items():
            setattr(torch, name, fn)
        _ACTIVE.remove(self)
        if exc_type is None:
            self.check()
        self._records = []
        self._unguarded = []
        return False

    def _wrapper(self, name):
        orig = self._orig[name]

        def poisoned(*args, **kwargs):
            t = orig(*args, **kwargs)
            return self._poison(t, kwargs)
        poisoned.__name__ = name
        poisoned.__wrapped__ = orig
        return poisoned

    def _poison(self, t, kwargs):
        if (not isinstance(t, torch.Tensor) or t.device.type not in self.device_types or t.numel() == 0
                or kwargs.get('pin_memory') or kwargs.get('out') is not None or t.layout != torch.strided):
            return t
        self.wrapped += 1
        empty = self._orig['empty']
        if not t.is_contiguous():
            # torch's own tensor, its whole storage filled: no guard
            whole = empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
            whole.fill_(self.pattern)
            self._unguarded.append((whole, 'shape %s, strides %s, %s, allocated at %s'
                                    % (tuple(t.shape), tuple(t.stride()), t.dtype, _call_site())))
            return t
        nbytes = t.numel() * t.element_size()
        g = self.guard_bytes
        base = empty(nbytes + 2 * g, dtype=torch.uint8, device=t.device)
        base.fill_(self.pattern)
        self._records.append(_Record(base, nbytes, tuple(t.shape), t.dtype, _call_site()))
        self.guarded += 1
        return base[g:g + nbytes].view(t.dtype).view(t.shape)

    # ---- checking ------------------------------------------------------------------------------------------
    def check(self, release=True):
        """AssertionError if a guard band of any allocation made so far no longer holds the pattern: the message
        names the allocation, the side and the first changed offset (in bytes, before: counted back from the
        tensor's first byte, after: counted from its end).  release: forget the allocations checked, so that a loop
        over many cases does not keep every case's memory."""
        if any(r.base.is_cuda for r in self._records):
            torch.cuda.synchronize()
        g = self.guard_bytes
        try:
            for r in self._records:
                for side, band in (('before', r.base[:g]), ('after', r.base[g + r.nbytes:])):
                    bad = band != self.pattern
                    if bool(bad.any()):
                        at = int(bad.nonzero()[0, 0])
                        off = (at - g) if side == 'before' else at
                        raise AssertionError(
                            'guard band %s the tensor (%s) was written: first changed byte at offset %d %s, it holds '
                            '0x%02X where the pattern is 0x%02X; %d of %d guard bytes changed'
                            % (side, r.describe(), off,
                               'from its first byte' if side == 'before' else 'past its last byte', int(band[at]),
                               self.pattern, int(bad.sum()), g))
        finally:
            if release:
                self._records = []
                self._unguarded = []

    def is_poison(self, t):
        """elementwise: every byte of the element still holds the pattern (a bool tensor shaped like t)"""
        c = t.contiguous()
        if c.dtype == torch.bool:
            c = c.view(torch.uint8)
        b = c.reshape(-1).view(torch.uint8).view(-1, c.element_size())
        return (b == self.pattern).all(dim=1).view(t.shape)
