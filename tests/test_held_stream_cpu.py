"""tests/held_stream.py without a GPU: a fake library of Python callables, CPU tensors and a fake timeline in place of
the streams.  The proxy forwards arguments, return values, argtypes and restype unchanged; the header parse yields
exactly the entries with a `hip_stream` parameter, all of them symbols of nd_amd/_lib.py; held, waited and
inconclusive are told apart as the module's docstring says; a changed byte of a held call is reported by entry,
allocation and offset; nd_amd._lib._lib and torch's functions are restored, after an exception too."""
import ctypes as C
import os
import re

import pytest
import torch

from nd_amd import _lib
from tests import held_stream as hs
from tests.canary import PATCHED
from tests.held_stream import HELD, INCONCLUSIVE, WAITED, held_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')
HANDLE = 0x5EED


class FakeFunction(object):
    """a Python callable with the attributes of a ctypes function"""

    def __init__(self, fn, argtypes, restype=C.c_int):
        self.fn, self.argtypes, self.restype, self.calls = fn, argtypes, restype, []

    def __call__(self, *args):
        self.calls.append(args)
        return self.fn(*args)


class FakeLibrary(object):
    def __init__(self):
        vp, i64 = C.c_void_p, C.c_int64
        self.nd_amd_split_complex = FakeFunction(lambda *a: 0, [vp, vp, vp, C.c_int, i64, vp])
        self.nd_amd_merge_complex = FakeFunction(lambda *a: -3, [vp, vp, vp, C.c_int, i64, vp])
        self.nd_amd_zonal_workspace_bytes = FakeFunction(lambda *a: 4096, [i64] * 4, C.c_size_t)
        self.nd_amd_last_error = FakeFunction(lambda: b'nothing', [], C.c_char_p)


class FakeTimeline(object):
    """script: per call (reached behind the call, reached behind the comparison); compare() diffs for real"""
    stream_handle = HANDLE

    def __init__(self, script=()):
        self.script, self.begun, self.compared, self.finished = list(script), 0, 0, 0

    def begin(self, tracked):
        self.begun += 1
        after = self.script.pop(0) if self.script else (False, False)
        return {'tracked': list(tracked), 'snaps': [t.clone() for t in tracked], 'after': list(after)}

    def reached(self, token):
        return token['after'].pop(0)

    def compare(self, token):
        self.compared += 1
        for i, (now, then) in enumerate(zip(token['tracked'], token['snaps'])):
            ne = now != then
            if bool(ne.any()):
                at = int(ne.to(torch.uint8).argmax())
                return i, at, int(then[at]), int(now[at])
        return None

    def finish(self):
        self.finished += 1


@pytest.fixture
def fake():
    before = _lib._lib
    _lib._lib = FakeLibrary()
    try:
        yield _lib._lib
    finally:
        _lib._lib = before


def test_header_parse_yields_the_stream_taking_entries():
    entries = hs.header_entries()
    streamed = hs.stream_entries()
    text = open(hs.HEADER).read()
    # every prototype the header declares is a symbol of the binding, and the other way round
    assert set(entries) == set(_lib.SYMBOLS), (sorted(set(entries) ^ set(_lib.SYMBOLS)))
    assert set(streamed) <= set(_lib.SYMBOLS)
    # counted another way: the declarations that mention the parameter, comments removed
    bare = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    assert len(streamed) == len(re.findall(r'void\s*\*\s*hip_stream\b', bare)) > 40
    for name, params in streamed.items():
        assert params.count('hip_stream') == 1 and params[-1] == 'hip_stream', name
    for name in ('nd_amd_abi_version', 'nd_amd_last_error', 'nd_amd_timing_enable', 'nd_amd_timing_collect',
                 'nd_amd_zonal_workspace_bytes', 'nd_amd_omnibus_c2_uses_wave_search',
                 'nd_amd_classify_workspace_bytes'):
        assert name in entries and name not in streamed
    assert entries['nd_amd_abi_version'] == [] and entries['nd_amd_timing_enable'] == ['capacity']
    # names, with array brackets and comments inside the list out of the way
    assert entries['nd_amd_omnibus_c3'][:3] == ['planes', 'dtype', 'ny'] and 'k' in entries['nd_amd_omnibus_c3']
    assert entries['nd_amd_correlate'][6] == 'ntaps'
    assert entries['nd_amd_resample_check_table'][:3] == ['start', 'count', 'm']
    # as many names as the binding has argument types
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        for name, params in entries.items():
            assert len(getattr(L, name).argtypes) == len(params), name


def test_proxy_forwards_arguments_results_and_types(fake):
    with held_stream(CPU, 20.0, timeline=FakeTimeline()) as h:
        L = _lib.lib()
        assert L is h.proxy and L is not fake
        # no stream: the library's own object
        assert L.nd_amd_zonal_workspace_bytes is fake.nd_amd_zonal_workspace_bytes
        assert L.nd_amd_zonal_workspace_bytes(1, 2, 3, 4) == 4096 and L.nd_amd_last_error() == b'nothing'
        # a stream: wrapped, the same types, arguments and result
        f = L.nd_amd_split_complex
        assert f is not fake.nd_amd_split_complex and f is L.nd_amd_split_complex
        assert f.argtypes is fake.nd_amd_split_complex.argtypes and f.restype is C.c_int
        args = (C.c_void_p(8), C.c_void_p(16), None, 1, 77, C.c_void_p(HANDLE))
        assert f(*args) == 0 and L.nd_amd_merge_complex(*args) == -3
        assert fake.nd_amd_split_complex.calls == [args] and fake.nd_amd_merge_complex.calls == [args]
        assert [(c.entry, c.verdict) for c in h.calls] == [('nd_amd_split_complex', HELD),
                                                           ('nd_amd_merge_complex', HELD)]
        assert h.calls[0].args == {'in': 8, 'out_re': 16, 'out_im': None, 'dtype': 1, 'n': 77, 'hip_stream': HANDLE}
        # types set through the proxy reach the function
        f.restype = C.c_long
        assert fake.nd_amd_split_complex.restype is C.c_long
        with pytest.raises(AttributeError):
            L.nd_amd_no_such_entry
    assert _lib._lib is fake


def test_the_stream_argument_is_checked_before_anything_is_enqueued(fake):
    timeline = FakeTimeline()
    with held_stream(CPU, 20.0, timeline=timeline) as h:
        for wrong in (C.c_void_p(None), C.c_void_p(HANDLE + 1), 0):
            with pytest.raises(AssertionError) as err:
                _lib.lib().nd_amd_split_complex(None, None, None, 0, 1, wrong)
            assert 'nd_amd_split_complex was handed the stream' in str(err.value)
        assert _lib.lib().nd_amd_split_complex(None, None, None, 0, 1, HANDLE) == 0        # a plain integer will do
    assert timeline.begun == 1 and len(fake.nd_amd_split_complex.calls) == 1 and len(h.calls) == 1


def test_verdicts():
    assert hs.classify(True, True) == WAITED and hs.classify(True, False) == WAITED
    assert hs.classify(False, True) == INCONCLUSIVE and hs.classify(False, False) == HELD


def test_held_waited_and_inconclusive_calls(fake):
    timeline = FakeTimeline([(False, False), (True,), (False, True), (False, False)])
    with held_stream(CPU, 20.0, timeline=timeline) as h:
        for _ in range(4):
            _lib.lib().nd_amd_split_complex(None, None, None, 0, 1, C.c_void_p(HANDLE))
        assert [c.verdict for c in h.calls] == [HELD, WAITED, INCONCLUSIVE, HELD]
        assert timeline.begun == 4 and timeline.compared == 3        # a call that waited is not compared
        with h.unheld():
            _lib.lib().nd_amd_split_complex(None, None, None, 0, 1, C.c_void_p(123))       # forwarded untouched
        assert len(h.calls) == 4 and timeline.begun == 4 and len(fake.nd_amd_split_complex.calls) == 5
        assert all(c.seconds >= 0 for c in h.calls)


def test_a_write_during_the_hold_is_reported(fake):
    def entry_writing(t, at):
        def fn(*args):
            t.view(-1)[at] = 3
            return 0
        return FakeFunction(fn, [C.c_void_p] * 2)

    with held_stream(CPU, 20.0, pattern=0x55, timeline=FakeTimeline()) as h:
        out = torch.empty((4, 5), dtype=torch.uint8)                    # poisoned and guard-banded by the canary
        counts = torch.zeros(7, dtype=torch.int64)                      # recorded only
        full = torch.full((3,), 2.5)
        pinned_like = torch.zeros(0)                                    # empty: not tracked
        assert h.wrapped == 1 and h.tracked_total == 3 and len(h.tracked()) == 3 and pinned_like.numel() == 0
        assert bool((out == 0x55).all()) and int(counts.sum()) == 0 and float(full[0]) == 2.5
        h.register('fake_out', entry_writing(out, 6), ('out', 'hip_stream'))
        h.register('fake_counts', entry_writing(counts, 2), ('out', 'hip_stream'))
        with pytest.raises(AssertionError) as err:
            _lib.lib().fake_out(None, HANDLE)
        msg = str(err.value)
        assert 'fake_out wrote memory while its stream was held' in msg and '(4, 5)' in msg and 'torch.uint8' in msg
        assert 'test_held_stream_cpu.py' in msg and 'test_a_write_during_the_hold_is_reported' in msg
        assert 'first at byte %d ' % (4096 + 6) in msg and '0x55 -> 0x03' in msg            # behind the guard band
        with pytest.raises(AssertionError) as err:
            _lib.lib().fake_counts(None, HANDLE)
        msg = str(err.value)
        assert 'fake_counts' in msg and 'torch.zeros' in msg and '(7,)' in msg and 'first at byte 16 ' in msg
        assert 'test_a_write_during_the_hold_is_reported' in msg
        # the same writes by a call that waited or was inconclusive are nobody's fault
        h.timeline.script = [(True,), (False, True)]
        out.fill_(0x55)
        assert _lib.lib().fake_out(None, HANDLE) == 0
        out.fill_(0x55)
        assert _lib.lib().fake_out(None, HANDLE) == 0
        assert [c.verdict for c in h.calls] == [HELD, HELD, WAITED, INCONCLUSIVE]
        h.check()
        assert h.tracked() == [] and h.timeline.finished == 1
        again = torch.zeros_like(counts)
        assert len(h.tracked()) == 1 and again.shape == counts.shape
    assert not hasattr(_lib._lib, 'fake_out')


def test_everything_is_restored_after_an_exception(fake):
    names = PATCHED + hs.RECORDED
    before = {name: getattr(torch, name) for name in names}
    with held_stream(CPU, 20.0, timeline=FakeTimeline()):
        assert all(getattr(torch, name) is not before[name] for name in names)
        assert isinstance(_lib._lib, hs.Proxy)
    assert all(getattr(torch, name) is before[name] for name in names) and _lib._lib is fake
    with pytest.raises(KeyError):
        with held_stream(CPU, 20.0, timeline=FakeTimeline()):
            torch.empty(3)
            raise KeyError('inside')
    assert all(getattr(torch, name) is before[name] for name in names) and _lib._lib is fake
    with pytest.raises(AssertionError):                         # a touched guard: restored all the same
        with held_stream(CPU, 20.0, timeline=FakeTimeline()):
            t = torch.empty(3)
            torch.as_strided(t, (4,), (1,))[3] = 0.0
    assert all(getattr(torch, name) is before[name] for name in names) and _lib._lib is fake
    with pytest.raises(RuntimeError):
        with held_stream(CPU, 20.0, timeline=FakeTimeline()):
            with held_stream(CPU, 20.0, timeline=FakeTimeline()):
                pass
    assert all(getattr(torch, name) is before[name] for name in names) and _lib._lib is fake
