"""Every entry point held to its stream: a proxy library for tests, in the style of tests/canary.py.

include/nd_amd.h promises that an entry enqueues its work on `hip_stream` and returns without synchronising.  On
torch's default stream, where the suite runs, a launch, memset or copy that lands on the null stream, or an entry
that waits where the header says it does not, changes nothing that a test compares.  Inside

    with held_stream(device, 20.0) as h:
        out = kernels.something(...)         # on the side stream S, which the block makes current
        ...compare out with its reference...
        h.check()                            # the canary's guards; releases what was tracked

the loaded library (nd_amd._lib._lib) is replaced by a proxy that forwards every attribute.  The entries whose
parameter list in include/nd_amd.h has `void *hip_stream` (stream_entries: parsed, not listed by hand) are wrapped.
For each call of one the proxy

  1. asserts that the stream argument is S's handle;
  2. waits for S (so that the snapshot is taken now, not behind an earlier hold), then on S: clones every tracked
     allocation (a snapshot), records ev0, enqueues torch.cuda._sleep (bounded: an entry that waits for its stream
     ends the wait after the delay) and records ev_held;
  3. forwards the call;
  4. ev_held already reached: the call took longer than the hold, it is WAITED;
  5. otherwise synchronises the default stream (misplaced null-stream work has then run) and, on the checking stream
     R behind ev0, compares every tracked allocation with its snapshot into one row per allocation (changed?, first
     changed byte), copied to pinned memory without blocking; waits for R's event alone: S is never touched and the
     device never synchronised;
  6. ev_held reached by now: INCONCLUSIVE (the hold was too short to judge), else HELD;
  7. a HELD call with a changed byte raises AssertionError: the entry, the allocation (its call site, as the canary
     reports it) and the first changed byte.  While S was provably still asleep nothing the call enqueued may have
     written anything.

Tracked: every device tensor that torch.empty, empty_like and empty_strided (through the canary, so outputs and
workspaces stay poisoned and guard-banded) and torch.zeros, zeros_like and full (recorded only) hand out inside the
block.  Tracked tensors and snapshots stay referenced until check() or the end of the block, both of which
synchronise S first.

A call that is slow on the host for reasons of its own (the first launch out of a code object, a first hipFFT plan,
a decision table built for a new series length) outlasts the hold exactly as one that waits for the stream does.
`with h.unheld():` forwards calls untouched; tests run every case once inside it, on S, before the judged run.

S and R are made once per device and used by every block: library state that is keyed by the stream is then built
once.  torch's pool streams do not synchronise with the null stream; step 5 relies on that.

This is a plain helper: no conftest, no plugin, no pytest setting."""
import collections
import contextlib
import os
import re
import time

import torch

from tests import canary as canary_module
from tests.canary import canary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nd_amd.h')
STREAM_PARAMETER = 'hip_stream'
RECORDED = ('zeros', 'zeros_like', 'full')          # initialised allocations the wrappers hand out: recorded only
HELD, WAITED, INCONCLUSIVE = 'held', 'waited', 'inconclusive'
MAX_TRACKED = 512
_HERE = os.path.abspath(__file__)
if _HERE not in canary_module.HELPERS:
    canary_module.HELPERS.append(_HERE)

Call = collections.namedtuple('Call', 'entry verdict args seconds check_seconds')


# ---- the header ----------------------------------------------------------------------------------------------------
def header_entries(path=HEADER):
    """{entry: [parameter names]} of every prototype of the header, comments removed"""
    with open(path) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\b(nd_amd_\w+)\s*\(([^()]*)\)\s*;', text):
        names = []
        for p in m.group(2).split(','):
            p = re.sub(r'(\[[^\]]*\])+\s*$', '', p.strip())
            ident = re.findall(r'[A-Za-z_]\w*', p)
            if ident and not (ident == ['void']):
                names.append(ident[-1])
        out[m.group(1)] = names
    return out


def stream_entries(path=HEADER):
    """{entry: [parameter names]} of the entries that take `void *hip_stream`"""
    return {name: params for name, params in header_entries(path).items() if STREAM_PARAMETER in params}


def classify(reached_after_call, reached_after_check):
    """the verdict from ev_held.query() behind the forwarded call and behind the comparison"""
    if reached_after_call:
        return WAITED
    return INCONCLUSIVE if reached_after_check else HELD


def _plain(v):
    """a ctypes scalar's value, anything else as it is"""
    return getattr(v, 'value', v) if not isinstance(v, (int, float)) else v


# ---- the hold on a real device -------------------------------------------------------------------------------------
_STREAMS = {}
_CYCLES_PER_MS = {}
_WARM = set()


def streams(device):
    """(S, R): the side stream the blocks make current and the checking stream, one pair per device"""
    key = torch.device(device)
    if key not in _STREAMS:
        _STREAMS[key] = (torch.cuda.Stream(key), torch.cuda.Stream(key))
    return _STREAMS[key]


def _sleep_ms(S, cycles):
    """milliseconds of one torch.cuda._sleep(cycles) on S between two events.  A sleep of the same length runs in
    front of the first event: the kernel is loaded by then, and the measured one is already enqueued when it starts,
    so no time the host takes between the launches is measured with it."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        a.record(S)
        torch.cuda._sleep(cycles)
        b.record(S)
    b.synchronize()
    return a.elapsed_time(b)


def calibrate(device):
    """cycles of torch.cuda._sleep per millisecond on `device`, measured once: two events around one sleep
    (_sleep_ms), lengthened tenfold (at most six times) until it lasts 2 ms, then once more at about 5 ms."""
    key = torch.device(device)
    if key in _CYCLES_PER_MS:
        return _CYCLES_PER_MS[key]
    S, _ = streams(key)
    cycles = 100000
    for _ in range(7):
        ms = _sleep_ms(S, cycles)
        if ms >= 2.0:
            break
        cycles *= 10
    assert ms > 0.05, 'torch.cuda._sleep(%d) lasted %.3f ms: no hold can be built from it' % (cycles, ms)
    cycles = max(1, int(5.0 * cycles / ms))
    ms = _sleep_ms(S, cycles)
    assert 2.0 < ms < 12.5, 'a sleep calibrated to 5 ms lasted %.3f ms' % ms
    _CYCLES_PER_MS[key] = cycles / ms
    return _CYCLES_PER_MS[key]


class DeviceTimeline(object):
    """steps 2, 4, 5 and 6 on a device.  begin(tracked) -> token, reached(token), compare(token) -> None or
    (index of the allocation, first changed byte, old value, new value)."""

    def __init__(self, device, delay_ms):
        self.device = torch.device(device)
        self.S, self.R = streams(self.device)
        self.cycles = int(calibrate(self.device) * delay_ms)
        self.stream_handle = self.S.cuda_stream
        self.pinned = torch.empty((MAX_TRACKED, 4), dtype=torch.int64, pin_memory=True)
        if self.device not in _WARM:
            # the comparison's own kernels, loaded before the first hold: their first launch would outlast it
            with torch.cuda.stream(self.S):
                a = torch.arange(4096, device=self.device).to(torch.uint8)
                token = {'tracked': [a, a[:7]], 'snaps': [a.clone(), a[:7] + 1], 'ev0': torch.cuda.Event()}
                token['ev0'].record(self.S)
            found = self.compare(token)
            self.S.synchronize()
            assert found == (1, 0, 1, 0), found
            _WARM.add(self.device)

    def begin(self, tracked):
        # S idle first: behind an earlier call's hold the snapshot would be taken late, after misplaced work of this
        # call had run, and would hold what that work wrote
        self.S.synchronize()
        with torch.cuda.stream(self.S):
            snaps = [t.clone() for t in tracked]
            ev0, held = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(self.S)
            torch.cuda._sleep(self.cycles)
            held.record(self.S)
        return {'tracked': list(tracked), 'snaps': snaps, 'ev0': ev0, 'held': held}

    def reached(self, token):
        return bool(token['held'].query())

    def compare(self, token):
        torch.cuda.default_stream(self.device).synchronize()
        n = len(token['tracked'])
        if n == 0:
            return None
        done = torch.cuda.Event()
        with torch.cuda.stream(self.R):
            self.R.wait_event(token['ev0'])
            rows = []
            for now, then in zip(token['tracked'], token['snaps']):
                ne = now != then
                at = ne.to(torch.uint8).argmax().view(1)          # the first of equal maxima; no read-back
                rows.append(torch.cat([ne.any().to(torch.int64).view(1), at, then.index_select(0, at).to(torch.int64),
                                       now.index_select(0, at).to(torch.int64)]))
            self.pinned[:n].copy_(torch.stack(rows), non_blocking=True)
            done.record(self.R)
        done.synchronize()
        host = self.pinned[:n].numpy()
        for i in range(n):
            if host[i, 0]:
                return i, int(host[i, 1]), int(host[i, 2]), int(host[i, 3])
        return None

    def finish(self):
        self.S.synchronize()

    def held_ms(self, token):
        """how long the hold of a call lasted; after finish()"""
        return token['ev0'].elapsed_time(token['held'])


# ---- the proxy -----------------------------------------------------------------------------------------------------
class _Entry(object):
    """one wrapped entry: called like the library's function, argtypes and restype are the function's own"""

    def __init__(self, name, target, params, owner):
        self.__dict__.update(_name=name, _target=target, _params=params, _owner=owner)

    def __call__(self, *args):
        return self._owner._call(self._name, self._target, self._params, args)

    def __getattr__(self, attr):
        return getattr(self._target, attr)

    def __setattr__(self, attr, value):
        setattr(self._target, attr, value)


class Proxy(object):
    """stands in for the ctypes library: every attribute is the library's own, the stream-taking entries wrapped"""

    def __init__(self, real, entries, owner):
        self.__dict__.update(_real=real, _entries=dict(entries), _owner=owner, _fakes={}, _wrapped={})

    def __getattr__(self, name):
        if name in self._fakes:
            target = self._fakes[name]
        else:
            target = getattr(self._real, name)
        if name not in self._entries:
            return target
        if name not in self._wrapped or self._wrapped[name]._target is not target:
            self._wrapped[name] = _Entry(name, target, self._entries[name], self._owner)
        return self._wrapped[name]

    def __setattr__(self, name, value):
        setattr(self._real, name, value)


class held_stream(object):
    """Context manager; see the module's docstring.  `calls`: a Call (entry, verdict, {parameter: value}, seconds on
    the host, seconds of the comparison) for every stream-taking call so far; `wrapped`: allocations the canary
    poisoned; `tracked_total`: every allocation tracked, the recorded ones included; `shortest_hold_ms`: the shortest
    hold measured so far.  timeline: steps 2 to 6 on something else than a device (the CPU tests); the default is
    DeviceTimeline(device, delay_ms)."""

    def __init__(self, device, delay_ms, pattern=0xFF, timeline=None, header=HEADER):
        self.device = torch.device(device)
        self.delay_ms = float(delay_ms)
        self.pattern = pattern
        self.timeline = timeline
        self.entries = stream_entries(header)
        self.calls = []
        self.tracked_total = 0
        self.shortest_hold_ms = None
        self.canary = None
        self.proxy = None
        self._own = []
        self._tokens = []
        self._orig = None
        self._real = None
        self._held = True
        self._stream_ctx = None

    # ---- entering and leaving --------------------------------------------------------------------------------------
    def __enter__(self):
        from nd_amd import _lib
        if self.timeline is None:
            self.timeline = DeviceTimeline(self.device, self.delay_ms)
        self._real = _lib.lib()
        if isinstance(self._real, Proxy):
            raise RuntimeError('held_stream blocks do not nest')
        self.S = getattr(self.timeline, 'S', None)
        self.R = getattr(self.timeline, 'R', None)
        self.canary = canary(self.pattern, device_types=(self.device.type,))
        self.canary.__enter__()
        try:
            self._orig = {name: getattr(torch, name) for name in canary_module.PATCHED + RECORDED}
            for name in canary_module.PATCHED:
                setattr(torch, name, self._counting(name))
            for name in RECORDED:
                setattr(torch, name, self._recording(name))
            self.proxy = Proxy(self._real, self.entries, self)
            _lib._lib = self.proxy
            if self.S is not None:
                self._stream_ctx = torch.cuda.stream(self.S)
                self._stream_ctx.__enter__()
        except BaseException:
            self._restore()
            self.canary.__exit__(RuntimeError, None, None)
            raise
        return self

    def _restore(self):
        from nd_amd import _lib
        if self._orig:
            for name, fn in self._orig.items():
                setattr(torch, name, fn)
        if self._real is not None:
            _lib._lib = self._real

    def __exit__(self, exc_type, exc, tb):
        try:
            if self._stream_ctx is not None:
                self._stream_ctx.__exit__(exc_type, exc, tb)
        finally:
            self._restore()
            try:
                if exc_type is None:
                    self.timeline.finish()
                    self._measure()
            finally:
                self._own, self._tokens = [], []
        return self.canary.__exit__(exc_type, exc, tb)

    # ---- tracking --------------------------------------------------------------------------------------------------
    def _counting(self, name):
        poisoned = self._orig[name]             # the canary's wrapper

        def counted(*args, **kwargs):
            before = self.canary.wrapped
            t = poisoned(*args, **kwargs)
            self.tracked_total += self.canary.wrapped - before
            return t
        counted.__name__ = name
        counted.__wrapped__ = poisoned
        return counted

    def _recording(self, name):
        orig = self._orig[name]

        def recorded(*args, **kwargs):
            t = orig(*args, **kwargs)
            if (isinstance(t, torch.Tensor) and t.device.type == self.device.type and t.numel() > 0
                    and not kwargs.get('pin_memory') and kwargs.get('out') is None and t.layout == torch.strided):
                whole = self._orig['empty'].__wrapped__(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
                self._own.append((whole, 'shape %s, %s, torch.%s at %s' % (tuple(t.shape), t.dtype, name,
                                                                          canary_module._call_site())))
                self.tracked_total += 1
            return t
        recorded.__name__ = name
        recorded.__wrapped__ = orig
        return recorded

    def tracked(self):
        """[(flat uint8 tensor of every byte, description)] of what is tracked now"""
        return self.canary.allocations() + list(self._own)

    @property
    def wrapped(self):
        return self.canary.wrapped

    def is_poison(self, t):
        return self.canary.is_poison(t)

    def check(self, release=True):
        """S synchronised, then the canary's guards; release: forget what was tracked and the snapshots"""
        self.timeline.finish()
        self._measure()
        try:
            self.canary.check(release=release)
        finally:
            if release:
                self._own, self._tokens = [], []

    def _measure(self):
        """the shortest hold so far into `shortest_hold_ms`, where the timeline can tell; S is synchronised"""
        if hasattr(self.timeline, 'held_ms'):
            for token in self._tokens:
                if not token.get('measured'):
                    token['measured'] = True
                    ms = self.timeline.held_ms(token)
                    self.shortest_hold_ms = ms if self.shortest_hold_ms is None else min(self.shortest_hold_ms, ms)

    # ---- the calls -------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def unheld(self):
        """calls inside are forwarded untouched and not listed in `calls`: see the module's docstring"""
        was, self._held = self._held, False
        try:
            yield
        finally:
            self._held = was

    def register(self, name, fn, params):
        """a fake entry `name` (a Python callable) with the parameter names `params`, for the positive controls"""
        self.proxy._fakes[name] = fn
        if STREAM_PARAMETER in params:
            self.proxy._entries[name] = list(params)

    def _call(self, name, target, params, args):
        if not self._held:
            return target(*args)
        at = params.index(STREAM_PARAMETER)
        given = (_plain(args[at]) or 0) if at < len(args) else None
        want = self.timeline.stream_handle
        assert given == want, ('%s was handed the stream %s: the current stream of the block is %s'
                               % (name, 'none' if given is None else hex(given), hex(want)))
        tracked = self.tracked()
        assert len(tracked) <= MAX_TRACKED, '%d allocations tracked at once: call check() between cases' % len(tracked)
        token = self.timeline.begin([t for t, _ in tracked])
        self._tokens.append(token)
        t0 = time.perf_counter()
        rv = target(*args)
        seconds = time.perf_counter() - t0
        diff = None
        after_call = self.timeline.reached(token)
        after_check = after_call
        t1 = time.perf_counter()
        if not after_call:
            diff = self.timeline.compare(token)
            after_check = self.timeline.reached(token)
        verdict = classify(after_call, after_check)
        named = {p: _plain(a) for p, a in zip(params, args)}
        self.calls.append(Call(name, verdict, named, seconds, time.perf_counter() - t1))
        if verdict == HELD and diff is not None:
            i, offset, old, new = diff
            raise AssertionError('%s wrote memory while its stream was held: the allocation (%s) changed, first at '
                                 'byte %d of it, 0x%02X -> 0x%02X.  The call enqueued work on another stream than '
                                 'the one it was given' % (name, tracked[i][1], offset, old, new))
        return rv
