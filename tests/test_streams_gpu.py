"""Every stream-taking entry of include/nd_amd.h on a held-back side stream, and two host threads on a stream each.

include/nd_amd.h: "Calls enqueue work on `hip_stream` and return without synchronising (exceptions are noted per
function)"; nd_amd/streaming.py and nd_amd/tiles.py overlap copies with kernels on the strength of it.  The rest of
the suite runs on torch's default stream from one host thread, where a launch, memset or copy on the null stream, an
entry that waits, or library-owned state shared between calls cannot change a compared value.  tests/held_stream.py
describes the hold; DESIGN.md, "State the library keeps between calls", says what orders each piece of such state.

  (a) cases the suite already passes, replayed inside held_stream and judged by each family's own rule against its
      own reference: the first 8 cases of every family of tools/fuzz_parity.py (seed of tests/test_fuzz_gpu.py;
      omnibus_long the first 4) and of tests/resample_cases.py, speckle_cases.py, regions_cases.py, rasterize and
      zonal_cases.py as their test_*_fuzz_gpu.py modules drive them, and the fixed cases of tests/fixed_cases.py.
      Every case runs once without the hold first (h.unheld(), on the same stream): first-use work on the host
      would otherwise outlast the hold and read as a wait.
  (b) WAITS below is the contract: the entries that may wait for their stream, each with its condition.  Every call
      classified `waited` must be in it under its condition, every other call must be `held`, none `inconclusive`;
      test_every_stream_taking_entry_was_seen requires the union of entries seen to be the header's whole set.
  (c) positive controls, fake entries registered with the proxy (harmless torch ops on initialised memory): a fill
      from a third stream is reported by entry and allocation site, a fill on S passes as held, S.synchronize() reads
      as waited, the default stream's handle fails the stream-argument check.
  (d) two host threads started by a barrier, a torch.cuda.Stream each and no hold, run the same seeded cases: the
      same shapes, hence the same cached tables and plans.

An exception from a device call that is not a comparison's verdict ends the test and makes every later test of this
module skip: the device may have faulted, and nothing more is started on it.  No retries, no subprocesses.

The hold: DELAY_MS = 20 ms of torch.cuda._sleep, calibrated once with two events around one sleep.  It is no
performance figure; it only has to outlast the host side of one call and the comparison behind it: 0.16 ms and
1.2 ms at the most in a run of the whole suite (the last test prints both, and the holds as measured).
Seconds on one MI355X (pytest --durations=0, call phase; the host's oracle and restatements and the run without the
hold included), with every measured hold between 19.9 and 20.0 ms, 457 held calls, 22 that waited, none inconclusive:
  seeded families    omnibus_long 2.5 (4 cases), omnibus 1.7, c3 1.2, zonal 1.0, c3_more 0.45, gaussian 0.44,
                     linear 0.42,
                     to_rgb, omnibus_ml and kmeans_step 0.36, change_segments 0.32, regions, forest and omnibus_diag
                     0.28, nlmeans 0.25, warp 0.22, knn, correlate and speckle 0.20, rasterize and resample 0.19,
                     kmeans_predict 0.18
  fixed cases        coregister_shifts 5.1 (the process's first hipFFT plans), relayout 2.4 (float32) and 2.2 (float64),
                     split / merge 0.49, classify_gather / class_stats / class_fill 0.25, feature_moments / gather_rows
                     0.17, region_sizes 0.15, resample_check_table 0.10, rgb_limits 0.04
  controls 0.06; threads: the newer families 0.36, the run_case families 0.11, coregister_shifts 0.03,
                     change_detection 0.01
The whole module: 25 s, 39 tests.  What waited: nd_amd_label_regions, nd_amd_sieve_regions and
nd_amd_resample_check_table in every call, nd_amd_omnibus_c2 and nd_amd_omnibus_diag beyond 96 dates; nothing else, the
classifier's entries with their pageable hipMemcpyAsync of the pointer table included (held in all 76 calls).
nd_amd_correlate beyond 128 taps and the long series of the other omnibus entries are in WAITS from reading: the first
cases of the generators do not reach them."""
import contextlib
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

from tests import fixed_cases, synth
from tests.held_stream import HELD, INCONCLUSIVE, WAITED, held_stream, stream_entries

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELAY_MS = 20.0
TROUBLE = []            # the first exception of a device call that was no comparison's verdict
SEEN = {}               # entry -> {verdict: calls}, over the whole module
SLOWEST = [0.0, 0.0]    # the longest host side of a held call and the longest comparison, in seconds
HOLDS = []              # the shortest measured hold of every block, in milliseconds

K_TAB_ARGS = 96         # nd_amd/csrc/omnibus_tables.hpp kTabArgs: the longest series whose table is a kernel argument
K_TAPS_ARGS = 128       # nd_amd/csrc/correlate.hip kTapsArgs: the taps that travel as a kernel argument


def _long_series(a):
    return a['k'] > K_TAB_ARGS


# the entries that may wait for their stream, and when (include/nd_amd.h, "Streams and threads")
WAITS = {
    'nd_amd_correlate': lambda a: a['ntaps'] > K_TAPS_ARGS,     # the tap list goes through a pageable host copy
    'nd_amd_omnibus_c2': _long_series,                          # stage_table (omnibus_common.hpp): the table likewise
    'nd_amd_omnibus_c2_pixel_major': _long_series,
    'nd_amd_omnibus_c3': _long_series,
    'nd_amd_omnibus_c3_pixel_major': _long_series,
    'nd_amd_omnibus_diag': _long_series,
    'nd_amd_resample_check_table': lambda a: True,              # reads its flag back
    'nd_amd_label_regions': lambda a: True,                     # reads the give-up word back
    'nd_amd_sieve_regions': lambda a: True,
}


@pytest.fixture(autouse=True)
def _nothing_after_trouble():
    if TROUBLE:
        pytest.skip('an earlier test of this module ended on %s: the device may have faulted, nothing more is started '
                    'on it' % TROUBLE[0])


@pytest.fixture(scope='module')
def fuzz(device, oracle):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fuzz_parity
    return fuzz_parity


@pytest.fixture(scope='module')
def K(device):
    from nd_amd import kernels
    return kernels


@contextlib.contextmanager
def device_calls(what):
    """an AssertionError is a verdict and passes through; any other exception is trouble: recorded, the test fails"""
    try:
        yield
    except AssertionError:
        raise
    except Exception as e:                  # noqa: BLE001
        TROUBLE.append('%s: %r' % (what, e))
        pytest.fail('%s raised %r: not a comparison\'s verdict, the rest of this module is skipped' % (what, e))


def note(calls):
    """the calls into SEEN, before anything is asserted of them: a failing test hides no entry from the last one"""
    for c in calls:
        SEEN.setdefault(c.entry, {}).setdefault(c.verdict, 0)
        SEEN[c.entry][c.verdict] += 1
        if c.verdict != WAITED:
            SLOWEST[:] = max(SLOWEST[0], c.seconds), max(SLOWEST[1], c.check_seconds)


def judge(what, calls):
    """(b): every call against WAITS"""
    bad = []
    for c in calls:
        shown = {p: v for p, v in c.args.items() if isinstance(v, (int, float))}
        if c.verdict == INCONCLUSIVE:
            bad.append('%s was inconclusive (%.1f ms on the host, %.1f ms for the comparison): the hold of %g ms is '
                       'too short' % (c.entry, 1e3 * c.seconds, 1e3 * c.check_seconds, DELAY_MS))
        elif c.verdict == WAITED and not (c.entry in WAITS and WAITS[c.entry](c.args)):
            bad.append('%s waited for its stream (%.1f ms on the host) and the contract does not allow it here: %s' %
                       (c.entry, 1e3 * c.seconds, shown))
        elif c.verdict not in (HELD, WAITED):
            bad.append('%s: %r' % (c.entry, c.verdict))
    assert not bad, '%s: %d of %d calls break the stream contract: %s' % (what, len(bad), len(calls), bad[:4])


def held_replay(what, device, count, one_case):
    """one_case(i) -> None, or what differs: once without the hold, then held.  The canary's guards are checked after
    every case; the calls of the held runs are judged by (b) at the end."""
    fails = []
    with device_calls(what), held_stream(device, DELAY_MS) as h:
        for i in range(count):
            try:
                with h.unheld():
                    why = one_case(i)
                h.check()
                why = why or one_case(i)
            except AssertionError as e:
                why = str(e) or 'assertion'
            try:
                h.check()
            except AssertionError as e:
                why = '%s%s' % (why + '; ' if why else '', e)
            if why:
                fails.append((i, why))
        tracked, calls = h.tracked_total, list(h.calls)
    HOLDS.extend(ms for ms in [h.shortest_hold_ms] if ms is not None)
    note(calls)
    assert tracked > 0, 'no allocation of %s was tracked: the hold compares nothing' % what
    assert calls, '%s called no stream-taking entry' % what
    assert not fails, '%d of %d %s cases fail on a held-back side stream: %s' % (len(fails), count, what, fails[:3])
    judge(what, calls)
    return calls


def held_fixed(what, device, body, allocations=True):
    """body(h): once without the hold, then held; (b) at the end"""
    with device_calls(what), held_stream(device, DELAY_MS) as h:
        with h.unheld():
            body(h)
        h.check()
        body(h)
        h.check()
        tracked, calls = h.tracked_total, list(h.calls)
    HOLDS.extend(ms for ms in [h.shortest_hold_ms] if ms is not None)
    note(calls)
    if allocations:
        assert tracked > 0, 'no allocation of %s was tracked: the hold compares nothing' % what
    assert calls, '%s called no stream-taking entry' % what
    judge(what, calls)
    return calls


# =====================================================================================================================
# (a) the seeded families
# =====================================================================================================================
FUZZ_SEED = 20261004                # tests/test_fuzz_gpu.py
FUZZ_CASES = {name: 8 for name in ('omnibus', 'omnibus_ml', 'c3', 'c3_more', 'omnibus_diag', 'change_segments',
                                   'nlmeans', 'correlate', 'gaussian', 'to_rgb', 'forest', 'kmeans_predict', 'knn',
                                   'linear', 'kmeans_step', 'warp')}
FUZZ_CASES['omnibus_long'] = 4
COUNT = 8


@pytest.mark.parametrize('family', sorted(FUZZ_CASES))
def test_held_fuzz_family(fuzz, device, family):
    def one(i):
        ok, desc = fuzz.CASES[family](np.random.default_rng([FUZZ_SEED, i]))
        return None if ok else 'differs from its reference: %s' % (desc,)
    held_replay(family, device, FUZZ_CASES[family], one)


def test_held_rasterize(fuzz, device):
    from nd_amd import vector                                   # noqa: F401  (the family needs the feature)
    seed = 20261019                 # tests/test_rasterize_fuzz_gpu.py

    def one(i):
        ok, desc = fuzz.CASES['rasterize'](np.random.default_rng([seed, i]))
        return None if ok else 'differs from the restatement: %s' % (desc,)
    held_replay('rasterize', device, COUNT, one)


def test_held_resample(K, device):
    from tests import resample_cases as cases, resample_ref as ref
    seed = 20261019                 # tests/test_resample_fuzz_gpu.py

    def one(i):
        case = cases.random_case(np.random.default_rng([seed, i]))
        args = (case['src'], case['tr_s'], case['tr_d'], case['H'], case['W'], case['method'])
        want = ref.regrid(*args, fill=case['fill'])
        got = cases.device_regrid(K, *args, case['layout'], fill=case['fill'], crop=case['crop'],
                                  strided_out=case['strided_out'])
        cases.assert_same(got, want, payloads=case['method'] == 'nearest')
    held_replay('resample', device, COUNT, one)


def test_held_speckle(K, device):
    from tests import speckle_cases as cases
    seed = 20261020                 # tests/test_speckle_fuzz_gpu.py

    def one(i):
        got, want = cases.run_case(K, cases.random_case(np.random.default_rng([seed, i])))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            cases.assert_same(g, w)
    held_replay('speckle', device, COUNT, one)


def test_held_regions(K, device):
    from tests import regions_cases as cases
    seed = 20261020                 # tests/test_regions_fuzz_gpu.py

    def one(i):
        got, want = cases.run_case(K, cases.random_case(np.random.default_rng([seed, i])))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            cases.assert_same(g, w)
    held_replay('regions', device, COUNT, one)


def test_held_zonal(K, device):
    from tests import zonal_cases as cases
    seed = 20261021                 # tests/test_zonal_fuzz_gpu.py

    def one(i):
        cases.run_case(K, cases.random_case(np.random.default_rng([seed, i])))
    held_replay('zonal', device, COUNT, one)


# =====================================================================================================================
# (a) the fixed cases of tests/fixed_cases.py
# =====================================================================================================================
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_held_relayout(K, device, dtype):
    held_fixed('relayout', device, lambda h: fixed_cases.relayout(K, device, dtype, h))


def test_held_split_and_merge_complex(K, device):
    held_fixed('split_complex / merge_complex', device, lambda h: fixed_cases.split_and_merge_complex(K, device, h))


def test_held_coregister_shifts(K, device):
    """the run without the hold also builds the hipFFT plans of the stream: seconds on the host in a fresh process"""
    held_fixed('coregister_shifts', device, lambda h: fixed_cases.coregister_shifts(K, device, h))


def test_held_classify_gather_class_stats_class_fill(K, device):
    held_fixed('classify_gather / class_stats / class_fill', device,
               lambda h: fixed_cases.classify_gather_class_stats_class_fill(K, device, h))


def test_held_feature_moments_and_gather_rows(K, device):
    held_fixed('feature_moments / gather_rows', device,
               lambda h: fixed_cases.feature_moments_and_gather_rows(K, device, h))


def test_held_rgb_limits(K, device):
    held_fixed('rgb_limits', device, lambda h: fixed_cases.rgb_limits(K, device, h))


def test_held_resample_check_table(K, device):
    """its flag is the library's own allocation: nothing of torch's to track, the entry always waits"""
    calls = held_fixed('resample_check_table', device, lambda h: fixed_cases.resample_check_table(K, device, h),
                       allocations=False)
    assert {c.entry for c in calls} == {'nd_amd_resample_check_table'}


def test_held_region_sizes(K, device):
    case = fixed_cases.region_sizes_case()
    calls = held_fixed('region_sizes', device, lambda h: fixed_cases.region_sizes_counted(K, device, case, h))
    assert {(c.entry, c.verdict) for c in calls} == {('nd_amd_region_sizes', HELD)}
    held_fixed('label_regions + region_sizes', device, lambda h: fixed_cases.region_sizes_labelled(K, device, case, h))


# =====================================================================================================================
# (c) positive controls
# =====================================================================================================================
def test_controls(device):
    """Four fake entries, each `int fake(void *out, void *hip_stream)`: without them a silent harness would prove
    nothing.  The memory they touch is initialised (the canary's pattern) and they only fill it."""
    import torch
    from nd_amd import _lib
    with device_calls('the controls'), held_stream(device, DELAY_MS) as h:
        handle = ctypes.c_void_p(h.S.cuda_stream)
        third = torch.cuda.Stream(device)       # torch hands out pool streams in turn: not S or R again
        if third.cuda_stream in (h.S.cuda_stream, h.R.cuda_stream):
            third = [s for s in (torch.cuda.Stream(device) for _ in range(3))
                     if s.cuda_stream not in (h.S.cuda_stream, h.R.cuda_stream)][0]
        t = torch.empty(1000, dtype=torch.float32, device=device)           # tracked: this line is its call site
        u = torch.zeros(300, dtype=torch.int32, device=device)              # tracked, recorded only
        assert h.tracked_total == 2 and h.wrapped == 1

        def stray_fill(out, stream):
            with torch.cuda.stream(third):
                u.fill_(7)
            third.synchronize()
            return 0

        def own_fill(out, stream):
            t.fill_(2.0)                        # on the current stream: S, behind the hold
            return 0

        def waits(out, stream):
            h.S.synchronize()
            return 0

        for name, fn in (('fake_stray_fill', stray_fill), ('fake_own_fill', own_fill), ('fake_waits', waits)):
            h.register(name, fn, ('out', 'hip_stream'))
        # 1. a write from a third stream while S sleeps
        with pytest.raises(AssertionError) as err:
            _lib.lib().fake_stray_fill(None, handle)
        msg = str(err.value)
        assert 'fake_stray_fill' in msg and 'test_streams_gpu.py' in msg and 'test_controls' in msg, msg
        assert 'torch.zeros' in msg and '(300,)' in msg and 'first at byte 0 ' in msg and '0x00 -> 0x07' in msg, msg
        assert h.calls[-1].entry == 'fake_stray_fill' and h.calls[-1].verdict == HELD
        # 2. the same write on S
        assert _lib.lib().fake_own_fill(None, handle) == 0
        assert h.calls[-1].entry == 'fake_own_fill' and h.calls[-1].verdict == HELD
        # 3. a wait for S
        assert _lib.lib().fake_waits(None, handle) == 0
        assert h.calls[-1].entry == 'fake_waits' and h.calls[-1].verdict == WAITED
        # 4. another stream's handle: refused before anything is enqueued
        before = len(h.calls)
        with pytest.raises(AssertionError) as err:
            _lib.lib().fake_own_fill(None, ctypes.c_void_p(torch.cuda.default_stream(device).cuda_stream))
        assert 'fake_own_fill was handed the stream' in str(err.value) and len(h.calls) == before
        h.check()
        assert float(t[0]) == 2.0 and int(u[0]) == 7
        assert [c.verdict for c in h.calls] == [HELD, HELD, WAITED]
    assert _lib.lib() is h._real and not hasattr(torch.empty, '__wrapped__')


# =====================================================================================================================
# (d) two host threads, a stream each, the same shapes
# =====================================================================================================================
STOP = threading.Event()


def in_two_threads(what, device, work):
    """work(which) -> result, run by two threads behind a barrier, each under its own torch.cuda.Stream.  A thread that
    raises anything but an AssertionError is trouble: the other thread is told (work reads STOP before each case)."""
    import torch
    barrier = threading.Barrier(2)
    results, errors = [None, None], [None, None]

    def run(which):
        try:
            torch.cuda.set_device(device)
            s = torch.cuda.Stream(device)
            barrier.wait(timeout=60)
            with torch.cuda.stream(s):
                results[which] = work(which)
            s.synchronize()
        except BaseException as e:          # noqa: BLE001
            errors[which] = e
            if not isinstance(e, AssertionError):
                STOP.set()
                barrier.abort()

    threads = [threading.Thread(target=run, args=(w,)) for w in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for e in errors:
        if e is not None and not isinstance(e, AssertionError):
            TROUBLE.append('%s: %r' % (what, e))
            pytest.fail('%s raised %r in a thread: not a comparison\'s verdict, the rest of this module is skipped'
                        % (what, e))
    for e in errors:
        if e is not None:
            raise e
    return results


class Stopped(AssertionError):
    """the other thread met trouble: this one ends before its next case"""


def each_case(count, one):
    out = []
    for i in range(count):
        if STOP.is_set():
            raise Stopped('the other thread raised')
        out.append(one(i))
    return out


def test_threads_newer_families(fuzz, device):
    """The families of tools/fuzz_parity.py that come in gen_ / want_ / run_ / compare_ pieces (its NEWER tuple), cases
    0 - 7: inputs and references on the main thread, run_ in both threads at once, compare_ afterwards.
    Shared state shows here only if the two threads happen to meet inside it: the test can catch such a defect by
    chance, never prove its absence, and it is not looped to raise the odds."""
    from nd_amd import vector                                   # noqa: F401  (rasterize needs the feature)
    fails = []
    for name in fuzz.NEWER:
        gen, want_of, run, compare = (getattr(fuzz, p + name) for p in ('gen_', 'want_', 'run_', 'compare_'))
        seed = 20261019 if name == 'rasterize' else FUZZ_SEED
        drawn = [gen(np.random.default_rng([seed, i])) for i in range(COUNT)]
        wants = [want_of(inp) for inp, _ in drawn]
        gots = in_two_threads(name, device, lambda which: each_case(COUNT, lambda i: run(drawn[i][0])))
        for which, got in enumerate(gots):
            for i in range(COUNT):
                if not compare(got[i], wants[i], drawn[i][0]):
                    fails.append((name, 'thread %d' % which, i, drawn[i][1]))
    assert not fails, '%d results of two concurrent threads differ from their references: %s' % (len(fails), fails[:3])


def test_threads_run_case_families(K, device):
    """resample, speckle, regions and zonal, cases 0 - 7 of each through the comparison of their fuzz modules, in both
    threads at once.
    Shared state shows here only if the two threads happen to meet inside it: the test can catch such a defect by
    chance, never prove its absence, and it is not looped to raise the odds."""
    from tests import regions_cases, resample_cases, resample_ref, speckle_cases, zonal_cases

    def resample(i):
        case = resample_cases.random_case(np.random.default_rng([20261019, i]))
        args = (case['src'], case['tr_s'], case['tr_d'], case['H'], case['W'], case['method'])
        got = resample_cases.device_regrid(K, *args, case['layout'], fill=case['fill'], crop=case['crop'],
                                           strided_out=case['strided_out'])
        want = resample_ref.regrid(*args, fill=case['fill'])
        resample_cases.assert_same(got, want, payloads=case['method'] == 'nearest')

    def pairs(cases, seed):
        def one(i):
            got, want = cases.run_case(K, cases.random_case(np.random.default_rng([seed, i])))
            assert len(got) == len(want)
            for g, w in zip(got, want):
                cases.assert_same(g, w)
        return one

    def zonal(i):
        zonal_cases.run_case(K, zonal_cases.random_case(np.random.default_rng([20261021, i])))

    for what, one in (('resample', resample), ('speckle', pairs(speckle_cases, 20261020)),
                      ('regions', pairs(regions_cases, 20261020)), ('zonal', zonal)):
        in_two_threads(what, device, lambda which: each_case(COUNT, one))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_threads_change_detection(K, oracle, device, dtype):
    """One dual-pol stack of 24 dates, 13 x 70 pixels, through kernels.change_detection in both threads at once,
    at a threshold of the fused and of the sparse regime: both maps equal the oracle's, byte for byte.
    Shared state shows here only if the two threads happen to meet inside it: the test can catch such a defect by
    chance, never prove its absence, and it is not looped to raise the odds."""
    planes = synth.omnibus_stack(seed=77, k=24, ny=13, nx=70, dtype=dtype, change_frac=0.3)
    yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
    alphas = (0.01, 0.99)
    wants = [oracle.change_detection_planes(yxt, a, 9, njobs=8, stats=False) for a in alphas]

    def work(which):
        dev = [fixed_cases.up(p, device) for p in planes]
        return each_case(len(alphas), lambda i: K.change_detection(*dev, alpha=alphas[i], n=9).cpu().numpy())
    for which, maps in enumerate(in_two_threads('change_detection', device, work)):
        for got, want, alpha in zip(maps, wants, alphas):
            want = want[0] if isinstance(want, (tuple, list)) else want
            assert got.dtype == np.uint8 and got.shape == want.shape
            assert int((got != want).sum()) == 0, ('%d map bytes differ' % (got != want).sum(), which, alpha)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_threads_coregister_shifts(K, device, dtype):
    """coregister_shifts on stacks of one shape (6 x 31 x 37, u = 7: tests/coreg_cases.py CASES[0]) and different
    planted shifts, one per thread, at once: each result by coreg_cases.check_shifts against tests/coreg_ref.py.  The
    hipFFT plans of a shape are cached per stream (nd_amd/csrc/coregister.hip): with one plan for both streams a
    transform could run on the other thread's stream.
    Shared state shows here only if the two threads happen to meet inside it: the test can catch such a defect by
    chance, never prove its absence, and it is not looped to raise the odds."""
    from tests import coreg_cases as cases
    ny, nx, u = cases.CASES[0]
    stacks = [cases.stack(cases.case_seed(ny, nx, u) + 1000 * (which + 1), cases.K, ny, nx, dtype)['C11']
              for which in (0, 1)]
    assert stacks[0].shape == stacks[1].shape and not np.array_equal(stacks[0], stacks[1])
    wants = [cases.decided_stack(s, 0, u) for s in stacks]

    def work(which):
        if STOP.is_set():
            raise Stopped('the other thread raised')
        sh, status = K.coregister_shifts(fixed_cases.up(stacks[which], device), 0, u)
        return sh.cpu().numpy(), status.cpu().numpy()
    for which, (got, status) in enumerate(in_two_threads('coregister_shifts', device, work)):
        assert (status == 0).all() and (got[0] == 0).all(), which
        cases.check_shifts(got, wants[which][0], wants[which][1], u, (ny, nx))


# =====================================================================================================================
# (b) no entry left out
# =====================================================================================================================
def test_every_stream_taking_entry_was_seen(device):
    """The union of entries the held tests of this module called is the header's set of stream-taking entries, every
    one of them classified at least once, and what waited is in WAITS.  Needs the whole module to have run."""
    want = set(stream_entries())
    seen = {e for e in SEEN if not e.startswith('fake_')}
    for e in sorted(SEEN):
        print(e, SEEN[e])
    print('of the hold of %g ms, the longest call took %.2f ms on the host and the longest comparison %.2f ms'
          % (DELAY_MS, 1e3 * SLOWEST[0], 1e3 * SLOWEST[1]))
    print('the measured holds: %.2f ms at the least, %.2f ms at the most' % (min(HOLDS), max(HOLDS)))
    assert min(HOLDS) > 0.8 * DELAY_MS, 'a hold of %g ms lasted %.2f ms: calibration is off' % (DELAY_MS, min(HOLDS))
    assert set(WAITS) <= want, sorted(set(WAITS) - want)
    assert seen == want, 'never called on a held stream: %s; unknown to the header: %s' % (sorted(want - seen),
                                                                                           sorted(seen - want))
    assert not [e for e in seen if INCONCLUSIVE in SEEN[e]]
    assert {e for e in seen if WAITED in SEEN[e]} <= set(WAITS)
    assert all(HELD in SEEN[e] or e in WAITS for e in seen), sorted(e for e in seen if HELD not in SEEN[e])
