"""Every kernel family on poisoned, guard-banded scratch memory (tests/canary.py).

nd_amd's wrappers hand the library outputs and workspaces from torch.empty / empty_like / empty_strided.  In a pytest
process that memory is usually zeros, or the correct result of the previous, identically shaped case; here every such
allocation is filled with 0xFF (NaN, -1, 255) and then with 0x55 (1.5e13, 1431655765, 85) and a contiguous one lies
between two 4 KiB guard bands.  Cases the suite already passes are replayed with nothing else changed and judged by
the family's own rule against its own reference (the CPU oracle or the numpy restatements under tests/, never a
second run of the device code): an output element no kernel writes, a counter or list nobody zeroes on the call's
stream, or a write past the bytes a *_workspace_bytes entry reported now changes a compared value or a guard band.
DESIGN.md, "Memory the library is handed uninitialised", says for every region who initialises it; it was written
from the code before these tests first ran.

  * the seeded families: the first 32 cases of every family of tools/fuzz_parity.py (seed and indices of
    tests/test_fuzz_gpu.py and tests/test_rasterize_fuzz_gpu.py; omnibus_long, at 0.25 s a case, the first 8) and of
    tests/resample_cases.py, speckle_cases.py, regions_cases.py and zonal_cases.py as their test_*_fuzz_gpu.py modules
    drive them;
  * fixed cases, with references written inline (tests/fixed_cases.py holds the bodies that tests/test_streams_gpu.py
    runs too), for the entries no generator reaches: the three relayout entries in
    every staging class of relayout.hip, split_complex / merge_complex, coregister_shifts, classify_gather,
    class_stats, class_fill, feature_moments, gather_rows, rgb_limits, polygon_boxes, resample_check_table,
    region_sizes and the z / P rasters of the omnibus wrappers;
  * the regimes of the three omnibus dispatchers, from the parameter lists of tests/test_omnibus_gpu.py, with the
    kernel labels each call launched: the union must be what is reachable at these sizes (see the three tests);
  * where the contract leaves part of an output unwritten, exactly that part still holds the pattern: outside `core`
    in pixelwise_nlmeans_3d, the padding of strided out= tensors and of pitched relayout planes, the other half of a
    complex destination, the planes behind the ones a label_regions call was given.

Every test asserts that the canary wrapped at least one allocation during its device calls: a wrapper that stops
allocating through torch would otherwise turn its test into a no-op.  polygon_boxes (host only), resample_check_table
(its flag is the library's own allocation) and region_sizes (torch.zeros) get no uninitialised memory from torch at
all: their tests assert exactly that, so that a change of it is noticed here.

An exception from a device call that is not a comparison's verdict ends the test and makes every later test of this
module skip: the device may have faulted, and nothing more is started on it.  No retries, no subprocesses.

Seconds on one MI355X (pytest --durations=0, call phase, the slower of the two patterns; the host's oracle and
restatements included):
  seeded families    omnibus 1.8, omnibus_long 1.7 (8 cases), c3 1.2, c3_more 0.8, omnibus_ml 0.35, change_segments 0.35,
                     zonal 0.38, omnibus_diag 0.3, gaussian 0.25, nlmeans 0.15, rasterize 0.11, regions 0.11, knn 0.09,
                     warp 0.08, kmeans_step 0.07, forest 0.06, resample 0.06, correlate 0.05, speckle 0.05, to_rgb 0.04,
                     linear 0.04, kmeans_predict 0.03
  fixed cases        coregister_shifts 5.0 in the first pattern, under 0.01 in the second: the process's first hipFFT
                     plans and the restatement's shifts, which tests/test_coregister_edges_gpu.py then finds cached;
                     stats rasters 0.33, relayout 0.17 (float32) and 0.10 (float64), every other one 0.01 or less
  regimes            dual-pol 1.4 in the first pattern (the stacks and the oracle's maps, computed once), 0.05 in the
                     second; full-pol 0.16, diagonal 0.12
  unwritten parts    0.01 each
The whole module: 25 s, 78 tests."""
import contextlib
import os
import sys

import numpy as np
import pytest

from tests import fixed_cases, synth
from tests.canary import PATTERNS, canary
from tests.fixed_cases import up

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_IDS = ['0x%02X' % p for p in PATTERNS]
TROUBLE = []            # the first exception of a device call that was no comparison's verdict


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
    """an AssertionError is a verdict and passes through; any other exception is trouble: recorded, and the test fails"""
    try:
        yield
    except AssertionError:
        raise
    except Exception as e:                  # noqa: BLE001
        TROUBLE.append('%s: %r' % (what, e))
        pytest.fail('%s raised %r: not a comparison\'s verdict, the rest of this module is skipped' % (what, e))


def replay(what, pattern, count, one_case):
    """one_case(i) -> None, or what differs.  The guards are checked after every case; a touched guard is a failure
    of that case, with the canary's message."""
    fails = []
    with device_calls(what), canary(pattern) as c:
        for i in range(count):
            try:
                why = one_case(i)
            except AssertionError as e:
                why = str(e) or 'assertion'
            try:
                c.check()
            except AssertionError as e:
                why = '%s%s' % (why + '; ' if why else '', e)
            if why:
                fails.append((i, why))
        seen = c.wrapped
    assert seen > 0, 'the canary saw no allocation of %s: the test checks nothing' % what
    assert not fails, '%d of %d %s cases fail on memory filled with 0x%02X: %s' % (len(fails), count, what, pattern,
                                                                                   fails[:3])


def fixed(what, pattern, body, allocations=True):
    """body(c) under the canary; its guards checked; it must have seen an allocation (or, allocations=False, none)"""
    with device_calls(what), canary(pattern) as c:
        body(c)
        c.check()
        seen = c.wrapped
    if allocations:
        assert seen > 0, 'the canary saw no allocation of %s: the test checks nothing' % what
    else:
        assert seen == 0, '%s now takes uninitialised memory from torch: give it a real check here' % what


# =====================================================================================================================
# the seeded families
# =====================================================================================================================
FUZZ_SEED = 20261004                # tests/test_fuzz_gpu.py
# tests/test_fuzz_gpu.py records omnibus_long at about 20 s for 80 cases (193 - 4096 dates, most of it the oracle): 8
FUZZ_CASES = {name: 32 for name in ('omnibus', 'omnibus_ml', 'c3', 'c3_more', 'omnibus_diag', 'change_segments',
                                    'nlmeans', 'correlate', 'gaussian', 'to_rgb', 'forest', 'kmeans_predict', 'knn',
                                    'linear', 'kmeans_step', 'warp')}
FUZZ_CASES['omnibus_long'] = 8


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize('family', sorted(FUZZ_CASES))
def test_fuzz_family(fuzz, family, pattern):
    def one(i):
        ok, desc = fuzz.CASES[family](np.random.default_rng([FUZZ_SEED, i]))
        return None if ok else 'differs from its reference: %s' % (desc,)
    replay(family, pattern, FUZZ_CASES[family], one)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_fuzz_rasterize(fuzz, pattern):
    from nd_amd import vector                                   # noqa: F401  (the family needs the feature)
    seed = 20261019                 # tests/test_rasterize_fuzz_gpu.py

    def one(i):
        ok, desc = fuzz.CASES['rasterize'](np.random.default_rng([seed, i]))
        return None if ok else 'differs from the restatement: %s' % (desc,)
    replay('rasterize', pattern, 32, one)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_fuzz_resample(K, pattern):
    from tests import resample_cases as cases, resample_ref as ref
    seed = 20261019                 # tests/test_resample_fuzz_gpu.py

    def one(i):
        case = cases.random_case(np.random.default_rng([seed, i]))
        args = (case['src'], case['tr_s'], case['tr_d'], case['H'], case['W'], case['method'])
        want = ref.regrid(*args, fill=case['fill'])
        got = cases.device_regrid(K, *args, case['layout'], fill=case['fill'], crop=case['crop'],
                                  strided_out=case['strided_out'])
        cases.assert_same(got, want, payloads=case['method'] == 'nearest')
    replay('resample', pattern, 32, one)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_fuzz_speckle(K, device, pattern):
    """tests/speckle_cases.py hands every call an `out` it filled itself: only the workspace of the two-pass form is
    the library's to initialise there.  Each case therefore runs a second time with out=None, the wrapper's own
    uninitialised output in the input's memory order, against the same restatement."""
    import torch
    from tests import speckle_cases as cases
    seed = 20261020                 # tests/test_speckle_fuzz_gpu.py

    def one(i):
        case = cases.random_case(np.random.default_rng([seed, i]))
        got, want = cases.run_case(K, case)
        v = case['variables']
        ups = [cases._upload(torch, device, a, case['layout']) for a in v]
        if case['filter'] == 'lee':
            own = [K.speckle_lee(ups[0][0], case['w'], case['looks'], case['method'], dims=ups[0][1])]
        else:
            own = K.speckle_multitemporal([u[0] for u in ups], case['w'], dims=ups[0][1])
        got = list(got) + [cases._download(o, ups[0][2], v[0].shape) for o in own]
        for g, w in zip(got, list(want) * 2):
            cases.assert_same(g, w)
    replay('speckle', pattern, 32, one)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_fuzz_regions(K, pattern):
    from tests import regions_cases as cases
    seed = 20261020                 # tests/test_regions_fuzz_gpu.py

    def one(i):
        case = cases.random_case(np.random.default_rng([seed, i]))
        got, want = cases.run_case(K, case)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            cases.assert_same(g, w)
    replay('regions', pattern, 32, one)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_fuzz_zonal(K, pattern):
    """zonal_index, zonal_stats and zonal_paint: the keys, the permutation and the offsets, the seven tables of every
    plane and the workspace of the tree are all the wrappers' own uninitialised memory; run_case compares them bit for
    bit with tests/zonal_ref.py."""
    from tests import zonal_cases as cases
    seed = 20261021                 # tests/test_zonal_fuzz_gpu.py

    def one(i):
        cases.run_case(K, cases.random_case(np.random.default_rng([seed, i])))
    replay('zonal', pattern, 32, one)


# =====================================================================================================================
# entries no generator reaches (the bodies: tests/fixed_cases.py, which tests/test_streams_gpu.py runs too)
# =====================================================================================================================
@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_relayout_in_every_staging_class(K, device, dtype, pattern):
    """relayout_planar, relayout_planar_complex and relayout_pixel_major are copies: every destination element equals
    its source element bit for bit (numpy's moveaxis is the reference), for real sources and for the .real / .imag
    halves of a complex one.  Destination planes have a pitch of ny * nx + 5: the padding keeps the pattern.  A
    complex destination of relayout_pixel_major keeps the pattern in the half that was not written.  One series
    length per staging class (pixels_per_block), the first of each: tests/test_api_gpu.py stops at 700 dates, so
    the classes of 8, 4, 2 and 1 pixels per block run nowhere else."""
    fixed('relayout', pattern, lambda c: fixed_cases.relayout(K, device, dtype, c))


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_split_and_merge_complex(K, device, pattern):
    """split_complex and merge_complex move values unchanged: numpy's .real / .imag are the reference, bit for bit.
    Lengths around the four values a thread moves and the 1024 a block moves."""
    fixed('split_complex / merge_complex', pattern, lambda c: fixed_cases.split_and_merge_complex(K, device, c))


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_coregister_shifts(K, device, pattern):
    """One small stack per type of tests/coreg_cases.py (31 x 37, u = 7: prime sizes) against tests/coreg_ref.py by the
    near-tie rule of that module: its workspace holds the staged stack, two spectra, the argmax partials, the DFT
    tables and the upsampled region, all uninitialised."""
    fixed('coregister_shifts', pattern, lambda c: fixed_cases.coregister_shifts(K, device, c))


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_classify_gather_class_stats_class_fill(K, device, pattern):
    """classify_gather against classify_ref.make_Xy (the kept rows in row order, bit for bit; mask = kept),
    class_stats against per-class numpy sums -- exact: the values are multiples of 1 / 256, so a float64 sum of them
    is the same in any order -- and class_fill against its definition in kernels.py restated with numpy.where.
    37 x 67 = 2479 rows: several blocks, the last one partial."""
    fixed('classify_gather / class_stats / class_fill', pattern,
          lambda c: fixed_cases.classify_gather_class_stats_class_fill(K, device, c))


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_feature_moments_and_gather_rows(K, device, pattern):
    """feature_moments against kmeans_fit_ref.moments by the rule of check_moments (tests/test_kmeans_fit_gpu.py, as
    tools/fuzz_parity.py restates it): the count equal, mean and variance within rows * 2^-52 of the magnitudes
    behind them.  gather_rows against numpy indexing, bit for bit: NaN rows and valid = 0 for indices outside."""
    fixed('feature_moments / gather_rows', pattern, lambda c: fixed_cases.feature_moments_and_gather_rows(K, device, c))


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_rgb_limits(K, device, pattern):
    """rgb_limits on three channels, one of them a quotient, against rgb_ref.limits by the rule of
    tests/test_to_rgb_cpu.py (equal values of the data type, NaN where NaN); the counts equal.  `limits` is the
    uninitialised output, the workspace holds the selection state and the histograms of every pass."""
    fixed('rgb_limits', pattern, lambda c: fixed_cases.rgb_limits(K, device, c))


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_polygon_boxes_and_a_table(K, device, pattern):
    """polygon_boxes runs on the host alone (no allocation to see): its boxes against the definition in its
    docstring, polygon by polygon.  The table built from them then burns into the wrapper's own uninitialised raster
    and owner workspace, against rasterize_ref.burn, the same bytes everywhere."""
    from tests import rasterize_cases as cases, rasterize_ref as ref
    rng = np.random.default_rng(10)
    ny, nx = 41, 77
    polys = [cases.random_polygon(rng, ny, nx, hole=bool(i % 2), m=[3, 7, 64, 65][i % 4]) for i in range(9)]
    polys.insert(4, [])
    polys.append([np.array([[-30.0, -20.0], [-10.0, -20.0], [-10.0, -5.0]])])      # off the raster
    verts, ro, po = ref.pack(polys)

    def boxes_only(c):
        boxes, row_work = K.polygon_boxes(verts, ro, po, ny, nx)
        for p, rings in enumerate(polys):
            want = np.zeros(4, np.int32)
            if rings:
                v = np.concatenate(rings)
                lo = [np.clip(np.floor(v[:, a].min() - 0.5), 0, n) for a, n in ((1, ny), (0, nx))]
                hi = [max(l, np.clip(np.floor(v[:, a].max() - 0.5) + 2, 0, n)) for l, (a, n) in zip(lo, ((1, ny), (0, nx)))]
                if hi[0] > lo[0] and hi[1] > lo[1]:
                    want = np.array([lo[0], hi[0], lo[1], hi[1]], np.int32)
            assert np.array_equal(boxes[p], want), (p, boxes[p], want)
        assert np.array_equal(row_work, np.concatenate([[0], np.cumsum(boxes[:, 1].astype(np.int64) - boxes[:, 0])]))
    fixed('polygon_boxes', pattern, boxes_only, allocations=False)

    def burned(c):
        for values, fill in ((np.arange(1, len(polys) + 1), -1), (np.arange(len(polys)) + 0.5, np.nan)):
            layer = np.arange(len(polys)) % 2
            got = K.rasterize_polygons(K.PolygonTable(verts, ro, po, ny, nx, device=device), None, None, values, ny, nx,
                                       layer=layer, nlayers=2, fill=fill)
            want = ref.burn(polys, values, ny, nx, layer=layer, nlayers=2, fill=fill)
            g = got.cpu().numpy()
            assert g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes()
    fixed('rasterize_polygons with a PolygonTable', pattern, burned)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_resample_check_table(K, device, pattern):
    """resample_check_table accepts what resample_axis builds and refuses a run that leaves its axis.  Its flag is
    memory the library allocates and zeroes itself: the canary must see nothing."""
    fixed('resample_check_table', pattern, lambda c: fixed_cases.resample_check_table(K, device, c), allocations=False)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_region_sizes(K, device, pattern):
    """region_sizes counts into a torch.zeros tensor that the library zeroes again itself (regions.hip, the memset in
    front of regions_sizes_kernel): no uninitialised memory of torch's, which the first part asserts on labels
    uploaded from the restatement.  The second part labels on the device first (poisoned labels and workspace) and
    counts those labels: regions_ref.sizes is the reference both times."""
    case = fixed_cases.region_sizes_case()
    fixed('region_sizes', pattern, lambda c: fixed_cases.region_sizes_counted(K, device, case, c), allocations=False)
    fixed('label_regions + region_sizes', pattern, lambda c: fixed_cases.region_sizes_labelled(K, device, case, c))


def close_stats(res, want, p_atol):
    """maps equal, z within 1e-5 relative, P within 1e-5 relative and p_atol: the rule of tools/fuzz_parity.py"""
    got = [t.cpu().numpy() for t in res]
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0]), '%d map bytes differ' % (got[0] != want[0]).sum()
    with np.errstate(all='ignore'):
        assert np.allclose(got[1], want[1], rtol=1e-5, atol=0, equal_nan=True), 'z differs'
        assert np.allclose(got[2], want[2], rtol=1e-5, atol=p_atol, equal_nan=True), 'P differs'


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_stats_rasters_of_the_omnibus_wrappers(K, fuzz, oracle, device, pattern):
    """stats=True: z and P are two more uninitialised outputs.  Each wrapper at a threshold of the fused and of the
    sparse regime, 24 x 131 pixels (ragged last block), against the oracle (dual-pol, multilooked, full-pol) or the
    restatement (diagonal) by the rules of tools/fuzz_parity.py.  The generators' own cases draw stats at random;
    these do not depend on the draw."""
    import scipy.ndimage as ndi

    def body(c):
        ny, nx = 24, 131
        for dtype, k in ((np.float32, 12), (np.float64, 9), (np.float32, 40)):
            planes = synth.omnibus_stack(seed=70 + k, k=k, ny=ny, nx=nx, dtype=dtype, change_frac=0.3)
            yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
            for alpha in (0.01, 0.99):
                want = oracle.change_detection_planes(yxt, alpha, 9, njobs=8, stats=True)
                close_stats(K.change_detection(*[up(p, device) for p in planes], alpha=alpha, n=9, stats=True), want, 1e-7)
                if k <= 24:
                    res = K.change_detection_pixel_major(*[up(a, device) for a in yxt], alpha=alpha, n=9, stats=True)
                    assert res is not None
                    close_stats(res, want, 1e-7)
                c.check()
        planes = synth.omnibus_stack(seed=71, k=9, ny=ny, nx=nx, dtype=np.float32, change_frac=0.3)
        kern = (np.ones((3, 3), dtype=np.float64) / 9).reshape(1, 3, 3)
        mlp = [np.ascontiguousarray(np.moveaxis(ndi.convolve(p, kern), 0, -1)) for p in planes]
        for alpha in (0.01, 0.99):
            want = oracle.change_detection_planes(mlp, alpha, 9, njobs=8, stats=True)
            res = K.change_detection_multilooked(*[up(p, device) for p in planes], alpha=alpha, ml=3, stats=True)
            assert res is not None
            close_stats(res, want, 1e-7)
            c.check()
        # full-pol and diagonal: the generators' cases 0 .. 5 with stats forced on, in every layout they draw
        for i in range(6):
            for name in ('c3', 'omnibus_diag'):
                inp, desc = getattr(fuzz, 'gen_' + name)(np.random.default_rng([FUZZ_SEED, i]))
                inp['stats'] = True
                want = getattr(fuzz, 'want_' + name)(inp)
                got = getattr(fuzz, 'run_' + name)(inp)
                assert 'z' in got and 'P' in got
                assert getattr(fuzz, 'compare_' + name)(got, want, inp), (name, desc)
            c.check()
    fixed('the stats=True forms', pattern, body)


# =====================================================================================================================
# the regimes of the omnibus dispatchers
# =====================================================================================================================
def launched(call):
    """the kernel labels `call` launched, as tests/test_omnibus_diag_gpu.py records them"""
    from nd_amd import _lib
    _lib.timing_enable(64)
    try:
        res = call()
        return res, {name for name, _ in _lib.timing_collect()}
    finally:
        _lib.timing_enable(0)


def planted_for_pass_b(dtype, k):
    """the stack of test_pass_b_one_lane_per_segment_start (tests/test_omnibus_gpu.py), 30 x 90 pixels"""
    planes = [p.copy() for p in synth.omnibus_stack(seed=900 + k, k=k, ny=30, nx=90, dtype=dtype, change_frac=0.3)]
    planes[1][:, 3, 5:45] = 0.9995 * np.sqrt(planes[0][:, 3, 5:45] * planes[3][:, 3, 5:45])    # nearly singular
    planes[2][:, 3, 5:45] = 0
    for p in planes:
        p[:, 7, 10:50] *= dtype(2.0 ** (-480.0 / k))
        p[:, 11, 10:50] *= dtype(2.0 ** (460.0 / k))
    planes[1][:, 20, 17] *= 6.0
    planes[0][k // 2, 21, 33] = np.nan
    for p in planes:
        p[:, 22, 44] = 0.0
    return planes


def planted_for_the_sparse_regime(dtype, k):
    """the stack of test_long_series_sparse_regime (tests/test_omnibus_gpu.py), 5 x 333 pixels"""
    rng = np.random.default_rng(k)
    planes = [p.copy() for p in synth.omnibus_stack(seed=700 + k, k=k, ny=5, nx=333, dtype=dtype, change_frac=0.25)]
    planes[1][:, 0, 10:40] *= 6.0
    planes[0][:, 1, 5:25] *= -1.0
    for p in planes:
        p[:, 2, 0:60] *= 1e-12
        p[:, 2, 60:120] *= 1e10
        p[k // 2:, 3, 0:50] *= 1e-9
        p[:, 3, 100:130] = 0.0
        p[:, 3, 130:160] = np.nan
    planes[3][k - 1, 4, 0:30] = np.inf
    planes[2][0, 4, 30:60] = np.nan
    for val in (0.0, -1.0):
        m = rng.random(planes[0].shape) < 0.002
        planes[int(rng.integers(0, 4))][m] = val
    return planes


SHARED = {}             # host-side cases and references, computed once for both patterns and left unchanged


def c2_regime_cases(oracle):
    """[(source test, planes, [(alpha, n, workspace, stats)], {(alpha, n): the oracle's map, z, P})] from the parameter
    lists of tests/test_omnibus_gpu.py"""
    if 'c2' in SHARED:
        return SHARED['c2']
    f32, f64 = np.float32, np.float64
    out = []
    # test_series_length_boundaries (24 x 323, n = 9, with the rasters): both sides of 16 / 24 / 32 / 48, and 8
    for k, dtype in ((8, f32), (17, f64), (24, f32), (33, f32), (49, f64)):
        planes = synth.omnibus_stack(seed=41 + k, k=k, ny=24, nx=323, dtype=dtype, change_frac=0.3)
        out.append(('boundaries', planes, [(a, 9, 'recommended', True) for a in (0.01, 0.5, 0.99)]))
    # test_long_series_at_low_thresholds (no rasters)
    for dtype, k in ((f32, 64), (f64, 17), (f32, 129)):
        planes = synth.omnibus_stack(seed=300 + k, k=k, ny=24 if k <= 64 else 6, nx=200, dtype=dtype, change_frac=0.3)
        out.append(('low thresholds', planes, [(a, 9, 'recommended', False) for a in (1e-4, 0.01, 0.2)]))
    # test_long_series_sparse_regime: the time-split pass A, both workspaces
    for dtype, k in ((f32, 49), (f32, 192), (f64, 25)):
        out.append(('sparse regime', planted_for_the_sparse_regime(dtype, k),
                    [(a, 9, ws, False) for a in (0.8, 0.99) for ws in ('recommended', 'minimal')]))
    # test_pass_b_one_lane_per_segment_start
    for dtype, k, alpha in ((f32, 130, 0.01), (f32, 12, 0.99), (f64, 12, 0.99)):
        out.append(('segment starts', planted_for_pass_b(dtype, k), [(alpha, 9, 'recommended', False)]))
    # test_minimal_workspace_gathers_from_planes: the other layout of the same buffer
    for dtype in (f32, f64):
        planes = synth.omnibus_stack(seed=17, k=9, ny=30, nx=90, looks=2, dtype=dtype, change_frac=0.3)
        out.append(('minimal workspace', planes, [(a, n, ws, False) for a, n in ((0.9, 9), (0.01, 1), (0.5, 1))
                                                  for ws in ('minimal', 'recommended')]))
    cases = []
    for source, planes, calls in out:
        yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
        with np.errstate(all='ignore'):
            wants = {key: oracle.change_detection_planes(yxt, key[0], key[1], njobs=8, stats=True)
                     for key in sorted({(a, n) for a, n, _, _ in calls})}
        cases.append((source, planes, calls, wants))
    SHARED['c2'] = cases
    return cases


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_dual_pol_regimes(K, oracle, device, pattern):
    """The regimes of omnibus_c2_impl (nd_amd/csrc/omnibus.hip) on poisoned workspaces and maps, against the oracle:
    the change map byte for byte, z and P (where asked for) within 1e-5 relative, as tests/test_omnibus_gpu.py
    compares them.  Cases: c2_regime_cases.  The labels launched, over all of them, must be exactly

        omnibus_c2_global   the plain, retaining, wave-search and time-split pass A (the sparse regime, or the rasters)
        omnibus_c2_fused    the chain and streaming searches inside pass A (alpha < 0.93 in registers, < 0.75 streaming)
        omnibus_c2_dense    behind a retaining pass A outside the fused regime (k <= 48 float32, 24 float64)
        omnibus_c2_search   pass B: segment starts of short lists, the chain form, the sweeps
        omnibus_c2_exact    the exact form behind a register form of pass B

    omnibus_c2_sample is not reachable at these sizes: take_sample returns before its launch unless the raster has
    at least 4096 blocks of 256 pixels (a megapixel), and tests stay far below."""
    seen = set()
    cases = c2_regime_cases(oracle)

    def body(c):
        for source, planes, calls, wants in cases:
            dev = [up(p, device) for p in planes]
            for alpha, n, ws, stats in calls:
                want = wants[alpha, n]
                what = (source, planes[0].dtype.name, planes[0].shape, alpha, n, ws, stats)
                res, names = launched(lambda: K.change_detection(*dev, alpha=alpha, n=n, stats=stats, workspace=ws))
                assert names, what
                seen.update(names)
                got = (res[0] if stats else res).cpu().numpy()
                assert got.dtype == np.uint8 and got.shape == want[0].shape
                assert int((got != want[0]).sum()) == 0, ('%d map bytes differ' % (got != want[0]).sum(), what)
                if stats:
                    np.testing.assert_allclose(res[1].cpu().numpy(), want[1], rtol=1e-5, atol=0, equal_nan=True)
                    np.testing.assert_allclose(res[2].cpu().numpy(), want[2], rtol=1e-5, atol=1e-30, equal_nan=True)
                c.check()
    fixed('the dual-pol regimes', pattern, body)
    assert seen == {'omnibus_c2_global', 'omnibus_c2_fused', 'omnibus_c2_dense', 'omnibus_c2_search',
                    'omnibus_c2_exact'}, sorted(seen)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_full_pol_regimes(K, oracle, device, pattern):
    """omnibus_c3_impl (nd_amd/csrc/omnibus_c3.hip) times its launches under the dual-pol labels.  Reachable, and
    required of the union: omnibus_c2_global (the plain, time-split and pixel-major pass A), omnibus_c2_fused (the
    streaming searches, alpha < 0.75), omnibus_c2_search (segment starts behind a fused search; the rounds on the
    dump; the pixel-major search; the last search where neither ran in front of it) and omnibus_c2_exact (the last
    search behind either).  omnibus_c2_dense and omnibus_c2_sample have no launch site in that file.  Cases: 12 x 131
    pixels; k = 2 (no segment starts), 12 and 24 (the time-split pass A and its dump: float32, 2 <= k <= 64, no
    rasters), 70 (beyond it), float64, n = 1 (the exact whole-series test), the pixel-major entry; maps against the
    oracle byte for byte, the rasters by the rule of tests/test_omnibus_c3_gpu.py."""
    seen = set()

    def body(c):
        for dtype, k, n, calls in ((np.float32, 2, 9, ((0.01, False), (0.99, False))),
                                   (np.float32, 12, 9, ((0.01, False), (0.5, True), (0.99, False), (0.99, True))),
                                   (np.float32, 24, 1, ((0.01, False), (0.99, False))),
                                   (np.float64, 12, 9, ((0.01, True), (0.99, False))),
                                   (np.float32, 70, 9, ((0.1, False), (0.9, False)))):
            planes = synth.omnibus_stack_c3(seed=80 + k, k=k, ny=12, nx=131, dtype=dtype, change_frac=0.3)
            yxt = [np.ascontiguousarray(np.moveaxis(p, 0, -1)) for p in planes]
            dev = [up(p, device) for p in planes]
            for alpha, stats in calls:
                with np.errstate(all='ignore'):
                    want = oracle.change_detection_pol(yxt, 3, alpha, n, njobs=8, stats=True)
                forms = [lambda: K.change_detection_c3(dev, alpha=alpha, n=n, stats=stats)]
                if alpha >= 0.75 and k == 12:
                    pm = [up(a, device) for a in yxt]
                    forms.append(lambda: K.change_detection_c3_pixel_major(pm, alpha=alpha, n=n, stats=stats))
                for form in forms:
                    res, names = launched(form)
                    assert res is not None and names, (dtype, k, n, alpha, stats)
                    seen.update(names)
                    got = (res[0] if stats else res).cpu().numpy()
                    assert int((got != want[0]).sum()) == 0, ('%d map bytes differ' % (got != want[0]).sum(),
                                                              np.dtype(dtype).name, k, n, alpha, stats)
                    if stats:
                        close_stats(res, want, 1e-30)
                    c.check()
    fixed('the full-pol regimes', pattern, body)
    assert seen == {'omnibus_c2_global', 'omnibus_c2_fused', 'omnibus_c2_search', 'omnibus_c2_exact'}, sorted(seen)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_diagonal_regimes(K, fuzz, device, pattern):
    """omnibus_diag_impl (nd_amd/csrc/omnibus_diag.hip): one launch, omnibus_c2_fused, where the series fit its LDS
    image and alpha < 0.75; otherwise omnibus_c2_global and, from two dates on, omnibus_c2_search.  These three are
    reachable and required; the file launches nothing under the other labels.  Cases: both sides of the form's limit on
    the series length (tests/omnibus_diag_cases.py FUSED_MAX_K) and of 0.75, q = 1 and 3, both types, a single date;
    against tests/omnibus_diag_ref.py by omnibus_diag_cases.compare."""
    from tests import omnibus_diag_cases as C
    seen = set()

    def body(c):
        for q, dtype in ((1, 'float32'), (3, 'float64')):
            limit = C.FUSED_MAX_K[(q, dtype)]
            for k, alpha, stats in ((limit, 0.74, True), (limit, 0.76, False), (limit + 1, 0.01, False),
                                    (limit + 1, 0.99, True), (1, 0.5, True), (10, 0.01, False)):
                ny, nx = fuzz.draw_raster(np.random.default_rng(k), max(1, min(2000, fuzz.DIAG_WORK // (k * k))))
                planes = C.gamma_stack(90 + k, q, k, ny, nx, 4.4, dtype)
                inp = dict(planes=planes, q=q, dtype=dtype, n=4.4, alpha=alpha, stats=stats, layout='tyx')
                want = fuzz.want_omnibus_diag(inp)
                got, names = launched(lambda: fuzz.run_omnibus_diag(inp))
                seen.update(names)
                want_names = {'omnibus_c2_fused'} if (2 <= k <= limit and alpha < 0.75) else \
                    ({'omnibus_c2_global', 'omnibus_c2_search'} if k >= 2 else {'omnibus_c2_global'})
                assert names == want_names, (q, dtype, k, alpha, names)
                assert fuzz.compare_omnibus_diag(got, want, inp), (q, dtype, k, ny, nx, alpha, stats)
                c.check()
    fixed('the diagonal regimes', pattern, body)
    assert seen == {'omnibus_c2_global', 'omnibus_c2_fused', 'omnibus_c2_search'}, sorted(seen)


# =====================================================================================================================
# what the contract leaves unwritten keeps the pattern
# =====================================================================================================================
@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_nlmeans_writes_its_core_and_nothing_else(K, oracle, device, pattern):
    """pixelwise_nlmeans_3d(..., core=box) writes the box: inside it the result equals the oracle's by the rule of
    tools/fuzz_parity.py for true patch distances (1e-5 relative, 2e-6 of the largest value absolute), outside it
    every element still holds the pattern.  The generic kernel (C-contiguous (a, b, c, var)) and the tiled one (planar
    memory seen as (y, x, time, var)); 40 x 70: more than one tile, the core ragged against it."""
    import torch

    def body(c):
        rng = np.random.default_rng(12)
        for shape, r, f, perm, core in (((9, 20, 30, 2), (1, 2, 2), (0, 1, 1), None, ((2, 7), (3, 18), (5, 26))),
                                        ((40, 70, 2, 1), (3, 2, 0), (1, 1, 0), (3, 2, 0, 1), ((6, 31), (4, 67), (0, 2)))):
            a = rng.gamma(4.0, 0.25, shape).astype(np.float32)
            want = np.empty_like(a)
            oracle.pixelwise_nlmeans_3d(a, want, r, f, 0.4, 0.5, -1, neff_policy=0, njobs=8, patch_mode=1)
            t = up(a, device)
            if perm is not None:
                inv = [perm.index(i) for i in range(4)]
                t = t.permute(*perm).contiguous().permute(*inv)
            out = torch.empty_like(t)
            K.pixelwise_nlmeans_3d(t, out, r, f, 0.4, 0.5, -1, patch_mode=1, neff_policy=0, core=core)
            box = tuple(slice(lo, hi) for lo, hi in core)
            left = c.is_poison(out)
            assert not bool(left[box].any()), 'core elements were not written'
            left[box] = True
            assert bool(left.all()), '%d elements outside the core were written' % int((~left).sum())
            got = out.cpu().numpy()
            assert np.isclose(got[box], want[box], rtol=1e-5, atol=2e-6 * float(a.max())).all(), shape
            c.check()
    fixed('pixelwise_nlmeans_3d with a core', pattern, body)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_strided_outputs_keep_their_padding(K, device, pattern):
    """out= as a window of a larger poisoned tensor (a margin on every side, every second element of the rows): the
    window equals the restatement everywhere, by each family's own rule, and every element around it keeps the
    pattern.  speckle_lee, speckle_multitemporal in both forms, resample, rasterize_polygons and sieve_regions."""
    import torch
    from tests import rasterize_cases, rasterize_ref, regions_cases, regions_ref, resample_cases, resample_ref
    from tests import speckle_cases, speckle_ref

    def window_of(c, shape, dtype):
        buf = torch.empty([n + 3 for n in shape[:-1]] + [2 * shape[-1] + 1], dtype=dtype, device=device)
        window = tuple(slice(1, 1 + n) for n in shape[:-1]) + (slice(1, 1 + 2 * shape[-1], 2),)

        def rest_is_poison():
            left = c.is_poison(buf)
            assert not bool(left[window].any()), 'elements of the window were not written'
            left[window] = True
            assert bool(left.all()), '%d elements around the window were written' % int((~left).sum())
        return buf[window], rest_is_poison

    def body(c):
        rng = np.random.default_rng(13)
        src = speckle_cases.speckle(rng, (3, 41, 77), np.float32)
        out, rest = window_of(c, src.shape, torch.float32)
        assert K.speckle_lee(up(src, device), 7, 4.0, 'lee', out=out) is out
        speckle_cases.assert_same(out.cpu().numpy(), speckle_ref.lee(src, 7, 4.0, 'lee'))
        rest()
        for k in (3, 40):                                   # the one-launch form, and the two passes with a workspace
            src = speckle_cases.speckle(rng, (k, 20, 77), np.float32)
            out, rest = window_of(c, src.shape, torch.float32)
            assert K.speckle_multitemporal(up(src, device), 5, out=out) is out
            speckle_cases.assert_same(out.cpu().numpy(), speckle_ref.multitemporal([src], 5)[0])
            rest()
        src = resample_cases.source(rng, (2, 37, 53))
        tr_s, tr_d = resample_cases.whole_extent(37, 53, 29, 71)
        for method in ('nearest', 'cubic'):
            ty = K.resample_axis(37, 29, resample_ref.axis_of(tr_s, 'y'), resample_ref.axis_of(tr_d, 'y'), method)
            tx = K.resample_axis(53, 71, resample_ref.axis_of(tr_s, 'x'), resample_ref.axis_of(tr_d, 'x'), method)
            out, rest = window_of(c, (2, 29, 71), torch.float32)
            assert K.resample(up(src, device), ty, tx, out=out) is out
            resample_cases.assert_same(out.cpu().numpy(), resample_ref.regrid(src, tr_s, tr_d, 29, 71, method),
                                       payloads=method == 'nearest')
            rest()
        polys = [rasterize_cases.random_polygon(rng, 33, 61, hole=bool(i % 2)) for i in range(6)]
        verts, ro, po = rasterize_ref.pack(polys)
        values = np.arange(1, 7)
        out, rest = window_of(c, (1, 33, 61), torch.int64)
        assert K.rasterize_polygons(torch.from_numpy(verts).to(device), ro, po, values, 33, 61, fill=-3, out=out) is out
        assert np.array_equal(out.cpu().numpy(), rasterize_ref.burn(polys, values, 33, 61, fill=-3))
        rest()
        stack = np.stack([regions_cases.mask(rng, (45, 67), d) for d in (0.59, 0.41)])
        out, rest = window_of(c, stack.shape, torch.uint8)
        assert K.sieve_regions(up(stack, device), 4, 8, out=out) is out
        regions_cases.assert_same(out.cpu().numpy(), np.stack(regions_ref.planes(regions_ref.sieve, stack, 4, 8, 0, False,
                                                                                 None)))
        rest()
    fixed('strided outputs', pattern, body)


@pytest.mark.parametrize('pattern', PATTERNS, ids=PATTERN_IDS)
def test_regions_leave_the_planes_they_were_not_given(K, device, pattern, monkeypatch):
    """label_regions on the first five planes of a seven-plane batch, into the first five planes of poisoned labels
    and areas, with the workspace cap of test_workspace_cap_walks_the_batch_in_chunks (two planes per call: chunks
    (0, 2), (2, 4), (4, 5), every one on the same poisoned workspace): the five planes equal the restatement, the two
    planes behind them keep the pattern, and the counts of a chunk do not reach into the next one's."""
    import torch
    from tests import regions_cases as cases, regions_ref as ref
    rng = np.random.default_rng(15)
    stack = np.stack([cases.mask(rng, (50, 70), 0.55) for _ in range(7)])
    monkeypatch.setattr(K, 'REGIONS_WORKSPACE_CAP', 2 * (50 * 70 * 8 + 600))
    assert K._region_chunks(5, 50, 70, True) == [(0, 2), (2, 4), (4, 5)]
    wl, wc = cases.want_label(stack[:5], 4)

    def body(c):
        labels = torch.empty(stack.shape, dtype=torch.int32, device=device)
        area = torch.empty(stack.shape, dtype=torch.int32, device=device)
        res = K.label_regions(up(stack, device)[:5], 4, labels=labels[:5], area=area[:5])
        assert res[0].data_ptr() == labels.data_ptr() and res[2].data_ptr() == area.data_ptr()
        assert np.array_equal(res[1].cpu().numpy(), wc)
        cases.assert_same(labels[:5].cpu().numpy(), wl)
        cases.assert_same(area[:5].cpu().numpy(), np.stack([ref.area(l, n) for l, n in zip(wl, wc)]))
        assert bool(c.is_poison(labels[5:]).all()) and bool(c.is_poison(area[5:]).all())
    fixed('label_regions in chunks', pattern, body)
