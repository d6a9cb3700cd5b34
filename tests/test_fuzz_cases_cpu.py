"""The randomised campaign of tools/fuzz_parity.py checked without a GPU, for the families merged after round 6:
over the very seeds tests/test_fuzz_gpu.py uses, the generators are deterministic, draw every regime the
dispatch code distinguishes at least MIN_DRAWS times (read from `desc` alone), leave out no more k-means rows
than tests/test_classify_gpu.py allows, and every compare_<name> accepts the restatement's own result and
rejects it after one seeded corruption.  The restatements' run time per family is printed and bounded."""
import functools
import hashlib
import os
import sys
import time

import numpy as np
import pytest

from tests import change_segments_cases, omnibus_diag_cases
from tests.test_fuzz_gpu import CASES_PER_FAMILY, NEWER_CASES_PER_FAMILY, SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_DRAWS = 5
SENSITIVITY_CASES = 20
FAMILIES = sorted(NEWER_CASES_PER_FAMILY) + ['c3']
# c3 is a round-6 family that gained layouts, rasters and the pixel-major entry point: its first 150 seeds
COUNT = dict(NEWER_CASES_PER_FAMILY, c3=min(150, CASES_PER_FAMILY['c3']))


@pytest.fixture(scope='module')
def F(oracle):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fuzz_parity
    return fuzz_parity


def digest(inputs):
    h = hashlib.sha1()
    for key in sorted(inputs):
        v = inputs[key]
        for a in (v if isinstance(v, list) else [v]):
            h.update(np.asarray(a).tobytes() if isinstance(a, np.ndarray) else repr(a).encode())
    return h.hexdigest()


def got_like(family, want, inputs):
    """the restatement's result cut down to what the device step of that case returns (copies)"""
    if family in ('omnibus_diag', 'c3', 'c3_more'):
        keys = ('map', 'z', 'P') if inputs['stats'] else ('map',)
    elif family == 'change_segments':
        keys = [k for k in want if inputs['outputs'] == 'both' or (k == 'direction') == (inputs['outputs'] == 'direction')]
    elif family in ('forest', 'knn'):
        keys = ('labels', 'proba') if inputs['outputs'] == 'both' else (inputs['outputs'],)
    elif family == 'kmeans_predict':
        keys = ('labels',)
    elif family == 'kmeans_step':
        keys = ('labels', 'sums', 'counts', 'inertia', 'changed', 'count', 'mean', 'var')
    else:
        keys = list(want)
    return {k: np.array(want[k]) for k in keys}


# ---- one seeded corruption each: -> True where it could be applied ------------------------------------------
def one_ulp(a, j):
    """the value at flat position j moved to a neighbour; a NaN there becomes a number (a mask position cleared)"""
    v = a.flat[j]
    a.flat[j] = 0 if np.isnan(v) else np.nextafter(v, np.inf if v <= 0 else -np.inf)


def pick(rng, mask):
    idx = np.flatnonzero(mask)
    return int(idx[rng.integers(0, idx.size)]) if idx.size else None


def flip_map_byte(got, rng, inputs):
    j = int(rng.integers(0, got['map'].size))
    got['map'].flat[j] ^= 1
    return True


def change_direction_code(got, rng, inputs):
    if 'direction' not in got:
        return False
    j = int(rng.integers(0, got['direction'].size))
    got['direction'].flat[j] = (got['direction'].flat[j] + 1) % 4
    return True


def move_mean(got, rng, inputs):
    keys = sorted(k for k in got if k.startswith('mean'))
    if not keys:
        return False
    a = got[keys[int(rng.integers(0, len(keys)))]]
    j = pick(rng, ~np.isnan(a))
    if j is None:
        return False
    one_ulp(a, j)
    return True


def move_limit(got, rng, inputs):
    one_ulp(got['limits'], int(rng.integers(0, got['limits'].size)))
    return True


def move_rgb_byte(got, rng, inputs):
    j = int(rng.integers(0, got['rgb'].size))
    got['rgb'].flat[j] = int(got['rgb'].flat[j]) + (1 if got['rgb'].flat[j] < 255 else -1)
    return True


def move_probability(key):
    def corrupt(got, rng, inputs):
        if key not in got:
            return False
        j = pick(rng, ~np.isnan(got[key]))
        if j is None:
            return False
        one_ulp(got[key], j)
        return True
    return corrupt


def replace_label(got, rng, inputs):
    """a compared row's label becomes another class (a number no class has where there is one class only)"""
    if 'labels' not in got:
        return False
    lab = got['labels']
    valid = ~np.isnan(lab) if lab.dtype.kind == 'f' else lab >= 0
    if 'centers' in inputs and 'prev' not in inputs:                     # kmeans_predict: a row that is compared
        valid = inputs['_compared']
    j = pick(rng, valid)
    if j is None:
        return False
    pool = inputs['classes'] if 'classes' in inputs else np.arange(inputs['centers'].shape[0])
    other = [c for c in pool if c != lab.flat[j]]
    lab.flat[j] = other[int(rng.integers(0, len(other)))] if other else lab.flat[j] + 1
    return True


def clear_mask_position(got, rng, inputs):
    key = next((k for k in ('labels', 'proba') if k in got and got[k].dtype.kind == 'f'), None)
    if key is None:
        return False
    j = pick(rng, np.isnan(got[key]))
    if j is None:
        return False
    got[key].flat[j] = inputs['classes'][0] if 'classes' in inputs else 0.0
    return True


def move_count(got, rng, inputs):
    got['counts'].flat[int(rng.integers(0, got['counts'].size))] += 1
    return True


def move_warped(got, rng, inputs):
    """float64: one value to its neighbour; float32: one value by twice the tolerance of the rule"""
    a = got[sorted(got)[int(rng.integers(0, len(got)))]]
    j = int(rng.integers(0, a.size))
    if a.dtype == np.float64:
        one_ulp(a, j)
    else:
        a.flat[j] += np.float32(2e-6 * max(float(np.abs(a).max()), 1e-30) + 1e-37)
    return True


CORRUPTIONS = {
    'omnibus_diag': [flip_map_byte], 'c3': [flip_map_byte], 'c3_more': [flip_map_byte],
    'change_segments': [change_direction_code, move_mean],
    'to_rgb': [move_limit, move_rgb_byte, move_count],
    'forest': [move_probability('proba'), replace_label, clear_mask_position],
    'knn': [move_probability('proba'), replace_label, clear_mask_position],
    'kmeans_predict': [replace_label, clear_mask_position],
    'linear': [move_probability('decision'), replace_label, clear_mask_position],
    'kmeans_step': [replace_label, move_count],
    'warp': [move_warped],
}


@functools.lru_cache(maxsize=None)
def _survey(F, family):
    gen, want_of, compare = (getattr(F, p + family) for p in ('gen_', 'want_', 'compare_'))
    out = dict(descs=[], same=True, seconds=0.0, codes=set(), compared=0, close=0, accepted=[], applied={}, missed=[])
    for i in range(COUNT[family]):
        inputs, desc = gen(np.random.default_rng([SEED, i]))
        again, desc2 = gen(np.random.default_rng([SEED, i]))
        out['same'] &= (repr(desc) == repr(desc2) and digest(inputs) == digest(again))
        out['descs'].append(desc)
        t0 = time.perf_counter()
        want = want_of(inputs)
        out['seconds'] += time.perf_counter() - t0
        if family == 'change_segments':
            out['codes'] |= set(np.unique(want['direction']).tolist())
        if family == 'kmeans_predict':
            inputs['_compared'] = F.compared_rows(want, inputs)
            if not inputs['planted']:
                keep = ~np.isnan(want['labels'])
                out['compared'] += int(keep.sum())
                out['close'] += int((keep & ~inputs['_compared']).sum())
        if i < SENSITIVITY_CASES:
            out['accepted'].append(bool(compare(got_like(family, want, inputs), want, inputs)))
            for c, corrupt in enumerate(CORRUPTIONS[family]):
                got = got_like(family, want, inputs)
                name = getattr(corrupt, '__name__', 'corrupt') + str(c)
                if corrupt(got, np.random.default_rng([SEED, i, c]), inputs):
                    out['applied'][name] = out['applied'].get(name, 0) + 1
                    if compare(got, want, inputs):
                        out['missed'].append((name, i, desc))
    return out


@pytest.fixture
def survey(F):
    return lambda family: _survey(F, family)


def drawn(descs, **conditions):
    """how many cases meet every condition: a value, or a predicate of the value"""
    return sum(all(v(d[k]) if callable(v) else d[k] == v for k, v in conditions.items()) for d in descs)


def assert_drawn(descs, what, **conditions):
    n = drawn(descs, **conditions)
    assert n >= MIN_DRAWS, '%s: drawn %d times in %d cases' % (what, n, len(descs))


@pytest.mark.parametrize('family', FAMILIES)
def test_generators_are_deterministic(survey, family):
    assert COUNT[family] >= 150
    assert survey(family)['same']


FORMS = {'<= 4': lambda n: n <= 4, '5 - 8': lambda n: 5 <= n <= 8, '> 8': lambda n: n > 8}
CLASS_SLOTS = {'<= 2': lambda n: n <= 2, '<= 4': lambda n: 2 < n <= 4, '<= 8': lambda n: 4 < n <= 8, '> 8': lambda n: n > 8}


def _row_table_coverage(descs, family, F):
    for layout in F.ROW_LAYOUTS:
        assert_drawn(descs, '%s layout %s' % (family, layout), layout=layout)
    assert_drawn(descs, family + ' a size-1 dimension among several', sizes=lambda s: len(s) > 1 and 1 in s)
    for nd in (1, 2, 3, 4):
        assert_drawn(descs, '%s %d row dimensions' % (family, nd), sizes=lambda s: len(s) == nd)
    assert_drawn(descs, family + ' base pointer off the 16-byte grid', base=lambda b: b > 0)
    assert_drawn(descs, family + ' NaN features', corner='nan')
    for rows in (1, 63, 65):
        assert_drawn(descs, '%s %d rows' % (family, rows), rows=rows)
    assert_drawn(descs, family + ' 255 to 257 rows', rows=lambda r: 255 <= r <= 257)
    for scale in F.SCALES:
        assert_drawn(descs, '%s scale %g' % (family, scale), scale=scale)


@pytest.mark.parametrize('family', ['forest', 'kmeans_predict', 'kmeans_step', 'knn', 'linear'])
def test_coverage_of_the_row_table_families(F, survey, family):
    descs = survey(family)['descs']
    _row_table_coverage(descs, family, F)
    for form, in_form in FORMS.items():
        for scaler in (False, True):
            for dtype in ('float32', 'float64'):
                assert_drawn(descs, '%s: %s features, scaler %s, %s' % (family, form, scaler, dtype),
                             features=in_form, scaler=scaler, dtype=dtype)
    if family in ('forest', 'knn'):
        for slot, in_slot in CLASS_SLOTS.items():
            assert_drawn(descs, '%s: %s classes' % (family, slot), classes=in_slot)
        for outputs in ('both', 'labels', 'proba'):
            assert_drawn(descs, '%s: outputs %s' % (family, outputs), outputs=outputs)
    if family == 'forest':
        assert_drawn(descs, 'forest: one tree', trees=1)
        assert_drawn(descs, 'forest: depth 8', depth=8)
        assert_drawn(descs, 'forest: a single leaf', depth=0)
    if family == 'kmeans_predict':
        assert_drawn(descs, 'kmeans_predict: planted duplicates', planted=True)
        assert_drawn(descs, 'kmeans_predict: one centre', k=1)
        assert_drawn(descs, 'kmeans_predict: more than 32 centres', k=lambda k: k > 32)
    if family == 'kmeans_step':
        assert_drawn(descs, 'kmeans_step: at the accumulator limit', at_limit=True)
        assert_drawn(descs, 'kmeans_step: no valid row', empty=True)
        for first in (False, True):
            assert_drawn(descs, 'kmeans_step: first iteration %s' % first, first=first)
    if family == 'knn':
        assert_drawn(descs, 'knn: integer features', integers=True)
        assert sum(d['k'] == d['ntrain'] for d in descs) >= MIN_DRAWS              # every sample a neighbour
        assert_drawn(descs, 'knn: k of 32', k=32)
        for ntrain in (8, 9, 1000):
            assert_drawn(descs, 'knn: %d training samples' % ntrain, ntrain=ntrain)
    if family == 'linear':
        for slot, in_slot in CLASS_SLOTS.items():
            assert_drawn(descs, 'linear: %s coefficient rows' % slot, ncoef=in_slot)
        for link in ('none', 'softmax', 'ovr'):
            assert_drawn(descs, 'linear: link %s' % link, link=link)
        assert_drawn(descs, 'linear: a zero row and identical rows', special=True)


def test_coverage_of_omnibus_diag(F, survey):
    descs = survey('omnibus_diag')['descs']
    for (q, dtype), kmax in sorted(omnibus_diag_cases.FUSED_MAX_K.items()):
        what = 'omnibus_diag q = %d %s: ' % (q, dtype)
        assert_drawn(descs, what + 'k <= %d' % kmax, q=q, dtype=dtype, k=lambda k: k <= kmax)
        assert_drawn(descs, what + 'k > %d' % kmax, q=q, dtype=dtype, k=lambda k: k > kmax)
        assert_drawn(descs, what + 'the one-launch form', q=q, dtype=dtype, k=lambda k: k <= kmax, alpha=lambda a: a < 0.75)
        assert_drawn(descs, what + 'short series above alpha = 0.75', q=q, dtype=dtype, k=lambda k: k <= kmax,
                     alpha=lambda a: a >= 0.75)
    assert_drawn(descs, 'omnibus_diag alpha = 0.74', alpha=0.74)
    assert_drawn(descs, 'omnibus_diag alpha = 0.75', alpha=0.75)
    assert_drawn(descs, 'omnibus_diag alpha = 0.76', alpha=0.76)
    assert_drawn(descs, 'omnibus_diag k >= 97', k=lambda k: k >= 97)
    for layout in F.STACK_LAYOUTS:
        assert_drawn(descs, 'omnibus_diag layout ' + layout, layout=layout)
    for stats in (False, True):
        assert_drawn(descs, 'omnibus_diag stats %s' % stats, stats=stats)
    assert_drawn(descs, 'omnibus_diag corner values', corner=lambda c: c != 'none')
    for n in (1, 2.5, 4.4, 9):
        assert_drawn(descs, 'omnibus_diag n = %g' % n, n=n)


def test_coverage_of_change_segments(F, survey):
    s = survey('change_segments')
    descs = s['descs']
    for structure, nplanes in change_segments_cases.STRUCTURES:
        assert_drawn(descs, 'change_segments %s %d' % (structure, nplanes), structure=structure, planes=nplanes)
    assert {1, 2, 3} <= s['codes']
    for k in (1, 63, 64, 65):
        assert_drawn(descs, 'change_segments k = %d' % k, k=k)
    assert_drawn(descs, 'change_segments k >= 130', k=lambda k: k >= 130)
    for p in (0, 0.02, 0.25, 0.9, 1):
        assert_drawn(descs, 'change_segments p = %g' % p, p=p)
    for layout in F.STACK_LAYOUTS:
        assert_drawn(descs, 'change_segments layout ' + layout, layout=layout)
    for outputs in ('both', 'direction', 'means'):
        assert_drawn(descs, 'change_segments outputs ' + outputs, outputs=outputs)
    for key in ('first', 'single'):
        for flag in (False, True):
            assert_drawn(descs, 'change_segments %s %s' % (key, flag), **{key: flag})
    assert_drawn(descs, 'change_segments corner values', corner=lambda c: c != 'none')


def test_coverage_of_to_rgb_warp_and_c3(F, survey):
    descs = survey('to_rgb')['descs']
    for layout in F.STACK_LAYOUTS:
        assert_drawn(descs, 'to_rgb layout ' + layout, layout=layout)
    for recipe in F.RGB_RECIPES:
        assert_drawn(descs, 'to_rgb recipe ' + recipe, recipes=lambda r: any(x.split('/')[0] == recipe for x in r))
    assert_drawn(descs, 'to_rgb quotient', recipes=lambda r: any(x.endswith('/quotient') for x in r))
    for nch in (1, 3):
        assert_drawn(descs, 'to_rgb %d channels' % nch, channels=nch)
    for frames in (1, 2, 3, 4):
        assert_drawn(descs, 'to_rgb %d frames' % frames, frames=frames)
    assert_drawn(descs, 'to_rgb store tails', nx=lambda n: n <= 9)
    assert sum(d['pmin'] > d['pmax'] for d in descs) >= MIN_DRAWS                 # reversed percentiles
    assert_drawn(descs, 'to_rgb vmin', vmin=lambda v: v is not None)
    assert_drawn(descs, 'to_rgb vmax alone', vmin=None, vmax=lambda v: v is not None)
    assert_drawn(descs, 'to_rgb mask', mask=True)
    descs = survey('warp')['descs']
    for layout in ('planar', 'pixel_major'):
        for dtype in ('float32', 'float64'):
            assert_drawn(descs, 'warp %s %s' % (layout, dtype), layout=layout, dtype=dtype)
    assert_drawn(descs, 'warp without a reference', reference=-1)
    assert_drawn(descs, 'warp with a reference', reference=lambda r: r >= 0)
    assert_drawn(descs, 'warp one date', k=1)
    for nv in (1, 2, 3):
        assert_drawn(descs, 'warp %d variables' % nv, variables=lambda v: len(v) == nv)
    assert_drawn(descs, 'warp odd raster', rows=lambda r: r % 2 == 1, cols=lambda c: c % 2 == 1)
    assert_drawn(descs, 'warp even raster', rows=lambda r: r % 2 == 0, cols=lambda c: c % 2 == 0)
    for family in ('c3', 'c3_more'):
        descs = survey(family)['descs']
        for layout in ('tyx', 'yxt', 'pad', 'pm', 'pmc'):
            assert_drawn(descs, '%s layout %s' % (family, layout), layout=layout)
        for stats in (False, True):
            assert_drawn(descs, '%s stats %s' % (family, stats), stats=stats)
    for k in F.C3_MORE_KS:
        assert_drawn(descs, 'c3_more k = %d' % k, k=k)
    assert_drawn(descs, 'c3_more: the pixel-major entry point takes the case', k=lambda k: k in (8, 16, 32, 96),
                 layout=lambda l: l in ('pm', 'pmc'), alpha=lambda a: a >= 0.75)


def test_kmeans_exclusion_cap(survey):
    """kmeans_predict is the one family that leaves rows out: at most 1 in 10^4 of the compared rows (the cap of
    test_kmeans_labels), the planted-duplicate cases, compared in full, aside"""
    s = survey('kmeans_predict')
    print('kmeans_predict: %d of %d rows lie within 1e-12 of a tie' % (s['close'], s['compared']))
    assert s['compared'] > 0 and s['close'] <= 1e-4 * s['compared']


@pytest.mark.parametrize('family', FAMILIES)
def test_compare_accepts_the_restatement_and_rejects_one_corruption(survey, family):
    s = survey(family)
    assert len(s['accepted']) == SENSITIVITY_CASES and all(s['accepted'])
    assert not s['missed'], s['missed'][:3]
    for c, corrupt in enumerate(CORRUPTIONS[family]):
        name = getattr(corrupt, '__name__', 'corrupt') + str(c)
        assert s['applied'].get(name, 0) >= 1, (name, s['applied'])           # every corruption was tried


@pytest.mark.parametrize('family', FAMILIES)
def test_reference_run_time(survey, family):
    s = survey(family)
    print('%s: %d restatement calls in %.1f s' % (family, COUNT[family], s['seconds']))
    assert s['seconds'] < 60.0
