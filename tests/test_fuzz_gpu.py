"""The randomised parity campaign of tools/fuzz_parity.py under pytest: fixed seeds, a fixed number
of cases per kernel family (random shapes, strides, layouts, parameters, thresholds, step changes,
zeros / NaNs / infinities / negative determinants), the HIP path through the C ABI against the CPU
oracle.  Bit-exact change maps, 1e-5 relative for the float outputs; the ill-posed n_eff corner of
non-local means is recognised from the oracle alone and not compared, as in the tool.
About forty seconds in all for the seven families of round 6.

The families merged since (intensity-only omnibus, change_segments, to_rgb, the four classifiers' predict, the
k-means fit step, the coregistration warp, and the full-pol test in every layout) run against the numpy
restatements under tests/, each by the comparison rule of its own test file; tests/test_fuzz_cases_cpu.py checks
their generators and rules without a GPU.  A case that raises ends its family's loop: the device may have
faulted, and nothing more is run on it."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261004
# (sized for ~40 s in all: the suite runs under a 900 s limit.  The long campaign is tools/fuzz_parity.py,
#  its result per round under profiles/ -- r06: 5 248 omnibus / c3 cases in 240 s, no difference)
# (omnibus_long: 193 - 4096 dates on rasters of at most 128 pixels, about 20 s)
CASES_PER_FAMILY = {'omnibus': 250, 'omnibus_long': 80, 'omnibus_ml': 300, 'c3': 400, 'nlmeans': 2500, 'correlate': 5000,
                    'gaussian': 6000}
# the families merged since (tools/fuzz_parity.py: NEWER), against the numpy restatements under tests/.  Measured on
# one MI355X with --durations=0, seconds per 150 cases: omnibus_diag 1.5, change_segments 1.6, c3_more 3.5, warp 0.5,
# knn 0.28, forest 0.27, kmeans_step 0.26, kmeans_predict 0.12, linear 0.11, to_rgb 0.10; c3 with its layouts and
# rasters 9.2 s for its 400 cases.  A round-6 family takes about 6 s; the cheap families get four times the minimum
# of 150 cases and stay near a second, because tests/test_fuzz_cases_cpu.py replays every seed on the CPU, where a
# case costs more than on the device.  omnibus_diag has 300: 150 do not draw every form limit five times.
NEWER_CASES_PER_FAMILY = {'omnibus_diag': 300, 'change_segments': 150, 'to_rgb': 600, 'forest': 600, 'kmeans_predict': 600,
                          'knn': 600, 'linear': 600, 'kmeans_step': 600, 'warp': 150, 'c3_more': 150}
CASES_PER_FAMILY.update(NEWER_CASES_PER_FAMILY)


@pytest.fixture(scope='module')
def fuzz(device, oracle):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fuzz_parity
    return fuzz_parity


@pytest.mark.parametrize('family', sorted(CASES_PER_FAMILY))
def test_fuzz_family(fuzz, family):
    fails = []
    for i in range(CASES_PER_FAMILY[family]):
        rng = np.random.default_rng([SEED, i])
        try:
            ok, desc = fuzz.CASES[family](rng)
        except Exception as e:              # noqa: BLE001
            # not a comparison's verdict: the device may have faulted, so no further case is drawn on it
            pytest.fail('%s case %d raised %r after %d differing cases %s; replay with tools/fuzz_replay.py'
                        % (family, i, e, len(fails), fails[:5]))
        if not ok:
            fails.append((i, desc))
    assert not fails, '%d of %d %s cases differ from the oracle; replay with tools/fuzz_replay.py: %s' % (
        len(fails), CASES_PER_FAMILY[family], family, fails[:5])
