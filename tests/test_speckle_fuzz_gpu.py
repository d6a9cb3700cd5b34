"""Two hundred seeded random cases of kernels.speckle_lee and kernels.speckle_multitemporal against
tests/speckle_ref.py, equal everywhere: sizes 1 ... 150, every window width, both filters and methods, one to four
variables, series on either side of the one-launch form's limit, types, layouts, crops, strided outputs and planted
NaN / inf / zero / negative / subnormal samples (tests/speckle_cases.py random_case).  A case that raises ends the
loop: the device may have faulted, and nothing more is run on it."""
import numpy as np
import pytest

from tests import speckle_cases as cases

pytestmark = pytest.mark.gpu
SEED = 20261020
CASES = 200


def test_fuzz_speckle(device):
    from nd_amd import kernels as K
    fails = []
    for i in range(CASES):
        case = cases.random_case(np.random.default_rng([SEED, i]))
        try:
            got, want = cases.run_case(K, case)
        except AssertionError as e:         # what surrounds a strided output was written, or `out` was not returned
            fails.append((i, str(e), cases.describe(case)))
            continue
        except Exception as e:              # noqa: BLE001
            pytest.fail('speckle case %d raised %r after %d differing cases; the case: %s'
                        % (i, e, len(fails), cases.describe(case)))
        try:
            for g, w in zip(got, want):
                cases.assert_same(g, w)
        except AssertionError as e:
            fails.append((i, str(e), cases.describe(case)))
    assert not fails, '%d of %d speckle cases differ from the restatement: %s' % (len(fails), CASES, fails[:3])
