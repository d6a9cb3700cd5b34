"""Two hundred seeded random cases of kernels.temporal_stats against tests/temporal_ref.py: sizes 1 ... 150 per axis,
series of 1 ... 140 dates, every data type, layout, crop and step, random subsets of the statistics and percentiles,
both skipna modes, NaN and inf injection (tests/temporal_cases.py random_case).  A case that raises ends the loop: the
device may have faulted, and nothing more is run on it."""
import numpy as np
import pytest

from tests import temporal_cases as cases

pytestmark = pytest.mark.gpu
SEED = 20261022
CASES = 200


def test_fuzz_temporal(device):
    from nd_amd import kernels as K
    fails = []
    for i in range(CASES):
        case = cases.random_case(np.random.default_rng([SEED, i]), K)
        try:
            cases.run_case(K, case)
        except AssertionError as e:
            fails.append((i, str(e)[:300], cases.describe(case)))
        except Exception as e:              # noqa: BLE001
            pytest.fail('temporal case %d raised %r after %d differing cases; the case: %s'
                        % (i, e, len(fails), cases.describe(case)))
    assert not fails, '%d of %d temporal cases differ from the restatement: %s' % (len(fails), CASES, fails[:3])
