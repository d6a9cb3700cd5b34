"""Two hundred seeded random cases of kernels.label_regions, region_sizes and sieve_regions against
tests/regions_ref.py, equal everywhere: sizes 1 ... 150 per axis, a density, both connectivities, every type,
by_value, backgrounds, 1 to 6 planes, layouts, crops, strided outputs and the three entry points
(tests/regions_cases.py random_case).  A case that raises ends the loop: the device may have faulted, and nothing more
is run on it."""
import numpy as np
import pytest

from tests import regions_cases as cases

pytestmark = pytest.mark.gpu
SEED = 20261020
CASES = 200


def test_fuzz_regions(device):
    from nd_amd import kernels as K
    fails = []
    for i in range(CASES):
        case = cases.random_case(np.random.default_rng([SEED, i]))
        try:
            got, want = cases.run_case(K, case)
        except AssertionError as e:         # what surrounds a strided output was written, or an output was not returned
            fails.append((i, str(e), cases.describe(case)))
            continue
        except Exception as e:              # noqa: BLE001
            pytest.fail('regions case %d raised %r after %d differing cases; the case: %s'
                        % (i, e, len(fails), cases.describe(case)))
        try:
            assert len(got) == len(want)
            for g, w in zip(got, want):
                cases.assert_same(g, w)
        except AssertionError as e:
            fails.append((i, str(e), cases.describe(case)))
    assert not fails, '%d of %d region cases differ from the restatement: %s' % (len(fails), CASES, fails[:3])
