"""Two hundred seeded random cases of kernels.zonal_index, zonal_stats and zonal_paint against tests/zonal_ref.py, bit
for bit: sizes 1 ... 150 per axis, zone maps from random class maps, label_regions-like blobs and random sparse ids,
1 to 6 planes, every label and data type, layouts, crops, strided label planes and outputs, NaN and inf injection
(tests/zonal_cases.py random_case).  A case that raises ends the loop: the device may have faulted, and nothing more is
run on it."""
import numpy as np
import pytest

from tests import zonal_cases as cases

pytestmark = pytest.mark.gpu
SEED = 20261021
CASES = 200


def test_fuzz_zonal(device):
    from nd_amd import kernels as K
    fails = []
    for i in range(CASES):
        case = cases.random_case(np.random.default_rng([SEED, i]))
        try:
            cases.run_case(K, case)
        except AssertionError as e:
            fails.append((i, str(e)[:300], cases.describe(case)))
        except Exception as e:              # noqa: BLE001
            pytest.fail('zonal case %d raised %r after %d differing cases; the case: %s'
                        % (i, e, len(fails), cases.describe(case)))
    assert not fails, '%d of %d zonal cases differ from the restatement: %s' % (len(fails), CASES, fails[:3])
