"""A few hundred seeded random cases of kernels.resample against tests/resample_ref.py, equal everywhere: sizes
1 ... 200, ratios 0.05 ... 40, offsets, signs of the pixel sizes on either side, methods, types, layouts, crops,
strided outputs, fills and non-finite samples (tests/resample_cases.py random_case).  A case that raises ends the
loop: the device may have faulted, and nothing more is run on it."""
import numpy as np
import pytest

from tests import resample_cases as cases
from tests import resample_ref as ref

pytestmark = pytest.mark.gpu
SEED = 20261019
CASES = 300


def test_fuzz_resample(device):
    from nd_amd import kernels as K
    fails = []
    for i in range(CASES):
        case = cases.random_case(np.random.default_rng([SEED, i]))
        args = (case['src'], case['tr_s'], case['tr_d'], case['H'], case['W'], case['method'])
        want = ref.regrid(*args, fill=case['fill'])
        try:
            got = cases.device_regrid(K, *args, case['layout'], fill=case['fill'], crop=case['crop'],
                                      strided_out=case['strided_out'])
        except Exception as e:              # noqa: BLE001
            pytest.fail('resample case %d raised %r after %d differing cases; the case: %s'
                        % (i, e, len(fails), cases.describe(case)))
        try:
            cases.assert_same(got, want, payloads=case['method'] == 'nearest')
        except AssertionError as e:
            fails.append((i, str(e), cases.describe(case)))
    assert not fails, '%d of %d resample cases differ from the restatement: %s' % (len(fails), CASES, fails[:3])
