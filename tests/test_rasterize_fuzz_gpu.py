"""The rasterize family of tools/fuzz_parity.py under pytest: a fixed seed and a fixed number of cases -- random
polygon sets, grids of either orientation, layers, value types and output strides -- against
tests/rasterize_ref.py, the same bytes everywhere.  A case that raises ends the loop: the device may have faulted,
and nothing more is run on it.  (150 cases: about 3 s of restatement on the host, well under a second of device.)"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261019
CASES = 150


def test_fuzz_rasterize(device):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fuzz_parity
    from nd_amd import vector                                   # noqa: F401  (the family needs the feature)
    fails = []
    for i in range(CASES):
        rng = np.random.default_rng([SEED, i])
        try:
            ok, desc = fuzz_parity.CASES['rasterize'](rng)
        except Exception as e:              # noqa: BLE001
            pytest.fail('rasterize case %d raised %r after %d differing cases %s; replay with tools/fuzz_replay.py'
                        % (i, e, len(fails), fails[:5]))
        if not ok:
            fails.append((i, desc))
    assert not fails, '%d of %d rasterize cases differ from the restatement: %s' % (len(fails), CASES, fails[:5])
