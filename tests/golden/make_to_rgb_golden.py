"""
tests/golden/make_to_rgb_golden.py -- records what numpy computes for the to_rgb case planes
(tests/rgb_cases.py): np.nanpercentile at every test percentile and the composite bytes numpy computes
(tests/rgb_ref.numpy_composite), with numpy's version.  The contract is numpy 2.2.6; run with that.

    python tests/golden/make_to_rgb_golden.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
from tests import rgb_cases, rgb_ref  # noqa: E402


def main():
    out = {'numpy_version': np.array(np.__version__), 'percentiles': np.array(rgb_cases.PERCENTILES, float)}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for dt in rgb_cases.DTYPES:
            tag = np.dtype(dt).name
            for name, a in rgb_cases.planes(dt).items():
                out['%s/%s/plane' % (tag, name)] = a
                out['%s/%s/pct' % (tag, name)] = np.array([np.nanpercentile(a, p) for p in rgb_cases.PERCENTILES],
                                                          dtype=dt)
                out['%s/%s/grey' % (tag, name)] = rgb_ref.numpy_composite([a])
            p = rgb_cases.planes(dt)
            tri = [p['exponential'][:32, :32], p['scaled_1e6'], p['one_binade'][:32, :32]]
            out['%s/rgb' % tag] = rgb_ref.numpy_composite(tri)
    np.savez_compressed(os.path.join(HERE, 'to_rgb_numpy.npz'), **out)


if __name__ == '__main__':
    main()
