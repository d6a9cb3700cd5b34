"""nd_amd_temporal_stats on a held-back side stream: cases 0 - 7 of the fuzz generator (tests/temporal_cases.py) inside
tests/held_stream.py's held_stream, once without the hold and once held, against the restatement.  No guard is touched
and no call is judged WAITED: the entry is not in the contract's list of entries that may wait.

The run goes through tests/test_streams_gpu.py's held_replay, so that its verdicts are judged by that module's rule
and noted where its last test, which requires every stream-taking entry of the header to have been seen on a held
stream, looks for them; this module therefore runs before that one."""
import numpy as np
import pytest

from tests import temporal_cases as cases
from tests import test_streams_gpu as streams

pytestmark = pytest.mark.gpu
SEED = 20261022                 # tests/test_temporal_fuzz_gpu.py


def test_held_temporal(device):
    from nd_amd import kernels as K

    def one(i):
        cases.run_case(K, cases.random_case(np.random.default_rng([SEED, i]), K))
    calls = streams.held_replay('temporal', device, streams.COUNT, one)
    assert {c.entry for c in calls} == {'nd_amd_temporal_stats'}
    assert all(c.verdict == streams.HELD for c in calls), [c.verdict for c in calls]
