"""The bodies of tests/test_action_streams.py on the device: policy-shaped action streams (chargers converging on one node, one spot for
everybody, zero charging times, stays, clip edges, repeats, and their mix in blocking, budgeted and time-sliced launches) and the capacity
of the charging-rate list, four networks per handle -- every request against the oracle through parity.RequestCheck, Node.energyRR to the
ulp (2 per stay on a shared node), no row with a negative status."""
import pytest

import test_action_streams as body
from sides import VecSide

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(body.CASES))
def test_stream_matches_oracle(name):
    body.stream_matches_oracle(VecSide, name)


@pytest.mark.parametrize("mode", sorted(body.MIXED))
def test_mixed_stream_matches_oracle(mode):
    body.stream_matches_oracle(VecSide, "mixed", mode)


@pytest.mark.parametrize("N,M,over,K", body.CAPACITY)
def test_list_capacity_matches_oracle(N, M, over, K):
    body.list_capacity_matches_oracle(VecSide, N, M, over, K)
