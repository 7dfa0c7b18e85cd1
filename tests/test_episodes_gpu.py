"""The episode ledger on the device: the bodies of tests/test_episodes.py on VecSide."""
import pytest
from sides import VecSide

import test_episodes as body

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M,step_budget", [(3, 0), (3, 1250), (1, 0), (8, 0)])
def test_ledger_against_host_loop(M, step_budget):
    body.loop_matches_host(VecSide, M, step_budget, need_both=(M == 3))


def test_ledger_quota_and_parking():
    body.parked_rows_are_left_alone(VecSide)


def test_ledger_consume():
    body.consume_leaves_the_requests(VecSide)


def test_ledger_pools():
    body.pool_records_are_logged(VecSide)


def test_ledger_extent_and_null_pointers():
    body.extent_and_null_pointers(VecSide)


def test_ledger_bad_arguments():
    body.bad_arguments(VecSide)
