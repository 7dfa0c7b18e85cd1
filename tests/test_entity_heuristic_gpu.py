"""The heuristic baseline on the device: the bodies of tests/test_entity_heuristic.py on VecSide."""
import pytest
from sides import VecSide

import test_entity_heuristic as body

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,M", body.SIZES)
def test_heuristic_sizes(N, M):
    body.sizes_match(VecSide, N, M)


def test_heuristic_planted():
    body.planted_cases(VecSide)


def test_heuristic_planted_single_charger():
    body.planted_cases(VecSide, N=64, M=1)


def test_heuristic_rows_are_independent():
    body.rows_are_independent(VecSide)


def test_heuristic_bad_arguments():
    body.bad_arguments(VecSide)


def test_heuristic_simulator_rows():
    body.simulator_rows(VecSide)
