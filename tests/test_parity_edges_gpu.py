"""The bodies of tests/test_parity_edges.py on the device: ragged batches stepped in one handle, the register-slot edges, the d > d0 arm
of the packet cost, and the parity sweep over ragged batches, com_range 100 m and eight-slot kernels -- every request against the oracle
through parity.RequestCheck (charger state and the provenance of prev_minfit included)."""
import pytest

import test_parity_edges as body
from sides import VecSide

pytestmark = pytest.mark.gpu


def test_ragged_batch_matches_oracle():
    body.ragged_batch_matches_oracle(VecSide)


@pytest.mark.parametrize("N", sorted(body.SLOT_EDGES))
def test_slot_edges_match_oracle(N):
    body.slot_edges_match_oracle(VecSide, N)


@pytest.mark.parametrize("seed,n,t", body.D4_NETWORKS)
def test_d4_packet_cost_matches_oracle(seed, n, t):
    body.d4_packet_cost_matches_oracle(VecSide, seed, n, t)


def test_d4_packet_cost_on_the_neighbour_list_path():
    body.d4_packet_cost_on_the_neighbour_list_path(VecSide)


def test_pushed_level_search_takes_the_neighbour_list():
    body.pushed_level_search_takes_the_neighbour_list(VecSide)


@pytest.mark.parametrize("budget", body.RAGGED_BUDGETS)
def test_ragged_slot_counts_in_one_handle_match_oracle(budget):
    body.ragged_slot_counts_in_one_handle_match_oracle(VecSide, budget)


@pytest.mark.parametrize("case", sorted(body.SWEEPS["gpu"]))
def test_parity_sweep_edges(case):
    body.parity_sweep_edges(VecSide, case)
