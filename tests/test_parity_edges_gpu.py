"""tests/test_parity_edges.py on the device: ragged batches stepped in one handle, the register-slot edges, and the parity sweep over
ragged batches, com_range 100 m (the d > d0 arm of the packet cost) and eight-slot kernels -- every request against the oracle through
parity.RequestCheck (charger state and the provenance of prev_minfit included)."""
import pytest

from parity import VecSide, run_requests
from test_parity_edges import SLOT_EDGES, SLOT_SEED, crowded_relay_scenario, spec_com100

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_ragged_batch_matches_oracle():
    """test_emu_kernel.py::test_emulated_batch_of_different_networks_matches_oracle as it is, on the device: three networks of different
    N / T in one handle, 14 decisions, non-terminal node deaths, the topology peeks."""
    _torch()
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(7, 90, 60), synth_scenario(8, 130, 100), synth_scenario(9, 64, 64)]
    side = VecSide(scs, DEFAULT_MC_SPEC, 3)
    chk, deaths_seen = run_requests(side, scs, DEFAULT_MC_SPEC, 3, K=14, seed=5, check_topology=True)
    side.close()
    assert deaths_seen > 0, "the scenario set should exercise non-terminal node deaths"
    assert chk.n_cmp >= 20 and chk.n_noise == 0


@pytest.mark.parametrize("N", sorted(SLOT_EDGES))
def test_slot_edges_match_oracle(N):
    """One handle per node count, four networks each: both sides of every register-slot count, of the 256-node switch of the level
    search and of the 64-padding of the targets."""
    _torch()
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    T, M = SLOT_EDGES[N]
    i = sorted(SLOT_EDGES).index(N)
    scs = [synth_scenario(SLOT_SEED + i + 10 * e, N, T) for e in range(4)]
    side = VecSide(scs, DEFAULT_MC_SPEC, M)
    chk, _ = run_requests(side, scs, DEFAULT_MC_SPEC, M, K=8, seed=N, third=0.3, hatch=True)
    side.close()
    assert chk.n_cmp >= 16 and chk.n_prov >= 12 and chk.n_noise <= max(2, chk.n_cmp // 200)     # the sweep's cap


def test_d4_packet_cost_on_the_neighbour_list_path():
    """The one hop cost the simulator computes itself (Sim::e_send: a node with more than eight neighbours) past d0."""
    _torch()
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    sc = crowded_relay_scenario()
    side = VecSide([sc], DEFAULT_MC_SPEC, 2)
    chk, _ = run_requests(side, [sc], DEFAULT_MC_SPEC, 2, K=10, seed=3, third=0.3, check_topology=True)
    side.close()
    assert chk.n_cmp >= 6 and chk.n_noise == 0


# case -> (arguments of parity_sweep.run, least requests compared, least episodes finished): half of what a green run reports (1 415 / 109,
# 1 536 / 126, 1 839 / 269, 397 / 41 -- the work budget is counted, not timed, so the emulator and the device report the same)
RAGGED = [(33, 17), (64, 64), (65, 65), (128, 64), (129, 128), (200, 200)]
SWEEPS = {"ragged_budget": (dict(B=64, K=24, budget=1250, seed0=71000, sizes=RAGGED), 707, 54),
          "ragged_blocking": (dict(B=64, K=24, budget=0, seed0=71000, sizes=RAGGED), 768, 63),
          "com100_budget": (dict(B=96, K=24, budget=1250, seed0=72000, N=200, node_spec="com100"), 919, 134),
          "slots8_budget": (dict(B=32, K=16, budget=1250, seed0=73000, sizes=[(257, 129), (300, 150), (512, 100)]), 198, 20)}


@pytest.mark.parametrize("case", sorted(SWEEPS))
def test_parity_sweep_edges(case):
    """tests/parity_sweep.py, three chargers, whole episodes with resets: ragged batches across one, two and four register slots (with
    the default work budget and blocking), 200 nodes at com_range 100 m, and the eight-slot kernels in a ragged batch."""
    _torch()
    import parity_sweep
    kw, min_cmp, min_term = SWEEPS[case]
    kw = dict(kw, M=3)
    if kw.get("node_spec") == "com100":
        kw["node_spec"] = spec_com100()
    n_cmp, n_term, n_noise = parity_sweep.run(verbose=False, **kw)
    assert n_cmp >= min_cmp and n_term >= min_term and n_noise <= max(2, n_cmp // 200)
