"""Edges of the kernels: one body each, run here on the emulator (the unmodified HIP sources on tests/emu) and by
tests/test_parity_edges_gpu.py on the device:
every request against the oracle through parity.RequestCheck -- status, level, energy, consumption rate, charger energy, exclusive
reward, reward, observation, and the provenance of prev_minfit.
  * the d > d0 arm of the packet cost (Node.py:107,114-115): com_range 100 m is past d0 = sqrt(efs / emp) = 87.7 m;
  * register-slot edges: node i lives in lane i & 63, slot i >> 6; node counts on both sides of every slot count the kernels are
    instantiated for (1, 2, 4, 8, 16), 256 / 257 also being the switch of the level search from node-set masks to the pushed
    frontier; target counts on both sides of the 64-padding;
  * environments of different slot counts in one handle, blocking and budgeted;
  * the pushed level search over a node that lives on the neighbour list (more than eight neighbours in a handle of more than 256 nodes);
  * tests/parity_sweep.py: whole episodes with masked resets, a table of cases per side.
Where the two sides differ it is in size only: the emulator steps single environments with the residue hatch off (its seeds were kept
because their runs need none), the device steps four networks per handle and allows the sweep's share of residue-dependent rewards."""
import numpy as np
import pytest

from conftest import golden_names, load_golden
from parity import run_requests
from sides import EmuSide

# N -> (T, chargers): T takes 64 and 65 once each, about N / 2 otherwise; 3 chargers up to 256 nodes, 5 up to 513, 8 at 1024
SLOT_EDGES = {64: (64, 3), 65: (65, 3), 128: (64, 3), 129: (65, 3), 256: (128, 3), 257: (129, 5), 512: (256, 5), 513: (257, 5), 1024: (512, 8)}
SLOT_SEED = 900                                             # i-th node count, environment e: seed 900 + i + 10 e
# per side: networks per handle, residue hatch, least requests compared / provenances traced, most residue-dependent rewards of n_cmp
SLOT_RUN = {"emu": (1, False, 4, 3, lambda n_cmp: 0), "gpu": (4, True, 16, 12, lambda n_cmp: max(2, n_cmp // 200))}     # (the sweep's cap)
COM100 = {"com_range": 100.0}
RAGGED_SLOTS = [(40, 30), (65, 65), (257, 129)]


def spec_com100():
    from multi_agent_rl_wrsn_amd.scenario import DEFAULT_NODE_SPEC
    return dict(DEFAULT_NODE_SPEC, **COM100)


def routed_hops(node_xy, bs_xy, level, com_range):
    """Node.find_receiver (Node.py:92-112) on the levels of the reset state, float64: the base station when it is in range, else the
    nearest neighbour one level down.  Length of every node's hop (nan: no receiver)."""
    xy = np.asarray(node_xy, dtype=np.float64); bs = np.asarray(bs_xy, dtype=np.float64)
    dbs = np.sqrt(((xy - bs) ** 2).sum(1))
    d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(2))
    hop = np.full(len(xy), np.nan)
    for i in range(len(xy)):
        if dbs[i] <= com_range:
            hop[i] = dbs[i]
            continue
        cand = [j for j in range(len(xy)) if j != i and d[i, j] <= com_range and level[j] >= 0 and level[j] < level[i]]
        if cand and level[i] >= 0:
            hop[i] = min(d[i, j] for j in cand)
    return hop


@pytest.mark.parametrize("name", [n for n in golden_names() if n.endswith("_com100")])
def test_com100_fixture_routes_packets_over_hops_longer_than_d0(name):
    """The fixtures that pin `et + emp d^4` to the reference must go on exercising it: at reset at least 5 routed hops exceed d0."""
    z = load_golden(name)
    spec = z["node_spec"]                                    # capacity, threshold, com_range, sen_range, prob_gp, package_size, er, et, efs, emp
    d0 = np.sqrt(spec[8] / spec[9])
    assert spec[2] > d0
    hop = routed_hops(z["node_xy"], z["bs_xy"], z["reset_node_level"], float(spec[2]))
    assert int((hop > d0).sum()) >= 5, (name, int((hop > d0).sum()), d0)


def test_both_com100_fixtures_are_present():
    assert len([n for n in golden_names() if n.endswith("_com100")]) == 2


def slot_edges_match_oracle(Side, N):
    """One handle per node count: both sides of every register-slot count, of the 256-node switch of the level search and of the
    64-padding of the targets."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    T, M = SLOT_EDGES[N]
    n_env, hatch, min_cmp, min_prov, noise_cap = SLOT_RUN[Side.name]
    scs = [synth_scenario(SLOT_SEED + sorted(SLOT_EDGES).index(N) + 10 * e, N, T) for e in range(n_env)]
    side = Side(scs, DEFAULT_MC_SPEC, M)
    chk, _ = run_requests(side, scs, DEFAULT_MC_SPEC, M, K=8, seed=N, third=0.3, hatch=hatch)
    side.close()
    assert chk.n_cmp >= min_cmp and chk.n_prov >= min_prov and chk.n_noise <= noise_cap(chk.n_cmp)


def ragged_batch_matches_oracle(Side):
    """Three networks of different N / T in one handle, 14 decisions, non-terminal node deaths, the topology peeks."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(7, 90, 60), synth_scenario(8, 130, 100), synth_scenario(9, 64, 64)]
    side = Side(scs, DEFAULT_MC_SPEC, 3)
    chk, deaths_seen = run_requests(side, scs, DEFAULT_MC_SPEC, 3, K=14, seed=5, check_topology=True)
    side.close()
    assert deaths_seen > 0, "the scenario set should exercise non-terminal node deaths"
    assert chk.n_cmp >= 20 and chk.n_noise == 0


def test_create_refuses_1025_nodes():
    from emu_env import emu_lib
    from multi_agent_rl_wrsn_amd import _lib
    with pytest.raises(_lib.WrsnError):
        _lib.RawHandle(emu_lib(), 1, 1025, 64, 3, 100, 100.0, 0, 0, 0)
    _lib.RawHandle(emu_lib(), 1, 1024, 64, 3, 100, 100.0, 0, 0, 0).close()


D4_NETWORKS = [(900, 60, 40), (901, 100, 80)]               # seed, nodes, targets


def d4_packet_cost_matches_oracle(Side, seed, n, t):
    """Synthetic networks at com_range 100 m: hops between d0 and com_range pay et + emp d^4, in the topology kernel's table (the
    closed-form seconds) and in the simulator's hop cost (the exact packet walk)."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    sc = synth_scenario(seed, n, t, node_spec=spec_com100())
    side = Side([sc], DEFAULT_MC_SPEC, 3)
    chk, _ = run_requests(side, [sc], DEFAULT_MC_SPEC, 3, K=12, seed=seed, check_topology=True)
    side.close()
    from wrsn_oracle import OracleWRSN
    o = OracleWRSN(sc.node_xy, sc.target_xy, sc.bs_xy, sc.node_spec, DEFAULT_MC_SPEC, sc.max_time, 3); o.reset()
    d0 = np.sqrt(sc.node_spec["efs"] / sc.node_spec["emp"])
    assert int((routed_hops(sc.node_xy, sc.bs_xy, o.nodes()["level"], 100.0) > d0).sum()) >= 5      # the network does use the arm
    assert chk.n_cmp >= 6 and chk.n_noise == 0


def crowded_relay_scenario():
    """A relay with more than eight neighbours whose only way down is a hop longer than d0: the base station at (500, 500), a direct
    node 95 m east of it, the relay another 95 m east, and a cluster of nine leaves within 30 m of the relay on its far side (more than
    100 m from the direct node, so one level above the relay).  More than eight neighbours takes a node off the packed neighbour words
    onto the sorted neighbour list (find_receiver's second branch), the one place where the simulator computes a hop cost itself
    (Sim::e_send) instead of reading the topology kernel's table.  A short chain to the west keeps a second branch alive."""
    from multi_agent_rl_wrsn_amd.scenario import Scenario
    nodes = [[595.0, 500.0], [690.0, 500.0]]
    for k in range(9):
        a = np.deg2rad(-60.0 + 15.0 * k); r = 20.0 + (k % 3) * 4.0
        nodes.append([690.0 + r * np.cos(a), 500.0 + r * np.sin(a)])
    nodes += [[420.0, 510.0], [345.0, 525.0], [270.0, 515.0]]
    xy = np.array(nodes)
    targets = [[x + 5.0, y + 3.0] for x, y in xy[2:11]] + [[262.0, 520.0], [340.0, 530.0]]
    return Scenario(node_xy=xy, target_xy=np.array(targets), bs_xy=np.array([500.0, 500.0]), node_spec=spec_com100(), name="crowded_relay")


def d4_packet_cost_on_the_neighbour_list_path(Side):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    from wrsn_oracle import OracleWRSN
    sc = crowded_relay_scenario()
    o = OracleWRSN(sc.node_xy, sc.target_xy, sc.bs_xy, sc.node_spec, DEFAULT_MC_SPEC, sc.max_time, 2); o.reset()
    d0 = np.sqrt(sc.node_spec["efs"] / sc.node_spec["emp"])
    hop = routed_hops(sc.node_xy, sc.bs_xy, o.nodes()["level"], 100.0)
    assert o.topology()["degree"][1] > 8 and hop[1] > d0      # the relay: on the neighbour list, and its hop pays et + emp d^4
    side = Side([sc], DEFAULT_MC_SPEC, 2)
    chk, _ = run_requests(side, [sc], DEFAULT_MC_SPEC, 2, K=10, seed=3, third=0.3, check_topology=True)
    side.close()
    assert chk.n_cmp >= 6 and chk.n_noise == 0


def pushed_level_search_takes_the_neighbour_list(Side):
    """The level search of handles with more than 256 nodes is pushed from the frontier, and a frontier node with more than eight
    neighbours pushes along its neighbour list instead of its packed words: the crowded relay (14 nodes) next to a 257-node network, whose
    size puts the handle on that search.  Reset state and every request against the oracle -- the levels of the nine leaves come through
    the relay alone."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    from wrsn_oracle import OracleWRSN
    scs = [crowded_relay_scenario(), synth_scenario(SLOT_SEED + 57, 257, 129)]
    sc = scs[0]
    o = OracleWRSN(sc.node_xy, sc.target_xy, sc.bs_xy, sc.node_spec, DEFAULT_MC_SPEC, sc.max_time, 2); o.reset()
    lv, deg = o.nodes()["level"], o.topology()["degree"]
    # the branch is reached: a node on the neighbour list is on a frontier (it has a level) and is the only way to nodes one level up
    assert max(s.n_node for s in scs) > 256 and deg[1] > 8 and lv[1] >= 1
    d = np.sqrt(((sc.node_xy[:, None] - sc.node_xy[None]) ** 2).sum(2))
    leaves = [i for i in range(2, 11) if lv[i] == lv[1] + 1 and not any(lv[j] == lv[1] and j != 1 and d[i, j] <= 100.0 for j in range(sc.n_node))]
    assert len(leaves) == 9, (lv, leaves)
    side = Side(scs, DEFAULT_MC_SPEC, 2)
    chk, _ = run_requests(side, scs, DEFAULT_MC_SPEC, 2, K=8, seed=11, third=0.3, check_topology=True, hatch=Side.name == "gpu")
    side.close()
    assert chk.n_cmp >= 8 and chk.n_noise <= (0 if Side.name == "emu" else 2)


RAGGED_BUDGETS = [0, 1250, 40]


def ragged_slot_counts_in_one_handle_match_oracle(Side, budget):
    """1, 2 and 8 register slots per lane side by side in a handle built for the largest: blocking, with the default work budget, and
    with one so small that most steps run out of it (they report status 4 and go on in the next call; these short steps never
    exhaust the default budget)."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(SLOT_SEED + i, n, t) for i, (n, t) in enumerate(RAGGED_SLOTS)]
    side = Side(scs, DEFAULT_MC_SPEC, 3, step_budget=budget)
    chk, _ = run_requests(side, scs, DEFAULT_MC_SPEC, 3, K=10, seed=17, third=0.3, check_topology=True)
    side.close()
    assert chk.n_cmp >= 15 and chk.n_prov >= 10 and chk.n_noise == 0
    assert (chk.n_flight > 0) == (budget == 40)


# side -> case -> (arguments of parity_sweep.run, least requests compared, least episodes finished, most residue-dependent rewards of n_cmp).
# Emulator: small sizes, whole episodes with masked resets, so that prev_minfit is traced across resets, through steps that stay in flight
# over several calls, and (time-sliced) through actions that wait in the latch; no request needs the residue hatch.  Device: ragged
# batches across one, two and four register slots (with the default work budget and blocking), 200 nodes at com_range 100 m, and the
# eight-slot kernels in a ragged batch; the least counts are half of what a green run reports (1 415 / 109, 1 536 / 126, 1 839 / 269,
# 397 / 41 -- the work budget is counted, not timed, so the emulator and the device report the same), the cap is the sweep's.
RAGGED = [(33, 17), (64, 64), (65, 65), (128, 64), (129, 128), (200, 200)]
_NONE, _SWEEP_CAP = (lambda n_cmp: 0), (lambda n_cmp: max(2, n_cmp // 200))
SWEEPS = {"emu": {"ragged_budget": (dict(B=12, K=150, budget=150, seed0=71000, sizes=[(33, 17), (64, 64), (65, 65), (129, 128)]), 100, 3, _NONE),
                  "com100_time_sliced": (dict(B=5, K=400, seed0=72000, N=70, deadline_us=20, node_spec="com100"), 100, 3, _NONE)},
          "gpu": {"ragged_budget": (dict(B=64, K=24, budget=1250, seed0=71000, sizes=RAGGED), 707, 54, _SWEEP_CAP),
                  "ragged_blocking": (dict(B=64, K=24, budget=0, seed0=71000, sizes=RAGGED), 768, 63, _SWEEP_CAP),
                  "com100_budget": (dict(B=96, K=24, budget=1250, seed0=72000, N=200, node_spec="com100"), 919, 134, _SWEEP_CAP),
                  "slots8_budget": (dict(B=32, K=16, budget=1250, seed0=73000, sizes=[(257, 129), (300, 150), (512, 100)]), 198, 20, _SWEEP_CAP)}}


def parity_sweep_edges(Side, case):
    """tests/parity_sweep.py, three chargers, whole episodes with resets."""
    import parity_sweep
    kw, min_cmp, min_term, noise_cap = SWEEPS[Side.name][case]
    kw = dict(kw, M=3, side=Side)
    if kw.get("node_spec") == "com100":
        kw["node_spec"] = spec_com100()
    n_cmp, n_term, n_noise = parity_sweep.run(verbose=False, **kw)
    assert n_cmp >= min_cmp and n_term >= min_term and n_noise <= noise_cap(n_cmp)


# ---- the bodies above on the emulator (tests/test_parity_edges_gpu.py: on the device)
@pytest.mark.parametrize("N", sorted(SLOT_EDGES))
def test_emulated_slot_edges_match_oracle(N, hip_lib):
    slot_edges_match_oracle(EmuSide, N)


def test_emulated_ragged_batch_matches_oracle(hip_lib):
    ragged_batch_matches_oracle(EmuSide)


@pytest.mark.parametrize("seed,n,t", D4_NETWORKS)
def test_emulated_d4_packet_cost_matches_oracle(seed, n, t, hip_lib):
    d4_packet_cost_matches_oracle(EmuSide, seed, n, t)


def test_emulated_d4_packet_cost_on_the_neighbour_list_path(hip_lib):
    d4_packet_cost_on_the_neighbour_list_path(EmuSide)


def test_emulated_pushed_level_search_takes_the_neighbour_list(hip_lib):
    pushed_level_search_takes_the_neighbour_list(EmuSide)


@pytest.mark.parametrize("budget", RAGGED_BUDGETS)
def test_emulated_ragged_slot_counts_in_one_handle_match_oracle(budget, hip_lib):
    ragged_slot_counts_in_one_handle_match_oracle(EmuSide, budget)


@pytest.mark.parametrize("case", ["ragged_budget", "com100_time_sliced"])
def test_parity_sweep_on_the_emulator(case, hip_lib):
    parity_sweep_edges(EmuSide, case)
