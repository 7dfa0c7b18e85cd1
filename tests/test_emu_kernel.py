"""Kernel logic without a GPU: the unmodified HIP sources (csrc/wrsn_api.hip + wrsn_sim.h) compiled by g++ against
the lockstep wavefront emulator of tests/emu and driven through the same C-ABI binding as the product.
Checks the device code paths (topology build, warm-up, event order, closed-form ticks, exact packet walk, routing
cache rebuild, reward softmax, widest-path fitness, observation) against the golden fixtures and the oracle."""
import numpy as np
import pytest

from conftest import golden_names, load_golden
from parity import check_decision, close, replay_reference_fixture
from sides import EmuSide


FAST = [n for n in golden_names() if "n150" not in n and "n200" not in n]


@pytest.mark.parametrize("name", FAST)
def test_emulated_kernel_matches_reference_fixture(name):
    replay_reference_fixture(EmuSide, name)


def test_emulated_batch_of_different_networks_matches_oracle(hip_lib):
    """B = 3 synthetic networks of different sizes in one handle (ragged N/T), several chargers, whole episodes with
    non-terminal node deaths: exercises per-environment sizes, the routing-cache rebuild and the level BFS."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    from wrsn_oracle import OracleWRSN
    scs = [synth_scenario(7, 90, 60), synth_scenario(8, 130, 100), synth_scenario(9, 64, 64)]
    M = 3
    ev = EmuSide(scs, DEFAULT_MC_SPEC, M)
    ors = [OracleWRSN(s.node_xy, s.target_xy, s.bs_xy, s.node_spec, DEFAULT_MC_SPEC, s.max_time, M) for s in scs]
    ev.reset()
    last = [o.reset() for o in ors]
    topo = ev.h.topology()
    for e, o in enumerate(ors):
        t = o.topology()
        assert np.array_equal(topo["degree"][e, :o.N], t["degree"])
        assert np.array_equal(topo["n_cover"][e, :o.N], t["n_cover"]) and np.array_equal(topo["direct"][e, :o.N], t["direct"])
    rng = np.random.RandomState(5)
    done = [False] * len(scs)
    deaths_seen = 0
    for step in range(14):
        act = rng.rand(len(scs), 3)
        ids = [(-2 if done[e] else (-1 if last[e]["agent_id"] is None else last[e]["agent_id"])) for e in range(len(scs))]
        ev.step(ids, act)
        nd = ev.nodes(); m = ev.mcs()
        for e, o in enumerate(ors):
            if done[e]:
                continue
            last[e] = o.step(last[e]["agent_id"], act[e])
            r = last[e]
            assert int(ev.agent_id[e]) == (-1 if r["agent_id"] is None else r["agent_id"]), (step, e)
            assert bool(ev.terminal[e]) == r["terminal"] and close(ev.now[e], r["now"], rtol=1e-9), (step, e)
            if r["terminal"]:
                done[e] = True
                continue
            on = o.nodes(); om = o.mcs()
            assert np.array_equal(nd["status"][e, :o.N], on["status"]), (step, e)
            assert np.array_equal(nd["level"][e, :o.N], on["level"]), (step, e)
            assert close(nd["energy"][e, :o.N], on["energy"]) and close(nd["cs"][e, :o.N], on["cs"], atol=1e-9), (step, e)
            assert close(m["energy"][e], om["energy"], atol=1e-6) and close(m["excl"][e], om["excl"], atol=1e-7), (step, e)
            assert close(ev.reward[e], r["reward"], atol=1e-9), (step, e, ev.reward[e], r["reward"])
            assert np.max(np.abs(ev.obs[e] - r["state"])) <= 1e-5 * max(1.0, np.abs(r["state"]).max()), (step, e)
            deaths_seen += int((on["status"] == 0).sum() > 0)
        if all(done):
            break
    assert deaths_seen > 0, "the scenario set should exercise non-terminal node deaths"


def test_emulated_auto_reset_and_untouched_rows(hip_lib):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    sc = synth_scenario(21, 70, 50)
    ev = EmuSide([sc, sc], DEFAULT_MC_SPEC, 2)
    ev.reset()
    e0 = ev.nodes()["energy"].copy()
    rng = np.random.RandomState(3)
    # env 1 is never touched (-2): its state must not move
    ids = np.array([0, -2], dtype=np.int32)
    seen_reset = False
    for _ in range(40):
        ev.step(ids, rng.rand(2, 3), auto_reset=True)
        assert np.array_equal(ev.nodes()["energy"][1], e0[1])
        if int(ev.status[0]) == 3:                      # auto-reset happened: back to the snapshot
            seen_reset = True
            assert int(ev.agent_id[0]) == 0 and float(ev.now[0]) == 100.0 and not ev.terminal[0]
            assert np.array_equal(ev.nodes()["energy"][0], e0[0])
            break
        ids[0] = ev.agent_id[0]
    assert seen_reset


@pytest.mark.parametrize("name", ["hanoi1000n50_m3_s1", "hanoi1000n50_m3_cap1500_mcdeath", "six_m3_bs_charge_ongrid", "hanoi1000n100_m3_s5"])
def test_emulated_step_budget_returns_the_same_requests(name):
    """wrsn_set_step_budget: a WRSN.step that exceeds the work budget of a launch reports status 4 and goes on in the
    next launch; the sequence of requests (and the state behind them) is the one of the blocking call."""
    z = load_golden(name)
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    sc, mc = scenario_from_golden(z)
    ev = EmuSide([sc], mc, int(z["num_agent"]), map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    ev.h.set_step_budget(25)
    ev.reset()
    n_susp = 0
    for k in range(len(z["in_action"])):
        ev.step([int(z["in_agent"][k])], z["in_action"][k][None])
        guard = 0
        while int(ev.status[0]) == 4:
            assert int(ev.agent_id[0]) == -1 and not bool(ev.terminal[0])
            n_susp += 1; guard += 1
            assert guard < 10000
            ev.step([-1], np.zeros((1, 3)))                  # the row is ignored while the step is in flight
        if z["is_none"][k]:
            assert int(ev.status[0]) == 1 and int(ev.agent_id[0]) == -1
            break
        assert int(ev.status[0]) == 0
        if np.isinf(z["reward"][k]):
            continue
        check_decision(z, k, ev.decision(), where=name + " (budget)", noise=[])
        if z["terminal"][k]:
            break
    assert n_susp > 0


def test_emulated_step_budget_equals_blocking_on_a_200_node_network_with_guarded_seconds():
    """A synthetic 200-node environment whose run passes through seconds that are looked at one by one (a node within a few
    seconds of its threshold: safe horizon 0) while the launch budget runs out: the budgeted requests equal the blocking
    ones.  (Regression: an exhausted budget once turned "no second may be skipped" into "skip one".)"""
    import torch
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    K, e = 12, 92
    acts = torch.rand((K, 96, 3), generator=torch.Generator().manual_seed(3), dtype=torch.float64).numpy()[:, e]
    sc = [synth_scenario(500 + e, 200, 200)]

    def run(budget):
        ev = EmuSide(sc, DEFAULT_MC_SPEC, 3)
        if budget:
            ev.h.set_step_budget(budget)
        ev.reset(with_obs=False)
        hist, k, busy, cur = [], 0, False, ev.agent_id.copy()
        for _ in range(4000):
            if k >= K and not busy:
                break
            ev.step(cur, acts[min(k, K - 1)][None], with_obs=False)
            if int(ev.status[0]) == 4:
                k += 0 if busy else 1
                busy = True
                continue
            k += 0 if busy else 1
            busy = False
            hist.append((int(ev.agent_id[0]), float(ev.now[0]), float(ev.reward[0]), int(ev.terminal[0])))
            if ev.terminal[0] or ev.agent_id[0] < 0:
                break
            cur = ev.agent_id.copy()
        return hist, ev.nodes()["energy"][0].copy()

    h0, e0 = run(0)
    h1, e1 = run(400)
    assert len(h0) == len(h1) and len(h0) >= 4
    for q0, q1 in zip(h0, h1):
        assert q0[0] == q1[0] and q0[1] == q1[1] and q0[3] == q1[3], (q0, q1)
        assert abs(q0[2] - q1[2]) <= 1e-7 * max(1.0, abs(q0[2])), (q0, q1)
    assert np.abs(e0 - e1).max() <= 1e-8 * np.abs(e0).max()


def test_emulated_step_deadline_argument_and_same_requests():
    """wrsn_set_step_deadline: argument checking, and (the emulator has no wall clock -- its stand-in ticks once per reading -- so
    the deadline falls somewhere inside a step) the requests of a run with a deadline equal the fixture's, like any budgeted run."""
    from multi_agent_rl_wrsn_amd import _lib
    z = load_golden("hanoi1000n50_m3_s1")
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    sc, mc = scenario_from_golden(z)
    ev = EmuSide([sc], mc, int(z["num_agent"]), map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    with pytest.raises(_lib.WrsnError):
        ev.h.set_step_deadline(-1)
    ev.h.set_step_budget(100000)
    ev.h.set_step_deadline(1)                                # 100 readings of the stand-in clock
    ev.reset()
    n_susp = 0
    for k in range(len(z["in_action"])):
        ev.step([int(z["in_agent"][k])], z["in_action"][k][None])
        guard = 0
        while int(ev.status[0]) == 4:
            n_susp += 1; guard += 1
            assert guard < 100000
            ev.step([-1], np.zeros((1, 3)))
        if z["is_none"][k]:
            break
        if not np.isinf(z["reward"][k]):
            check_decision(z, k, ev.decision(), where="deadline", noise=[])
        if z["terminal"][k]:
            break
    assert n_susp > 0


def test_emulated_rollout_table_matches_host_accumulation():
    """wrsn_rollout_table: returns per charger / finished episodes / lifetimes / completed steps accumulated by the step
    kernel equal what a host loop over the requests accumulates (RolloutStats layout)."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(40 + e, 70, 60) for e in range(3)]
    M = 2
    ev = EmuSide(scs, DEFAULT_MC_SPEC, M)
    ev.reset()
    want = np.zeros((3, M + 3))
    rng = np.random.RandomState(2)
    for k in range(25):
        ids = ev.agent_id.copy()
        ev.step(ids, rng.rand(3, 3), with_obs=False, auto_reset=True)
        for e in range(3):
            if ev.status[e] == 3:
                continue                                       # auto-reset: no WRSN.step was executed
            if ev.agent_id[e] >= 0:
                want[e, ev.agent_id[e]] += ev.reward[e]
            if ev.terminal[e]:
                want[e, M] += 1; want[e, M + 1] += ev.now[e]
            want[e, M + 2] += 1
    got = np.zeros((3, M + 3))
    ev.h.rollout_table(got.ctypes.data, True)
    assert want[:, M + 2].sum() > 0 and want[:, M].sum() > 0
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    ev.h.rollout_table(got.ctypes.data, False)
    assert not got.any()


def _density_cases(rng, G, node_cell):
    """logits, a probability map peaked on a node's cell, a flat map with ties at the percentile, a one-hot map"""
    peaked = np.full((G, G), 1e-9); peaked[node_cell] = 0.5; peaked[(node_cell[0] + 1) % G, node_cell[1]] = 0.25
    peaked += rng.rand(G, G) * 1e-6; peaked /= peaked.sum()
    onehot = np.zeros((G, G)); onehot[G // 3, G // 2] = 1.0
    return [rng.randn(G, G) * 2.0, peaked, np.full((G, G), 1.0 / (G * G)), onehot, rng.rand(G, G)]


@pytest.mark.parametrize("G", [100, 64])
def test_emulated_density_map_to_action(G):
    """wrsn_density_action vs the NumPy/SciPy restatement of WRSN.py:229-297: arg-max cell / box / third component exact,
    charging spot inside the box with an objective value not below SciPy's L-BFGS-B (its spot is not pinned)."""
    import density_ref
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    sc = synth_scenario(11, 120, 100)
    ev = EmuSide([sc] * 5, DEFAULT_MC_SPEC, 2, map_size=G)
    ev.reset(with_obs=False)
    rng = np.random.RandomState(3)
    for k in range(3):                                       # some dynamics first: energies / consumption rates differ per node
        ev.step(ev.agent_id.copy(), rng.rand(5, 3), with_obs=False)
    info = ev.env_info(); nd = ev.nodes()
    frame = [info["xmin"][0], info["xmax"][0], info["ymin"][0], info["ymax"][0]]
    mc = DEFAULT_MC_SPEC
    alive = nd["status"][0] == 1
    cellx = int((sc.node_xy[5, 0] - frame[0]) / (frame[1] - frame[0]) * G); celly = int((sc.node_xy[5, 1] - frame[2]) / (frame[3] - frame[2]) * G)
    maps = _density_cases(rng, G, (min(cellx, G - 1), min(celly, G - 1)))
    dm = np.ascontiguousarray(np.stack(maps)); ids = np.zeros(5, dtype=np.int32); ids[4] = -1
    out = np.full((5, 3), -7.0)
    ev.h.density_action(ids.ctypes.data, dm.ctypes.data, out.ctypes.data)
    assert np.all(out[4] == -7.0)                            # skipped row
    for e in range(4):
        ref = density_ref.density_map_to_action(density_ref.normalise(maps[e]), frame, sc.node_xy, alive, nd["energy"][0], nd["cs"][0],
                                                float(sc.node_spec["threshold"]), mc["charging_range"], mc["alpha"], mc["beta"])
        assert abs(out[e, 2] - ref["third"]) <= 1e-12 * ref["third"], (e, out[e, 2], ref["third"])
        spot = np.array([out[e, 0] * (frame[1] - frame[0]) + frame[0], out[e, 1] * (frame[3] - frame[2]) + frame[2]])
        (lx, ux), (ly, uy) = ref["bounds"]
        tol = 1e-9 * (ux - lx)
        assert lx - tol <= spot[0] <= ux + tol and ly - tol <= spot[1] <= uy + tol, (e, spot, ref["bounds"])
        val = density_ref.objective(spot, sc.node_xy, alive, nd["energy"][0], nd["cs"][0], float(sc.node_spec["threshold"]),
                                    mc["charging_range"], mc["alpha"], mc["beta"])
        assert val >= ref["objective"] * (1 - 1e-9) - 1e-300, (e, val, ref["objective"])


def test_emulated_step_budget_untouched_and_reset_rows():
    """Bookkeeping of the in-flight list (wrsn_set_step_budget): an environment left untouched (agent -2) while its step
    is in flight stays in flight and finishes later with the blocking result; a reset of an in-flight environment drops
    the step; other environments of the batch are not disturbed."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(60 + e, 80, 70) for e in range(4)]
    act = np.array([[0.3, 0.6, 0.9], [0.7, 0.2, 0.8], [0.5, 0.5, 0.7], [0.2, 0.8, 0.95]])

    ref = EmuSide(scs, DEFAULT_MC_SPEC, 2)                      # blocking run: what every finished step must return
    ref.reset(with_obs=False)
    ids0 = ref.agent_id.copy()
    ref.step(ids0, act, with_obs=False)
    want = (ref.agent_id.copy(), ref.now.copy(), ref.reward.copy())

    ev = EmuSide(scs, DEFAULT_MC_SPEC, 2)
    ev.h.set_step_budget(40)
    ev.reset(with_obs=False)
    ev.step(ids0, act, with_obs=False)
    assert (ev.status == 4).all()                            # budget far below one step: everybody is in flight
    done = np.zeros(4, dtype=bool); got_agent = np.full(4, -9); got_now = np.zeros(4); got_rew = np.zeros(4)
    # environment 1 is left untouched for a while, environment 3 is reset while in flight
    mask = np.zeros(4, dtype=np.uint8); mask[3] = 1
    ev.h.reset(mask.ctypes.data, **ev._ptrs(False))
    assert ev.now[3] == 100.0 and ev.agent_id[3] == ids0[3]
    for it in range(4000):
        ids = np.full(4, -1, dtype=np.int32)
        ids[done] = -2; ids[3] = -2
        if it < 50: ids[1] = -2
        ev.step(ids, np.zeros((4, 3)), with_obs=False)
        for e in (0, 1, 2):
            if ids[e] == -2 or done[e]: continue
            if ev.status[e] != 4:
                done[e] = True; got_agent[e] = ev.agent_id[e]; got_now[e] = ev.now[e]; got_rew[e] = ev.reward[e]
        if done[:3].all(): break
    assert done[:3].all()
    assert np.array_equal(got_agent[:3], want[0][:3]) and np.array_equal(got_now[:3], want[1][:3])
    assert np.allclose(got_rew[:3], want[2][:3], rtol=1e-7, atol=1e-12)
    # the reset environment starts a fresh step and finishes it like the blocking run
    ids = np.full(4, -2, dtype=np.int32); ids[3] = ids0[3]
    ev.step(ids, act, with_obs=False)
    for it in range(4000):
        if ev.status[3] != 4: break
        ids[3] = -1
        ev.step(ids, np.zeros((4, 3)), with_obs=False)
    assert ev.status[3] != 4 and ev.agent_id[3] == want[0][3] and ev.now[3] == want[1][3]


@pytest.mark.parametrize("order", [0, 1])
def test_emulated_step_budget_handles_every_environment_once_per_launch(order):
    """Ownership of an environment inside a budgeted launch (2 B blocks: listed in-flight environments first, everybody
    else behind): whatever order the blocks run in, an environment executes at most one WRSN.step per launch, the rollout
    table equals the host-side accumulation of the returned requests, and the requests equal the blocking run's."""
    from emu_env import emu_lib
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    B, M, K = 5, 2, 30
    scs = [synth_scenario(80 + e, 70, 60) for e in range(B)]
    rng = np.random.RandomState(9)
    acts = rng.rand(K, B, 3)

    def run(budget):
        ev = EmuSide(scs, DEFAULT_MC_SPEC, M)
        if budget: ev.h.set_step_budget(budget)
        ev.reset(with_obs=False)
        tab = np.zeros((B, M + 3)); want = np.zeros((B, M + 3)); hist = [[] for _ in range(B)]
        nxt = np.zeros(B, dtype=int); busy = np.zeros(B, dtype=bool); done = np.zeros(B, dtype=bool)
        cur = ev.agent_id.copy()
        for it in range(4000):
            if done.all(): break
            ids = cur.copy(); ids[done] = -2
            act = np.stack([acts[min(nxt[e], K - 1), e] for e in range(B)])
            before = (ev.agent_id.copy(), ev.reward.copy(), ev.now.copy())
            ev.step(ids, act, with_obs=False)
            ev.h.rollout_table(tab.ctypes.data, True)
            assert tab[:, M + 2].max() <= 1.0                 # never two WRSN.step calls of one environment in a launch
            for e in range(B):
                if done[e]:                                   # untouched row: every output keeps its value
                    assert tab[e].sum() == 0 and ev.agent_id[e] == before[0][e] and ev.reward[e] == before[1][e] and ev.now[e] == before[2][e]
                    continue
                if not busy[e]: nxt[e] += 1
                if ev.status[e] == 4:
                    busy[e] = True; assert tab[e].sum() == 0
                    continue
                busy[e] = False
                assert tab[e, M + 2] == 1.0
                if ev.agent_id[e] >= 0: want[e, ev.agent_id[e]] = ev.reward[e]
                want[e, M] = float(ev.terminal[e]); want[e, M + 1] = ev.now[e] if ev.terminal[e] else 0.0; want[e, M + 2] = 1.0
                assert np.allclose(tab[e], want[e], rtol=1e-12, atol=0); want[e] = 0
                hist[e].append((int(ev.agent_id[e]), float(ev.now[e]), float(ev.reward[e]), int(ev.terminal[e])))
                if ev.terminal[e] or ev.agent_id[e] < 0 or nxt[e] >= K: done[e] = True
            cur = ev.agent_id.copy()
        assert done.all()
        return hist

    lib = emu_lib()
    ref = run(0)
    lib.emu_set_block_order(order)
    try:
        got = run(30)
    finally:
        lib.emu_set_block_order(0)
    for e in range(B):
        assert len(got[e]) == len(ref[e])
        for a, b in zip(ref[e], got[e]):
            assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and abs(a[2] - b[2]) <= 1e-7 * max(1.0, abs(a[2])), (e, a, b)


def test_emulated_untouched_and_unmasked_rows_keep_their_request():
    """agent_id -2 in step() and a zero mask byte in reset(mask) leave a row's outputs alone -- the pending request id
    included -- so `r = reset(mask); step(r.agent_id, a)` is safe for the environments that were not reset."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(90 + e, 70, 60) for e in range(3)]
    ev = EmuSide(scs, DEFAULT_MC_SPEC, 2)
    ev.reset()
    rng = np.random.RandomState(1)
    for _ in range(3):
        ev.step(ev.agent_id.copy(), rng.rand(3, 3))
    keep = (ev.agent_id.copy(), ev.reward.copy(), ev.now.copy(), ev.terminal.copy(), ev.status.copy(), ev.obs.copy())
    assert (keep[0] >= 0).all()
    mask = np.array([0, 1, 0], dtype=np.uint8)
    ev.h.reset(mask.ctypes.data, **ev._ptrs(True))
    for e in (0, 2):
        assert ev.agent_id[e] == keep[0][e] and ev.reward[e] == keep[1][e] and ev.now[e] == keep[2][e] and np.array_equal(ev.obs[e], keep[5][e])
    assert ev.agent_id[1] == 0 and ev.now[1] == 100.0 and ev.reward[1] == 0.0
    keep1 = (ev.agent_id.copy(), ev.reward.copy(), ev.now.copy(), ev.obs.copy())
    ids = np.array([-2, int(ev.agent_id[1]), -2], dtype=np.int32)
    ev.step(ids, rng.rand(3, 3))
    for e in (0, 2):
        assert ev.agent_id[e] == keep1[0][e] and ev.reward[e] == keep1[1][e] and ev.now[e] == keep1[2][e] and np.array_equal(ev.obs[e], keep1[3][e])


@pytest.mark.parametrize("G", [12, 96, 128])
def test_emulated_observation_at_other_map_sizes(G):
    """get_state (WRSN.py:130-186) at map sizes that exercise the corners of the observation kernel's tiling: fewer rows than one
    matrix-core band (12), exactly three bands and no VALU rows (96), a full fourth band on the store wave (128)."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    from wrsn_oracle import OracleWRSN
    sc = synth_scenario(33, 90, 70)
    M = 3
    ev = EmuSide([sc], DEFAULT_MC_SPEC, M, map_size=G)
    o = OracleWRSN(sc.node_xy, sc.target_xy, sc.bs_xy, sc.node_spec, DEFAULT_MC_SPEC, sc.max_time, M, map_size=G)
    ev.reset(); r = o.reset()
    assert np.max(np.abs(ev.obs[0] - r["state"])) <= 1e-5 * max(1.0, np.abs(r["state"]).max())
    rng = np.random.RandomState(4)
    for k in range(5):
        a = rng.rand(3)
        ev.step([int(ev.agent_id[0])], a[None]); r = o.step(r["agent_id"], a)
        if r["terminal"] or r["agent_id"] is None:
            break
        assert int(ev.agent_id[0]) == r["agent_id"]
        assert np.max(np.abs(ev.obs[0] - r["state"])) <= 1e-5 * max(1.0, np.abs(r["state"]).max()), k


def test_emulated_launch_order_with_many_environments():
    """More environments than sort threads x 2 (the register / wave-shuffle / LDS variant of the launch-order sort): every environment
    is handled exactly once per launch and the requests equal those of the same environments stepped one by one."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    B, M = 520, 2
    uniq = [synth_scenario(600 + u, 24, 16) for u in range(8)]
    scs = [uniq[e % 8] for e in range(B)]
    ev = EmuSide(scs, DEFAULT_MC_SPEC, M, map_size=8)
    ev.h.set_step_budget(50)
    ev.reset(with_obs=False)
    rng = np.random.RandomState(12)
    acts = rng.rand(3, 8, 3)
    tab = np.zeros((B, M + 3))
    hist = [[] for _ in range(B)]
    nxt = np.zeros(B, dtype=int); busy = np.zeros(B, dtype=bool)
    cur = ev.agent_id.copy()
    for it in range(400):
        done = (nxt >= 3) & ~busy
        if done.all(): break
        ids = cur.copy(); ids[done] = -2
        act = np.stack([acts[min(nxt[e], 2), e % 8] for e in range(B)])
        ev.step(ids, act, with_obs=False)
        ev.h.rollout_table(tab.ctypes.data, True)
        assert tab[:, M + 2].max() <= 1.0
        for e in range(B):
            if done[e]: continue
            if not busy[e]: nxt[e] += 1
            busy[e] = ev.status[e] == 4
            if not busy[e]:
                assert tab[e, M + 2] == 1.0
                hist[e].append((int(ev.agent_id[e]), float(ev.now[e]), int(ev.terminal[e])))
                if ev.terminal[e] or ev.agent_id[e] < 0: nxt[e] = 3
        cur = ev.agent_id.copy()
    assert ((nxt >= 3) & ~busy).all()
    for e in range(8, B):                                    # replicas of a scenario with the same actions agree
        assert hist[e] == hist[e % 8], e


def test_emulated_observation_reuse_is_bit_identical():
    """wrsn_set_obs_reuse: map 1 of a row is left alone when no simulated second passed since it was rendered there -- the result
    equals the full render bit for bit, a render into another buffer in between does not confuse it, and a caller that does
    modify its buffer (reuse off) still gets full renders."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(50 + e, 70, 60) for e in range(3)]
    M, G = 3, 20
    a = EmuSide(scs, DEFAULT_MC_SPEC, M, map_size=G); b = EmuSide(scs, DEFAULT_MC_SPEC, M, map_size=G)
    b.h.set_obs_reuse(False)
    a.reset(); b.reset()
    assert np.array_equal(a.obs, b.obs)
    rng = np.random.RandomState(8)
    other = np.zeros_like(a.obs)
    zero_time = 0
    for k in range(14):
        act = rng.rand(3, 3)
        ids = a.agent_id.copy(); now0 = a.now.copy()
        b.obs[:] = -5.0                                       # the caller of b scribbles over its buffer: b renders in full every time
        a.step(ids, act, auto_reset=True); b.step(ids, act, auto_reset=True)
        zero_time += int(((a.now == now0) & (a.status == 0) & (a.agent_id >= 0)).sum())
        rows = a.agent_id >= 0
        assert np.array_equal(a.obs[rows], b.obs[rows]), k
        if k % 3 == 1:                                        # a render elsewhere moves the remembered address: the next one is full again
            agents = np.maximum(a.agent_id, 0).astype(np.int32)
            a.h.render(agents.ctypes.data, other.ctypes.data)
            assert np.array_equal(other[rows][:, 0], a.obs[rows][:, 0])
    assert zero_time >= 3


def test_emulated_work_queue_launches_return_the_same_requests():
    """wrsn_set_step_deadline = work-queue launches: persistent waves hand the environments out among themselves in a cyclic order until
    the common deadline of the launch; an environment nobody reaches is not touched -- its action waits in the latch over as many launches
    as it takes, its row says "in flight".  With auto-reset, rows marked -2 and a masked reset of an environment whose action is still
    latched: per environment the sequence of requests is the blocking run's (only the call that reports a request differs)."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    B, M, G = 5, 2, 12
    scs = [synth_scenario(300 + e, 70, 60) for e in range(B)]

    def act_of(e, n):
        return np.random.RandomState(1000 * e + n).rand(3)

    def run(deadline_us, calls, pause):
        ev = EmuSide(scs, DEFAULT_MC_SPEC, M, map_size=G)
        if deadline_us:
            ev.h.set_step_deadline(deadline_us)
        ev.reset()
        hist = [[] for _ in range(B)]; n_flight = 0; n_given = np.zeros(B, dtype=int)
        for it in range(calls):
            ids = ev.agent_id.copy()
            act = np.stack([act_of(e, n_given[e]) for e in range(B)])
            fresh = (ev.status != 4)                          # rows that carry a request: the action passed now starts their next WRSN.step
            if pause and it % 7 == 3:
                ids[1] = -2
            keep = (ev.agent_id[1], ev.now[1], ev.reward[1], ev.status[1])
            ev.step(ids, act, auto_reset=True)
            if ids[1] == -2:
                assert (ev.agent_id[1], ev.now[1], ev.reward[1], ev.status[1]) == keep
            for e in range(B):
                if ids[e] == -2:
                    continue
                if fresh[e]:
                    n_given[e] += 1                            # (also counts the ignored row of an auto-reset call: both runs do the same)
                if ev.status[e] == 4:
                    n_flight += 1
                else:
                    hist[e].append((int(ev.status[e]), int(ev.agent_id[e]), float(ev.now[e]), float(ev.reward[e]), int(ev.terminal[e])))
        return hist, n_flight
    full, nf0 = run(0, 120, False)
    assert nf0 == 0
    for pause in (False, True):
        q, n_flight = run(20, 700, pause)                      # 40 readings of the stand-in clock (50 ticks each) per launch: a fraction of one WRSN.step
        assert n_flight > 200
        for e in range(B):
            n = min(len(full[e]), len(q[e]))
            assert n >= 15 and sum(x[4] for x in q[e][:n]) >= 1, (e, n)
            for a, b in zip(full[e][:n], q[e][:n]):
                assert a[:3] == b[:3] and a[4] == b[4] and abs(a[3] - b[3]) <= 1e-7 * max(1.0, abs(a[3])), (e, a, b)   # a suspension splits a closed form / re-bases the float32 priorities: ~1e-9
    # a masked reset drops a latched action: the environment answers the reset, then takes the NEXT action it is given
    ev = EmuSide(scs, DEFAULT_MC_SPEC, M, map_size=G)
    ev.h.set_step_deadline(1)
    ev.reset()
    ev.step(ev.agent_id.copy(), np.full((B, 3), 0.9), auto_reset=True)
    untouched = [e for e in range(B) if ev.status[e] == 4 and ev.now[e] == 100.0 and ev.env_info()["n_events"][e] == ev.env_info()["n_events"].min()]
    assert len(untouched) >= 1
    e = untouched[-1]
    mask = np.zeros(B, dtype=np.uint8); mask[e] = 1
    ev.h.reset(mask.ctypes.data, **ev._ptrs(True))
    assert ev.agent_id[e] == 0 and ev.now[e] == 100.0
    ref = EmuSide([scs[e]], DEFAULT_MC_SPEC, M, map_size=G); ref.reset(); ref.step([0], np.array([[0.2, 0.3, 0.1]]))
    ids = np.full(B, -2, dtype=np.int32); ids[e] = 0
    act = np.zeros((B, 3)); act[e] = [0.2, 0.3, 0.1]
    for it in range(3000):
        ev.step(ids, act, auto_reset=False)
        if ev.status[e] != 4:
            break
        ids[e] = -1
    assert ev.status[e] == 0 and ev.agent_id[e] == ref.agent_id[0] and ev.now[e] == ref.now[0] and abs(ev.reward[e] - ref.reward[0]) < 1e-12
