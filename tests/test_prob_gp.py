"""prob_gp < 1 (Node.py:61: one random.random() per live node and second; packets only when the draw is below prob_gp) :
one body each, run here on the emulator (the unmodified HIP sources in the lockstep wavefront emulator of tests/emu) and by
tests/test_prob_gp_gpu.py on the device: against the reference runs of tests/golden/prob_gp/ (tools/gen_prob_gp_golden.py), against Python's own `random` after
every decision, and against the prob_gp == 1 kernels.  CPU only: launch modes on the emulator, the opt-in rules and the refusals."""
import os

import numpy as np
import pytest
import yaml

from parity import check_decision
from sides import EmuSide, PGP_DIR, PGP_NAMES, load_fixture, python_mt_state, scenario_from_prob_gp


def _load(name):
    return load_fixture("prob_gp/" + name)[0]


def test_fixtures_are_there_and_cover_what_they_should():
    assert len(PGP_NAMES) >= 10, PGP_NAMES
    pgps = {float(_load(n)["node_spec"][4]) for n in PGP_NAMES}
    assert {0.0, 0.1, 0.5, 0.7, 0.9} <= pgps
    z = _load("redundant_rev_m2_p05")
    assert int(z["rule4_skipped"]) >= 1                      # a node killed earlier in the same instant did not draw
    assert any(int(_load(n)["seed64"]) == 0 for n in PGP_NAMES)
    for n in PGP_NAMES:
        assert os.path.getsize(os.path.join(PGP_DIR, n + ".npz")) < 1 << 20


SEEDS = [0, 5, -5, -123456789, 2 ** 32, 2 ** 32 + 7, 2 ** 63 - 1, -2 ** 63]
PGP1_NAMES = ["six_m3_bs_charge_ongrid", "redundant_m2_deaths", "hanoi1000n50_m2_map64", "redundant_m2_maxtime130"]


def rng_state_after_the_warm_up_is_pythons(Side, seed):
    """random.seed(seed) followed by one draw per node and second of the warm-up (no node dies in it): word for word."""
    z = _load("six_m1_bs_charge_ongrid_p05")
    sc, mc = scenario_from_prob_gp(z, seed=seed)
    side = Side([sc], mc, 1, map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    side.reset()
    words, n = side.handle.rng_state()
    assert n[0] == int(z["rng_draws_reset"]) == sc.n_node * 100
    assert np.array_equal(words[0], python_mt_state(seed, int(n[0])))
    if seed == 5:
        assert np.array_equal(words[0], python_mt_state(-5, int(n[0])))     # random.seed takes abs(seed)
    side.close()


def kernel_matches_prob_gp_fixture(Side, name):
    z, sc, mc = load_fixture("prob_gp/" + name)
    seed = int(z["seed64"])
    side = Side([sc], mc, int(z["num_agent"]), map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    side.reset()
    assert side.rows()[0][0] == int(z["reset_agent"])
    nd = side.handle.nodes()
    assert np.array_equal(nd["status"][0], z["reset_node_status"])
    assert np.max(np.abs(nd["energy"][0] - z["reset_node_energy"]) / z["reset_node_energy"]) < 1e-9
    words, n = side.handle.rng_state()
    assert n[0] == int(z["rng_draws_reset"]) and np.array_equal(words[0], python_mt_state(seed, int(n[0])))
    noise = []
    for k in range(len(z["in_action"])):
        side.step([int(z["in_agent"][k])], z["in_action"][k][None])
        if z["is_none"][k]:
            agent, _, _, _, status = side.rows()[0]
            assert status == 1 and agent == -1
            break
        got = side.decision()
        # agent and terminal flag exact; the simulated time to the 1e-9 of check_decision (the fast-forwarded charger sub-steps of
        # the prob_gp == 1 path are closed forms too: a few ulps)
        assert got["agent_id"] == int(z["agent_id"][k]) and got["terminal"] == bool(z["terminal"][k]), (name, k)
        check_decision(z, k, got, where=name, noise=noise)
        if z["terminal"][k]:
            break                                            # (node state, draws included, is frozen once the network is declared dead)
        assert np.array_equal(got["node_status"], z["node_status"][k]), (name, k)
        words, n = side.handle.rng_state()
        assert n[0] == int(z["rng_draws"][k]), (name, k, int(n[0]), int(z["rng_draws"][k]))
        assert np.array_equal(words[0], python_mt_state(seed, int(n[0]))), (name, k, "generator words")
    # rewards that hang on the sign of a rounding residue of energyCS are far more common than with prob_gp 1: a node
    # that generated nothing for ten seconds keeps such a residue, and with prob_gp 0.1 most nodes do; each one was held to the
    # reference's algorithm on the product's own node state (parity._reward_depends_on_residue)
    assert len(noise) <= max(1, len(z["in_action"]) // 3), noise
    side.close()


def prob_gp_one_on_the_stochastic_kernels_is_bit_identical(Side, name):
    """An environment with prob_gp == 1 in a handle that runs the stochastic kernels (its neighbour has prob_gp 0.5) returns
    exactly what the plain handle returns, and its generator has taken one draw per live node and second."""
    z = load_fixture(name)[0]
    sc1, mc = scenario_from_prob_gp(z, seed=int(z["seed"]), stochastic=False)
    sc1s, _ = scenario_from_prob_gp(z, seed=int(z["seed"]), stochastic=True)
    other = load_fixture("prob_gp/six_m1_bs_charge_ongrid_p05")[1]
    kw = dict(map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    M = int(z["num_agent"])
    a = Side([sc1], mc, M, **kw); b = Side([sc1s, other], mc, M, **kw)
    a.reset(); b.reset()
    words, n = b.handle.rng_state()
    assert n[0] == sc1.n_node * int(z["warm_up"]) and np.array_equal(words[0], python_mt_state(int(z["seed"]), int(n[0])))
    for k in range(len(z["in_action"])):
        a.step([int(z["in_agent"][k])], z["in_action"][k][None])
        b.step([int(z["in_agent"][k]), -2], np.stack([z["in_action"][k], z["in_action"][k]]))
        ra = a.rows()[0]
        assert ra == b.rows()[0], (name, k)
        assert np.array_equal(a.obs_row(0), b.obs_row(0))
        na, nb = a.handle.nodes(), b.handle.nodes()
        for key in ("energy", "cs", "status", "level"):
            assert np.array_equal(na[key][0], nb[key][0][:sc1.n_node]), (name, k, key)
        if ra[3] or ra[0] < 0:
            break
    a.close(); b.close()


# ---- the bodies above on the emulator (tests/test_prob_gp_gpu.py: on the device)
@pytest.mark.parametrize("seed", SEEDS)
def test_rng_state_after_the_warm_up_is_pythons(hip_lib, seed):
    rng_state_after_the_warm_up_is_pythons(EmuSide, seed)


@pytest.mark.parametrize("name", PGP_NAMES)
def test_emulated_kernel_matches_prob_gp_fixture(hip_lib, name):
    kernel_matches_prob_gp_fixture(EmuSide, name)


@pytest.mark.parametrize("name", PGP1_NAMES)
def test_prob_gp_one_on_the_stochastic_kernels_is_bit_identical(hip_lib, name):
    prob_gp_one_on_the_stochastic_kernels_is_bit_identical(EmuSide, name)


def _requests(ev, acts, budget=0, deadline_us=0, rounds=400):
    """Per environment: the requests of K decisions driven by acts[k, e] (blocking when budget == deadline == 0)."""
    B, K = acts.shape[1], acts.shape[0]
    if budget:
        ev.h.set_step_budget(budget)
    if deadline_us:
        ev.h.set_step_deadline(deadline_us)
    ev.reset()
    hist = [[] for _ in range(B)]; nxt = np.zeros(B, dtype=int); busy = np.zeros(B, dtype=bool); done = np.zeros(B, dtype=bool)
    n_busy = 0
    for _ in range(rounds):
        if done.all():
            break
        ids = ev.agent_id.copy()
        ids[done | ((nxt >= K) & ~busy)] = -2
        act = np.stack([acts[min(nxt[e], K - 1), e] for e in range(B)])
        ev.step(ids, act)
        for e in range(B):
            if ids[e] == -2:
                continue
            if ev.status[e] == 4:
                if not busy[e]:
                    nxt[e] += 1
                busy[e] = True; n_busy += 1
                continue
            if not busy[e]:
                nxt[e] += 1
            busy[e] = False
            hist[e].append((int(ev.agent_id[e]), float(ev.now[e]), float(ev.reward[e]), int(ev.terminal[e])))
            if ev.terminal[e] or ev.agent_id[e] < 0 or nxt[e] >= K:
                done[e] = True
    assert done.all()
    return hist, n_busy


def test_budgeted_and_time_sliced_launches_return_the_blocking_requests(hip_lib):
    """prob_gp 0.5 with nodes dying: a work budget or a launch deadline only changes the call a request appears in (the reward to
    round-off: a suspension splits the reward accumulation of a grid service in two)."""
    z = _load("redundant_m2_p05"); z2 = _load("redundant_rev_m2_p05")
    scs = [scenario_from_prob_gp(z)[0], scenario_from_prob_gp(z2)[0], scenario_from_prob_gp(z, seed=-11)[0]]
    mc = scenario_from_prob_gp(z)[1]
    K = 14
    acts = np.random.RandomState(5).rand(K, 3, 3) * np.array([1.0, 1.0, 0.6])
    h0, _ = _requests(EmuSide(scs, mc, 2), acts)
    for kw in (dict(budget=300), dict(budget=4000, deadline_us=50), dict(deadline_us=30)):
        h1, busy = _requests(EmuSide(scs, mc, 2), acts, rounds=20000, **kw)
        assert busy > 0, kw
        for e in range(len(scs)):
            assert len(h1[e]) == len(h0[e]), (kw, e)
            for q0, q1 in zip(h0[e], h1[e]):
                assert q0[0] == q1[0] and q0[1] == q1[1] and q0[3] == q1[3], (kw, e, q0, q1)
                assert abs(q0[2] - q1[2]) <= 1e-9 * max(1.0, abs(q0[2])), (kw, e, q0, q1)


def test_scenario_opt_in_rules(tmp_path):
    from multi_agent_rl_wrsn_amd import DEFAULT_NODE_SPEC, Scenario, load_scenario_yaml
    spec = dict(DEFAULT_NODE_SPEC); spec["prob_gp"] = 0.3
    with pytest.raises(ValueError):
        Scenario(np.zeros((3, 2)), np.zeros((2, 2)), np.zeros(2), spec)
    s = Scenario(np.zeros((3, 2)), np.zeros((2, 2)), np.zeros(2), spec, seed=-4, stochastic_packets=True)
    assert s.stochastic_packets and s.seed == -4
    for bad in (2 ** 63, -2 ** 63 - 1):
        with pytest.raises(ValueError):
            Scenario(np.zeros((3, 2)), np.zeros((2, 2)), np.zeros(2), spec, seed=bad, stochastic_packets=True)
    spec2 = dict(spec); spec2["prob_gp"] = 1.5
    with pytest.raises(ValueError):
        Scenario(np.zeros((3, 2)), np.zeros((2, 2)), np.zeros(2), spec2, stochastic_packets=True)
    z = _load("hanoi1000n50_m2_p0_seed0")
    from multi_agent_rl_wrsn_amd.scenario import NODE_SPEC_KEYS
    d = {"node_phy_spe": {k: float(v) for k, v in zip(NODE_SPEC_KEYS, z["node_spec"])}, "seed": 2 ** 40 + 3,
         "max_time": float(z["max_time"]), "base_station": [float(v) for v in z["bs_xy"]],
         "nodes": z["node_xy"].tolist(), "targets": z["target_xy"].tolist()}
    p = tmp_path / "s.yaml"
    p.write_text(yaml.safe_dump(d))
    s = load_scenario_yaml(str(p))
    assert s.stochastic_packets and s.seed == 2 ** 40 + 3 and s.node_spec["prob_gp"] == 0.0
    d["node_phy_spe"]["prob_gp"] = 1.0
    p.write_text(yaml.safe_dump(d))
    assert not load_scenario_yaml(str(p)).stochastic_packets


def test_synth_scenario_passes_the_opt_in_through(hip_lib):
    from multi_agent_rl_wrsn_amd import DEFAULT_NODE_SPEC, synth_scenario
    spec = dict(DEFAULT_NODE_SPEC); spec["prob_gp"] = 0.7
    with pytest.raises(ValueError):
        synth_scenario(3, 40, 30, node_spec=spec)
    s = synth_scenario(3, 40, 30, node_spec=spec, stochastic_packets=True)
    assert s.stochastic_packets and s.seed == 3


def test_plain_call_still_refuses_prob_gp_below_one(hip_lib):
    """wrsn_set_scenario keeps refusing prob_gp != 1; the seeded call takes it; the generator is only tracked by stochastic handles."""
    import ctypes as C
    from emu_env import emu_lib
    from multi_agent_rl_wrsn_amd import _lib
    z = _load("six_m1_bs_charge_ongrid_p05")
    sc, mc = scenario_from_prob_gp(z)
    lib = emu_lib()
    h = _lib.RawHandle(lib, 1, sc.n_node, sc.n_target, 1, 100, 100.0)
    spec = (_lib.WrsnNodeSpec * 1)(); spec[0] = _lib.make_node_spec(sc.node_spec, sc.max_time)
    mcs = _lib.make_mc_spec(mc)
    nxy = np.ascontiguousarray(sc.node_xy); txy = np.ascontiguousarray(sc.target_xy); bs = np.ascontiguousarray(sc.bs_xy)
    rc = lib.wrsn_set_scenario(h._h, 0, 1, nxy.ctypes.data, txy.ctypes.data, bs.ctypes.data, None, None, spec, 1, C.byref(mcs), 0)
    assert rc == -1 and b"prob_gp" in lib.wrsn_last_error()
    rc = lib.wrsn_set_scenario_seeded(h._h, 0, 1, nxy.ctypes.data, txy.ctypes.data, bs.ctypes.data, None, None, spec, 1, C.byref(mcs), 0, None)
    assert rc == -1
    seed = np.array([7], dtype=np.int64)
    rc = lib.wrsn_set_scenario_seeded(h._h, 0, 1, nxy.ctypes.data, txy.ctypes.data, bs.ctypes.data, None, None, spec, 1, C.byref(mcs), 0, seed.ctypes.data)
    assert rc == 0
    h.close()
    spec[0].prob_gp = 1.0                                   # prob_gp 1 everywhere: the plain kernels, no generator to report
    h = _lib.RawHandle(lib, 1, sc.n_node, sc.n_target, 1, 100, 100.0)
    rc = lib.wrsn_set_scenario_seeded(h._h, 0, 1, nxy.ctypes.data, txy.ctypes.data, bs.ctypes.data, None, None, spec, 1, C.byref(mcs), 0, seed.ctypes.data)
    assert rc == 0
    with pytest.raises(_lib.WrsnError):
        h.rng_state()
    h.close()
