"""prob_gp < 1 on a real MI355X: the bodies of tests/test_prob_gp.py on the device (the reference runs of tests/golden/prob_gp/, Python's
own `random` after every decision, the prob_gp == 1 kernels), and at sizes the emulator cannot reach a mixed batch of 512, auto-reset
episodes, and the launch machinery (budgets, time slices, the pipelined step call) at 4096 environments."""
import numpy as np
import pytest

import test_prob_gp as body
from sides import VecSide, load_fixture, need_gpu, python_mt_state, scenario_from_prob_gp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", body.SEEDS)
def test_rng_state_after_the_warm_up_is_pythons(seed):
    body.rng_state_after_the_warm_up_is_pythons(VecSide, seed)


@pytest.mark.parametrize("name", body.PGP_NAMES)
def test_hip_matches_prob_gp_fixture(name):
    body.kernel_matches_prob_gp_fixture(VecSide, name)


@pytest.mark.parametrize("name", body.PGP1_NAMES)
def test_prob_gp_one_on_the_stochastic_kernels_is_bit_identical(name):
    body.prob_gp_one_on_the_stochastic_kernels_is_bit_identical(VecSide, name)


def _mixed_batch(B, N=200):
    from multi_agent_rl_wrsn_amd import DEFAULT_NODE_SPEC, synth_scenario
    pg = [0.0, 0.3, 0.7, 1.0]
    seeds = [0, -3, 2 ** 32 + 5, 12345, -(2 ** 40), 7]
    scs = []
    for e in range(B):
        spec = dict(DEFAULT_NODE_SPEC); spec["prob_gp"] = pg[e % 4]
        sc = synth_scenario(21000 + e // 4, N, N, node_spec=spec, stochastic_packets=True)
        sc.seed = seeds[e % len(seeds)] if e < 24 else 1000 + e
        scs.append(sc)
    return scs


def test_mixed_batch_of_512_environments():
    """512 synthetic 200-node networks, prob_gp 0 / 0.3 / 0.7 / 1, mixed seeds: the generator after the warm-up (no node dies in it) is
    Python's after N x 100 draws; prob_gp 0 never lowers a node's energy; prob_gp 1 equals the plain handle bit for bit."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN
    B, K, M = 512, 10, 3
    scs = _mixed_batch(B)
    env = VecWRSN(scs, None, M)
    r = env.reset(); env.synchronize()
    words, n = env._h.rng_state()
    for e in range(B):
        assert n[e] == 200 * 100, e
        assert np.array_equal(words[e], python_mt_state(scs[e].seed, 200 * 100)), e
    one = [e for e in range(B) if e % 4 == 3]
    from multi_agent_rl_wrsn_amd.scenario import Scenario
    plain = VecWRSN([Scenario(scs[e].node_xy, scs[e].target_xy, scs[e].bs_xy, scs[e].node_spec, scs[e].max_time, scs[e].seed) for e in one], None, M)
    rp = plain.reset(); plain.synchronize()
    g = torch.Generator().manual_seed(11)
    acts = torch.rand((K, B, 3), generator=g, dtype=torch.float64)
    e0 = env.nodes()["energy"][0::4].copy()
    for k in range(K):
        ids = r["agent_id"].clone(); ids[ids < 0] = -2
        r = env.step(ids, acts[k]); env.synchronize()
        ids_p = rp["agent_id"].clone(); ids_p[ids_p < 0] = -2
        rp = plain.step(ids_p, acts[k][one]); plain.synchronize()
        for key in ("agent_id", "now", "reward", "terminal", "status"):
            assert torch.equal(r[key][one].cpu(), rp[key].cpu()), (k, key)
        assert torch.equal(r["state"][one].cpu(), rp["state"].cpu()), k
        nd, ndp = env.nodes(), plain.nodes()
        assert np.array_equal(nd["energy"][one], ndp["energy"]) and np.array_equal(nd["cs"][one], ndp["cs"]), k
        e1 = nd["energy"][0::4]
        assert np.all(e1 >= e0), k                             # prob_gp 0: no packet is ever sent
        e0 = e1.copy()
    env.close(); plain.close()


def test_auto_reset_episodes_replay_bit_for_bit():
    """Every reset restores the generator with the rest of the post-warm-up snapshot (NetworkIO.py:22-24): the episodes of an environment
    driven by the same actions are the same, deaths and packet draws included."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN
    z = load_fixture("prob_gp/redundant_m2_p05")[0]
    scs = [scenario_from_prob_gp(z, seed=s)[0] for s in (3, 4, 5, 6)] * 16
    B = len(scs)
    env = VecWRSN(scs, scenario_from_prob_gp(z)[1], 2, auto_reset=True)
    r = env.reset(); env.synchronize()
    acts = torch.tensor(np.random.RandomState(2).rand(400, 3) * np.array([1.0, 1.0, 0.6]))
    step_no = np.zeros(B, dtype=int)                         # decisions into the current episode
    episodes = [[[]] for _ in range(B)]
    for it in range(300):
        act = acts[torch.from_numpy(step_no)]
        ids = r["agent_id"].clone(); ids[ids < 0] = 0
        r = env.step(ids, act); env.synchronize()
        st = r["status"].cpu().numpy(); a = r["agent_id"].cpu().numpy(); now = r["now"].cpu().numpy(); rew = r["reward"].cpu().numpy()
        term = r["terminal"].cpu().numpy()
        for e in range(B):
            if st[e] == 3:
                episodes[e].append([]); step_no[e] = 0
                continue
            episodes[e][-1].append((int(a[e]), float(now[e]), float(rew[e]), int(term[e])))
            step_no[e] += 1
    n_cmp = 0
    for e in range(B):
        done = [ep for ep in episodes[e][:-1] if ep]
        for ep in done[1:]:
            assert ep == done[0], e
            n_cmp += 1
    assert n_cmp >= B
    env.close()


def test_launch_modes_return_the_blocking_requests_at_4096():
    """4096 environments, prob_gp 0.5: budgeted launches, time slices and the pipelined step call (the default for a call that renders,
    up to two rounds of the wave slots; here the pipeline runs over the first 1 024) report the requests of blocking launches."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import DEFAULT_NODE_SPEC, VecWRSN, synth_scenario
    spec = dict(DEFAULT_NODE_SPEC); spec["prob_gp"] = 0.5
    uniq = [synth_scenario(23000 + u, 200, 200, node_spec=spec, stochastic_packets=True) for u in range(64)]
    B, K = 4096, 6
    scs = []
    for e in range(B):
        sc = uniq[e % 64]
        scs.append(type(sc)(sc.node_xy, sc.target_xy, sc.bs_xy, sc.node_spec, sc.max_time, 100 + e, stochastic_packets=True))
    g = torch.Generator().manual_seed(4)
    acts = torch.rand((K, B, 3), generator=g, dtype=torch.float64)

    def run(nenv, **kw):
        env = VecWRSN(scs[:nenv], None, 3, reuse_obs=True, **kw)
        r = env.reset(); env.synchronize()
        n_given = np.zeros(nenv, dtype=int); hist = [[] for _ in range(nenv)]; n_busy = 0
        for it in range(120 * K):
            fresh = (r["status"] != 4).cpu().numpy()
            if np.all(fresh & (n_given >= K)):
                break
            act = acts[torch.from_numpy(np.minimum(n_given, K - 1)), torch.arange(nenv)]
            ids = r["agent_id"].clone()
            ids[torch.from_numpy(fresh & (n_given >= K)).to(ids.device)] = -2
            r = env.step(ids, act); env.synchronize()
            n_given += (fresh & (n_given < K)).astype(int)
            st = r["status"].cpu().numpy(); a = r["agent_id"].cpu().numpy(); now = r["now"].cpu().numpy(); rew = r["reward"].cpu().numpy()
            osum = r["state"].sum(dim=(1, 2, 3)).cpu().numpy()
            n_busy += int((st == 4).sum())
            for e in range(nenv):
                if ids[e] != -2 and st[e] != 4:
                    hist[e].append((int(a[e]), float(now[e]), float(rew[e]), float(osum[e]) if a[e] >= 0 else 0.0))
        env.close()
        return hist, n_busy

    def same(h0, h1, n):
        for e in range(n):
            assert len(h1[e]) == len(h0[e]), e
            for q0, q1 in zip(h0[e], h1[e]):
                assert q0[0] == q1[0] and q0[1] == q1[1], (e, q0, q1)
                assert abs(q0[2] - q1[2]) <= 1e-7 * max(1.0, abs(q0[2])) and abs(q0[3] - q1[3]) <= 1e-6 * max(1.0, abs(q0[3])), (e, q0, q1)
    h0, _ = run(B)
    h1, busy1 = run(B, step_budget=1250)
    assert busy1 > 0
    same(h0, h1, B)
    h2, busy2 = run(B, step_deadline_us=300)
    assert busy2 > 0
    same(h0, h2, B)
    h3, _ = run(1024, step_budget=1250)                       # 1 024 environments: the two-stage pipeline
    same(h0, h3, 1024)
