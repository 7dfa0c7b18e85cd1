"""`evaluate_policy`, the policies and the trainer's episode log (multi_agent_rl_wrsn_amd/evaluate.py, ippo.py) on the emulated library.

The bodies take a factory of environments: this module builds them on EmuSide through the adapter of tests/episode_ref.py,
tests/test_evaluate_gpu.py builds VecWRSN.  B = 8 networks of 33 nodes whose nodes hold 1 000 J instead of 10 800 J: under any policy
here such a network dies after 280 to 500 simulated seconds, four to nine launches, and max_time = 320 s lies between those lifetimes, so
with time_limit=None both ways of ending occur.  Every comparison is of bytes: the reference evaluator does the ledger's float64 adds
in the ledger's order with torch ops, using only calls that existed before the ledger (`step`, `reset(mask)`)."""
import numpy as np
import pytest
from sides import EmuSide, FIELDS

import episode_ref as E

MAX_TIME, CAPACITY = 320.0, 1000.0
RESULT_KEYS = ("lifetime", "ep_return", "decisions", "ended", "record", "launches")


def scenarios(B, seed=500, max_time=MAX_TIME):
    from multi_agent_rl_wrsn_amd import DEFAULT_NODE_SPEC, synth_scenario
    spec = dict(DEFAULT_NODE_SPEC, capacity=CAPACITY)
    return [synth_scenario(seed + e, 33, 30, node_spec=spec, max_time=max_time) for e in range(B)]


def emu_env(B=8, max_time=MAX_TIME, auto_reset=False):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    return E.emu_eval_vec(EmuSide(scenarios(B, max_time=max_time), DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True, auto_reset=auto_reset))


def fresh_actors(env):
    import torch
    from multi_agent_rl_wrsn_amd import build_entity_networks, pack_entity_actor
    torch.manual_seed(5)
    Actor, _ = build_entity_networks(env.num_agent)
    return torch.stack([pack_entity_actor(Actor()) for _ in range(env.num_agent)]).to(env.device).contiguous()


def policies(env):
    """Policies that make progress on every network: draws from a seeded generator.  (A deterministic policy that repeats an action of
    zero duration -- the mode of freshly built actors, the heuristic at a node that is already full -- is handed the same request again
    at the same instant, in the reference too; `evaluate_policy` then ends by `max_launches`, which test 2 checks.)"""
    import torch
    from multi_agent_rl_wrsn_amd import EntityPolicy, UniformPolicy
    gen = lambda: torch.Generator(device=env.device).manual_seed(3)
    return {"uniform": UniformPolicy(gen()), "sampled": EntityPolicy(fresh_actors(env), deterministic=False, generator=gen())}


def named_policies(env):
    """The two deterministic policies: the heuristic as the kernel's rule stands, and the mode (eps == NULL) of freshly built actors.
    Both can stand still (see `policies`), so their runs are capped and the partial logs are what is compared."""
    from multi_agent_rl_wrsn_amd import EntityPolicy, HeuristicPolicy
    return {"heuristic": HeuristicPolicy(), "mode": EntityPolicy(fresh_actors(env), deterministic=True)}


def reference_evaluate(env, policy, episodes, time_limit, poll=8, max_launches=100000):
    """What evaluate_policy must return (or, at the launch cap, hand back as the partial log), from `step`, `reset(mask)` and
    elementwise torch alone."""
    t = env.torch
    B, M, E_ = env.num_env, env.num_agent, episodes
    dev = env.device
    z = lambda shape, dt: t.zeros(shape, dtype=dt, device=dev)
    run_ret, run_dec, finished = z((B, M), t.float64), z((B, M), t.int32), z((B,), t.int64)
    out = dict(lifetime=z((E_, B), t.float64), ep_return=z((E_, B, M), t.float64), decisions=z((E_, B, M), t.int32), ended=z((E_, B), t.int32),
               record=t.full((E_, B), 0, dtype=t.int32, device=dev))
    ids = env.reset()["agent_id"].clone()
    launches = 0
    while True:
        r = env.step(ids, policy(env, ids))
        agent, status, now, reward, terminal = (r[k].clone() for k in ("agent_id", "status", "now", "reward", "terminal"))
        stepped = ids != -2
        flying = stepped & (status == 4)
        term = stepped & ~flying & (terminal != 0)
        fresh = stepped & ~flying & (terminal == 0)
        rows = t.nonzero(fresh & (agent >= 0) & (agent < M)).flatten()
        cols = agent[rows].long()
        run_ret[rows, cols] = run_ret[rows, cols] + reward[rows]
        run_dec[rows, cols] = run_dec[rows, cols] + 1
        code = t.where(term, 1, t.where(fresh & (status == 1), 3, t.where(fresh & (now >= time_limit) & (time_limit > 0), 2, 0)))
        rows = t.nonzero(code > 0).flatten()
        k = finished[rows]
        assert bool((k < E_).all())
        out["lifetime"][k, rows] = now[rows]; out["ended"][k, rows] = code[rows].int()
        out["ep_return"][k, rows] = run_ret[rows]; out["decisions"][k, rows] = run_dec[rows]; out["record"][k, rows] = -1
        finished[rows] += 1
        run_ret[rows] = 0; run_dec[rows] = 0
        restart = (code > 0) & (finished < E_)
        ids = t.where(code > 0, -2, t.where(flying, -1, t.where(fresh, agent, ids))).int()
        r = env.reset(mask=restart.to(t.uint8))
        ids = t.where(restart, r["agent_id"], ids).int().contiguous()
        launches += 1
        if (launches % poll == 0 or launches >= max_launches) and bool((finished >= E_).all()):
            break
        if launches >= max_launches:
            break
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["launches"] = np.array(launches)
    res["finished"] = finished.int().cpu().numpy()
    res["running_return"], res["running_decisions"] = run_ret.cpu().numpy(), run_dec.cpu().numpy()
    return res


# ------------------------------------------------------------------------------------------------------------ 1. determinism, reference
def evaluation_is_deterministic_and_matches_the_reference(make_env, which):
    """Two runs on two identically built environments give equal bytes, and both equal the reference evaluator on a third; both ways of
    ending occur and the summary describes the arrays."""
    from multi_agent_rl_wrsn_amd import evaluate_policy
    envs = [make_env() for _ in range(3)]
    runs = [evaluate_policy(env, policies(env)[which], episodes=2, max_launches=400) for env in envs[:2]]
    ref = reference_evaluate(envs[2], policies(envs[2])[which], 2, MAX_TIME)
    for k in RESULT_KEYS:
        assert E.same(runs[0][k], runs[1][k]), (which, k)
        assert E.same(runs[0][k], ref[k]), (which, k, runs[0][k], ref[k])
    got = runs[0]
    assert got["lifetime"].shape == (2, 8) and got["ep_return"].shape == (2, 8, 3) and (got["lifetime"] > 0).all()
    assert set(got["ended"].reshape(-1).tolist()) == {1, 2}, got["ended"]
    s = got["summary"]
    assert s["episodes"] == 16 and s["lifetime_mean"] == float(got["lifetime"].mean()) and s["lifetime_median"] == float(np.median(got["lifetime"]))
    assert s["lifetime_min"] <= s["lifetime_median"] <= s["lifetime_max"] and len(s["return_per_charger"]) == 3
    assert abs(sum(s["ended"].values()) - 1.0) < 1e-12 and s["ended"]["terminal"] == float((got["ended"] == 1).mean())
    return envs


@pytest.mark.parametrize("which", ["uniform", "sampled"])
def test_emulated_evaluation_is_deterministic_and_matches_the_reference(which):
    for env in evaluation_is_deterministic_and_matches_the_reference(emu_env, which):
        env.side.close()


def named_policies_are_deterministic_and_match_the_reference(make_env, which, cap):
    """HeuristicPolicy and EntityPolicy(deterministic=True) of freshly built actors, two episodes, at most `cap` launches: the result --
    the full one, or the partial log of LaunchCapReached with `finished` -- is equal byte for byte on two identically built
    environments and equal to the reference evaluator's on a third, the sums of the episodes in progress included.  Requests were
    booked, no parked environment is reported as standing still, and at the cap some environment is."""
    from multi_agent_rl_wrsn_amd import evaluate_policy
    from multi_agent_rl_wrsn_amd.evaluate import LaunchCapReached
    envs = [make_env() for _ in range(3)]
    runs = []
    for env in envs[:2]:
        try:
            res = evaluate_policy(env, named_policies(env)[which], episodes=2, max_launches=cap)
            res["finished"] = np.full(env.num_env, 2, np.int32)
            res["running_return"], res["running_decisions"] = np.zeros((env.num_env, 3)), np.zeros((env.num_env, 3), np.int32)
        except LaunchCapReached as ex:
            res = ex.result
            assert int(res["launches"]) == cap and (res["finished"] < 2).any()
            assert (res["standing"][res["finished"] >= 2] == 0).all() and res["standing"].sum() > 0, (res["standing"], res["finished"])
        runs.append(res)
    ref = reference_evaluate(envs[2], named_policies(envs[2])[which], 2, MAX_TIME, max_launches=cap)
    for k in RESULT_KEYS + ("finished", "running_return", "running_decisions"):
        assert E.same(runs[0][k], runs[1][k]), (which, k)
        assert E.same(runs[0][k], ref[k]), (which, k, runs[0][k], ref[k])
    got = runs[0]
    assert got["finished"].sum() + got["running_decisions"].sum() > cap and (got["lifetime"][0][got["finished"] >= 1] > 0).all()
    return envs


@pytest.mark.parametrize("which,cap", [("heuristic", 48), ("mode", 24)])
def test_emulated_named_policies_are_deterministic_and_match_the_reference(which, cap):
    for env in named_policies_are_deterministic_and_match_the_reference(emu_env, which, cap):
        env.side.close()


def pooled_evaluation(make_env):
    """With a pool set, finished environments restart in the record the handle draws: `record` is -1 for the first episode (the
    environment's own scenario) and pool_draw(seed, e, 0, P) for the second; the heuristic with min_charge finishes everywhere."""
    import torch
    from multi_agent_rl_wrsn_amd import HeuristicPolicy, evaluate_policy, pool_draw
    env = make_env()
    env.reset()
    pool = env.save_envs()
    env.set_pool(pool, seed=7)
    got = evaluate_policy(env, HeuristicPolicy(min_charge=0.05), episodes=2, max_launches=400)
    B = env.num_env
    assert (got["record"][0] == -1).all() and got["record"][1].tolist() == [pool_draw(7, e, 0, B) for e in range(B)]
    assert (got["lifetime"] > 0).all() and set(got["ended"].reshape(-1).tolist()) <= {1, 2}
    return env


def test_emulated_pooled_evaluation():
    pooled_evaluation(emu_env).side.close()


# ------------------------------------------------------------------------------------------------------------ 2. the other policies, errors
def policies_and_errors(make_env, make_wrong_envs):
    """The sampled and the uniform policy run and are reproducible from their generators; the launch cap raises RuntimeError; an
    environment without entities or with auto-reset raises ValueError."""
    import torch
    from multi_agent_rl_wrsn_amd import EntityPolicy, HeuristicPolicy, UniformPolicy, evaluate_policy
    env = make_env()
    gen = lambda: torch.Generator(device=env.device).manual_seed(3)
    a = evaluate_policy(env, UniformPolicy(gen()), episodes=1, max_launches=400)
    b = evaluate_policy(env, UniformPolicy(gen()), episodes=1, poll=1, max_launches=400)
    for k in RESULT_KEYS[:-1]:                                 # the same episodes whatever the polling interval
        assert E.same(a[k], b[k]), k
    assert b["launches"] <= a["launches"] and a["launches"] % 8 == 0
    h = HeuristicPolicy(0.5)(env, env.reset()["agent_id"])     # the heuristic through the policy interface: float64 [B, 3] in the frame
    assert tuple(h.shape) == (env.num_env, 3) and h.dtype == torch.float64 and bool(((h >= 0) & (h <= 1)).all())
    with pytest.raises(RuntimeError) as ei:
        evaluate_policy(env, HeuristicPolicy(), episodes=2, max_launches=2)
    assert int(ei.value.result["launches"]) == 2 and (ei.value.result["finished"] == 0).all()
    for wrong in make_wrong_envs():
        with pytest.raises(ValueError):
            evaluate_policy(wrong, HeuristicPolicy())
    return env


def test_emulated_policies_and_errors():
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    made = []

    def wrong():
        made.append(emu_env(2, auto_reset=True))
        made.append(E.emu_eval_vec(EmuSide(scenarios(2), DEFAULT_MC_SPEC, 3, map_size=12, render=True, entities=False)))
        return made

    made.append(policies_and_errors(emu_env, wrong))
    for env in made:
        env.side.close()


# ------------------------------------------------------------------------------------------------------------ 3. the trainer
def trainer_logs_episodes(make_env, args, roll_launches):
    """Two BatchedEntityIPPO (every fused option) from one seed on one environment: the first with log_episodes=True really rolls out
    and trains; the second, without, is fed copies of the first one's buffers at the tail of every roll-out (the device of
    tests/test_entity_prepare.py: the slot a transition gets is an atomic counter's answer, so two roll-outs of the device are not
    comparable).  The rows of the first gain exactly `avg_ep_lifetime`, `avg_ep_lens` and `episodes`, equal to what a host loop over
    the requests of its launches gives; batches, packed nets and `_adam` after train(1) are equal bit for bit; `evaluate_episodes` on
    the trainer's own environment raises."""
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, pack_entity_actor, pack_entity_critic
    env = make_env()
    B, M = env.num_env, env.num_agent
    algos = []
    for log_episodes in (True, False):
        torch.manual_seed(11)
        algos.append(BatchedEntityIPPO(args, env, device=str(env.device), fused_policy=True, fused_update=True, joint_update=True, fused_prepare=True,
                                       log_episodes=log_episodes))
    a, b = algos
    assert b._ledger is None and a._ledger is not None
    with pytest.raises(ValueError):
        a.evaluate_episodes(env)
    kept, stored, launches, marks = ("state", "action", "next_state", "reward", "logp", "count"), [], [], []
    tail, step = a._prepare_batches, env.step

    def logging_step(ids, act):
        r = step(ids, act)
        launches.append((ids.cpu().numpy().copy(), {k: r[k].cpu().numpy().copy() for k in FIELDS}))
        return r

    def keeping():
        stored.append(({k: getattr(a.buffers, k).clone() for k in kept}, np.random.get_state()))
        marks.append(len(launches))
        return tail()

    def replay():
        snap, rng = stored[min(replay.k, len(stored) - 1)]
        replay.k += 1
        for k in kept:
            getattr(b.buffers, k).copy_(snap[k])
        np.random.set_state(rng)

    replay.k = 0
    env.step, a._prepare_batches = logging_step, keeping
    b.step_batch, b.buffers.clear, b._req = replay, (lambda keep_pending=False: None), {}
    np.random.seed(3)
    batches, rows = [], []
    for t in algos:
        batches.append(t.roll_out(max_launches=roll_launches))
        rows.append(t.train(1))
    env.step = step
    assert len(stored) == replay.k == 3 and len(marks) == 3
    for c in range(M):
        for k in batches[0][c]:
            assert E.same(batches[0][c][k].cpu().numpy(), batches[1][c][k].cpu().numpy()), (c, k)
        assert torch.equal(pack_entity_actor(a.actors[c]), pack_entity_actor(b.actors[c])), c
        assert torch.equal(pack_entity_critic(a.critics[c]), pack_entity_critic(b.critics[c])), c
        for k in ("m_a", "v_a", "m_c", "v_c"):
            assert torch.equal(a._adam[c][k], b._adam[c][k]), (c, k)
        assert a._adam[c]["step"] == b._adam[c]["step"] > 0
    new = {"avg_ep_lifetime", "avg_ep_lens", "episodes"}
    assert len(rows[0]) == len(rows[1]) == 2 * M
    for x, y in zip(rows[0], rows[1]):
        assert set(x) == set(y) | new and not (set(y) & new)
        assert {k: v for k, v in y.items() if k != "sps"} == {k: x[k] for k in y if k != "sps"}
    # the host loop over the requests: one ledger call after the reset, one per launch; read and emptied where a roll-out ended
    host, states = E.HostLedger(B, M, a._ledger.episodes, 0), E.RowStates(B)
    states.after_reset()
    host.collect(states, {k: np.zeros(B) for k in FIELDS}, consume=False)
    want, lo = [], 0
    for hi in marks[1:]:                                       # train() reads the log after ITS roll-outs: the first read covers roll_out() too
        for ids, req in launches[lo:hi]:
            states.after_step(ids, req); host.collect(states, req, consume=False)
        lo = hi
        fin = host.a["finished"]
        kept_mask = np.arange(host.E)[:, None] < np.minimum(fin, host.E)[None, :]
        life, dec = host.a["lifetime"][kept_mask], host.a["decisions"][kept_mask]
        want.append((float(life.mean()) if life.size else float("nan"), float(dec.mean()) if dec.size else float("nan"), int(fin.sum())))
        for k in ("finished", "dropped", "lifetime", "ep_return", "decisions", "ended", "record"):
            host.a[k][...] = 0
    assert all(w[2] > 0 for w in want)                         # episodes did close in both iterations
    for i, x in enumerate(rows[0]):
        life, lens, n = want[i // M]
        assert x["episodes"] == n and E.same(np.float64(x["avg_ep_lifetime"]), np.float64(life)) and \
            E.same(np.float64(x["avg_ep_lens"]), np.float64(lens)), (i, x, want)
    return env


def test_emulated_trainer_logs_episodes():
    """B = 16, N = 33, M = 3, batch 32, minibatch 16, two epochs; networks that live for 1e9 s at most, so that every episode ends by death."""
    import torch
    torch.set_num_threads(2)
    env = trainer_logs_episodes(lambda: emu_env(16, max_time=1e9, auto_reset=True), dict(batch_size=32, minibatch_size=16, n_updates_per_iteration=2), 200)
    env.side.close()
