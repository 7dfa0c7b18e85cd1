"""Entity transition rows on the device: the bodies of tests/test_entity_rollout.py on VecSide, racing slot claims over 512
environments, and the entity trainer end to end."""
import numpy as np
import pytest
from sides import VecSide, load_fixture, need_gpu

import test_entity_rollout as body

pytestmark = pytest.mark.gpu


def test_entity_transition_buffers_equal_the_reference_bookkeeping():
    body.bookkeeping_equals_the_reference_lists(VecSide)


def test_ragged_entity_rows():
    body.ragged_rows_arrive_whole(VecSide)


def test_large_entity_rows():
    body.large_rows_arrive_whole(VecSide)


def test_entity_rows_extent():
    body.extent_is_respected(VecSide)


def test_entity_collect_consume():
    body.consume_feeds_both_kinds_of_buffers(VecSide)


def test_entity_rollout_bad_arguments():
    body.bad_arguments_leave_everything_untouched(VecSide)


def _race_run(scs, mc, M, capacity, calls=8):
    """`calls` step calls of a fixed-seed random policy over the batch; returns the host arrays of the filled buffers."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import EntityTransitionBuffers, VecWRSN
    env = VecWRSN(scs, mc, M, render=False, entities=True, auto_reset=True, step_budget=1250)
    buf = EntityTransitionBuffers(env, capacity)
    g = torch.Generator(device="cpu").manual_seed(17)
    r = env.reset()
    for _ in range(calls):
        ids = r["agent_id"].clone()
        act = torch.rand((env.num_env, 3), generator=g).to(env.device)
        lp = -torch.rand((env.num_env,), generator=g).to(env.device)
        buf.record(ids, act, lp)
        r = env.step(ids, act.double())
        buf.collect()
    env.synchronize()
    assert env.state is None and int((r["status"] < 0).sum()) == 0
    out = {k: getattr(buf, k).cpu().numpy() for k in ("state", "next_state", "action", "reward", "logp", "now", "env_index", "count")}
    env.close()
    return out


def test_racing_slot_claims_fill_exactly_the_capacity_with_whole_transitions():
    """6: 512 copies of one network return the same charger in the same call, so up to 512 waves claim slots of one counter at once.
    With capacity 64 the count equals that of a run whose capacity holds everything, exactly 64 slots per charger are filled, their
    (env, now) keys are distinct, and each stored transition is bit for bit the large run's transition with that key."""
    z, sc, mc = load_fixture("hanoi1000n50_m3_s1")
    M, B = 3, 512
    scs = [sc] * B
    big = _race_run(scs, mc, M, 8 * B)
    small = _race_run(scs, mc, M, 64)
    assert np.array_equal(big["count"], small["count"]) and (big["count"] > 64).all() and (big["count"] <= 8 * B).all()
    for a in range(M):
        n = int(big["count"][a])
        ref = {(int(big["env_index"][a, q]), float(big["now"][a, q]), float(big["logp"][a, q])): q for q in range(n)}
        assert len(ref) == n                                   # the log-probability (a fresh random number per decision) settles a tie
        keys = [(int(small["env_index"][a, q]), float(small["now"][a, q])) for q in range(64)]
        assert len(set(keys)) == 64 and all(0 <= k[0] < B for k in keys)
        for q, k in enumerate(keys):
            p = ref[k + (float(small["logp"][a, q]),)]
            for name in ("state", "next_state", "action", "reward", "logp"):
                assert np.array_equal(small[name][a, q].view(np.uint32), big[name][a, p].view(np.uint32)), (a, q, name)


def test_entity_trainer_end_to_end():
    """10: 64 small environments without an image, one training iteration of BatchedEntityIPPO; every stored transition of charger a
    names a as its asking charger in state and next_state; evaluate reproduces the stored log-probabilities before the first
    optimiser step."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import (ENT_ENV, ENT_MC, BatchedEntityIPPO, EntityTransitionBuffers, VecWRSN, synth_scenario)
    torch.manual_seed(0); np.random.seed(0)
    M = 2
    env = VecWRSN([synth_scenario(500 + e, 40, 30) for e in range(64)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
    algo = BatchedEntityIPPO(dict(batch_size=32, minibatch_size=16, n_updates_per_iteration=2), env)
    assert env.state is None
    # the roll-out of the first iteration, checked before any optimiser step
    algo.buffers.clear(); algo._req = env.reset()
    for _ in range(200):
        algo.step_batch()
        assert env.state is None
        if min(algo.buffers.counts()) >= 32:
            break
    stored = algo.buffers.stored()
    assert min(stored) >= 32
    for a in range(M):
        n = stored[a]
        for name in ("state", "next_state"):
            nodes, mcs, envf = EntityTransitionBuffers.split(getattr(algo.buffers, name)[a, :n], M)
            assert bool((envf[:, ENT_ENV["agent"]] == a).all()) and bool((mcs[:, a, ENT_MC["is_self"]] == 1).all()), (a, name)
            assert bool((mcs[:, :, ENT_MC["is_self"]].sum(1) == 1).all())
        with torch.no_grad():
            new, _ = algo.evaluate(a, algo.buffers.state[a, :n], algo.buffers.action[a, :n])
        d = float((new - algo.buffers.logp[a, :n]).abs().max())
        print("charger %d: %d transitions, max |evaluate - stored logp| %.3g" % (a, n, d))
        assert d <= 1e-3, (a, d)
    rows = algo.train(0)                                       # goes on from the requests above: one roll-out, one update per charger
    assert len(rows) == M and sorted(r["agent"] for r in rows) == list(range(M))
    for r in rows:
        assert all(np.isfinite(r[k]) for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac")), r
    assert env.state is None
    env.close()
