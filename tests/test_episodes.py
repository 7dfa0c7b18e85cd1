"""The episode ledger (wrsn_episodes_collect; csrc/wrsn_rollout.h) on the emulated library.

The bodies take the side (tests/sides.py): this module runs them on EmuSide, tests/test_episodes_gpu.py on VecSide.  The reference is the
host loop of tests/episode_ref.py (`HostLedger`) over the request rows of the same side, with the same float64 adds in the same order:
every field of the log and both vectors of every call are compared bit for bit, so there is no tolerance.  B = 6 environments of 33
nodes: under a random action script such a network dies after 6 100 to 10 200 simulated seconds, within some twenty launches, and the
time limit lies between those lifetimes, so that some episodes end by network death (ended 1) and some by the limit (ended 2)."""
import numpy as np
import pytest
from sides import EmuSide

import entity_act_ref as R
import episode_ref as E

WRSN_ERR_ARG = -1
B0 = 6
TIME_LIMIT = 6300.0                                           # the ledger's time limit [s]
SHORT_LIMIT = 1500.0                                          # reached by every network within a few launches (extent, bad arguments)


def scenarios(B=B0, seed=500, mixed=True):
    """max_time alternates between the time limit and ten times it (mixed=False: ten times it everywhere)."""
    from multi_agent_rl_wrsn_amd import synth_scenario
    return [synth_scenario(seed + e, 33, 30, max_time=(TIME_LIMIT if mixed and e % 2 else 10 * TIME_LIMIT)) for e in range(B)]


def make_side(Side, M, B=B0, mixed=True, **kw):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    return Side(scenarios(B, mixed=mixed), DEFAULT_MC_SPEC, M, map_size=12, render=False, entities=True, **kw)


# ------------------------------------------------------------------------------------------------------------ 1. / 2. against a host loop
def loop_matches_host(Side, M, step_budget=0, need_both=True):
    """The evaluation loop under a fixed action script, two episodes per environment with parking: every call's log and vectors equal
    the host loop's; both ways of ending occur; with a step budget rows in flight occur; parked rows stay parked."""
    side = make_side(Side, M, step_budget=step_budget)
    loop = E.Loop(side, 2, 2, TIME_LIMIT)
    got = loop.run(lambda g: (g["finished"] >= 2).all())
    assert (got["finished"] == 2).all() and (got["dropped"] == 0).all() and (got["next"] == -2).all()
    codes = set(got["ended"].reshape(-1).tolist())
    assert codes <= {1, 2} and (not need_both or codes == {1, 2}), codes
    assert (got["lifetime"][got["ended"] == 2] >= TIME_LIMIT).all() and (got["lifetime"][got["ended"] == 1] > 0).all()
    assert (got["decisions"].sum(-1) > 0).all() and np.isfinite(got["ep_return"]).all() and (got["record"] == -1).all()
    assert {1, 2, 4} <= loop.seen_states and (not step_budget or 3 in loop.seen_states), loop.seen_states
    side.close()


@pytest.mark.parametrize("M,step_budget", [(3, 0), (3, 1250), (1, 0), (8, 0)])
def test_emulated_ledger_against_host_loop(M, step_budget):
    loop_matches_host(EmuSide, M, step_budget, need_both=(M == 3))


# ------------------------------------------------------------------------------------------------------------ 3. quota and parking
def parked_rows_are_left_alone(Side):
    """E = 2, quota = 2: once an environment is parked it gets -2 at every call and restart 0, and its record does not change any more
    while the others run on.  E = 1, quota = 0: nothing parks, later episodes are counted in `dropped` and not stored."""
    side = make_side(Side, 3)
    loop = E.Loop(side, 2, 2, TIME_LIMIT)
    got = loop.run(lambda g: (g["finished"] >= 2).any())
    first = int(np.argmax(got["finished"] >= 2))
    before = side.save_envs([first])
    before = before.copy() if isinstance(before, np.ndarray) else before.clone()
    n0 = len(loop.calls)
    for _ in range(6):
        got = loop.launch()
    for g in loop.calls[n0:]:
        assert g["next"][first] == -2 and g["restart"][first] == 0 and g["finished"][first] == 2
    after = side.save_envs([first])
    R.sync(side)
    assert E.same(np.asarray(before.cpu() if hasattr(before, "cpu") else before), np.asarray(after.cpu() if hasattr(after, "cpu") else after))
    side.close()
    side = make_side(Side, 3)
    loop = E.Loop(side, 1, 0, TIME_LIMIT)
    got = loop.run(lambda g: (g["finished"] >= 2).all())
    assert (got["dropped"] == got["finished"] - 1).all() and (got["dropped"] >= 1).all()
    first_life = loop.calls[[i for i, g in enumerate(loop.calls) if (g["finished"] >= 1).all()][0]]["lifetime"]
    assert E.same(got["lifetime"], first_life)                 # episode 0 of every row is what stays stored
    side.close()


def test_emulated_ledger_quota_and_parking():
    parked_rows_are_left_alone(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 4. consume
def consume_leaves_the_requests(Side):
    """An auto-reset roll-out with the ledger (consume = 0) in front of wrsn_rollout_collect_entities: the ledger equals the host loop,
    the transition buffers equal the mirror of tests/test_entity_rollout.py -- a run that knows of no ledger --, and a second, consuming
    ledger call after the same launch books nothing, as does a second collect."""
    import test_entity_rollout as TR
    side = make_side(Side, 3, mixed=False, auto_reset=True)       # no time limit here: every network must die
    B, M = side.B, side.M
    buf = TR.TrBuf(side, 256, TR.row_elems(side.N, M))
    led, host, states = E.Ledger(side, 4, 0), E.HostLedger(B, M, 4, 0), E.RowStates(B)
    mirror, done = TR.Mirror(side), [0] * B
    side.reset(); states.after_reset()
    led.collect(0.0, consume=False); host.collect(states, side._host(), consume=False)
    booked = ("run_return", "run_decisions", "finished", "dropped", "lifetime", "ep_return", "decisions", "ended", "record", "next")
    for call in range(60):
        ids, act, lp = TR.policy_ids(side, done)
        TR.record(side, buf.c(), ids, act, lp); mirror.record(ids, act, lp)
        side.step(ids, act.astype(np.float64)); states.after_step(ids, side._host())
        led.collect(0.0, consume=False); host.collect(states, side._host(), consume=False)
        E.assert_same(led.get(), host.get(), ("consume=0", call))
        TR.collect(side, buf.c()); mirror.collect(range(B))
        before, counts = led.get(), buf.arrays()["count"].copy()
        led.collect(0.0, consume=True)                         # the requests are consumed: nothing is booked twice
        E.assert_same(led.get(), before, ("second call", call), keys=booked)
        TR.collect(side, buf.c())
        assert np.array_equal(buf.arrays()["count"], counts), call
        if (before["finished"] >= 1).all() and call >= 20:
            break
    assert (led.get()["finished"] >= 1).all() and (led.get()["ended"][0] == 1).all()
    TR.assert_equals_mirror(buf, mirror, "with the ledger in front")
    side.close()


def test_emulated_ledger_consume():
    consume_leaves_the_requests(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 5. pools
def pool_records_are_logged(Side):
    """Restart by wrsn_pool_reset(mask = restart) with a stated record per row: `record` holds what pool_info() says at the time of
    closing -- -1 for the first episode (the environment's own scenario), the stated record for the second."""
    side = make_side(Side, 3)
    side.reset()
    pool = side.save_envs()
    R.sync(side)
    side.set_pool(pool, seed=7)
    index = lambda t: ((np.arange(B0) + 1 + t) % B0).astype(np.int32)
    loop = E.Loop(side, 2, 2, TIME_LIMIT, pool_index=index)
    got = loop.run(lambda g: (g["finished"] >= 2).all())
    assert (got["record"][0] == -1).all() and ((got["record"][1] >= 0) & (got["record"][1] < B0)).all()
    assert len(set(got["record"][1].tolist())) > 1
    side.close()


def test_emulated_ledger_pools():
    pool_records_are_logged(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 6. extent, 7. bad arguments
def extent_and_null_pointers(Side):
    """Guard bytes around every array hold (checked at every call of every loop above as well); with next_agent_id, restart and record
    NULL the other arrays get the bytes of a run that passed them, and the three buffers are not touched."""
    sides = [make_side(Side, 3) for _ in range(2)]
    full, bare = E.Ledger(sides[0], 2, 2), E.Ledger(sides[1], 2, 2)
    rng = np.random.default_rng(1)
    for s in sides:
        s.reset()
    full.collect(SHORT_LIMIT); bare.collect(SHORT_LIMIT, next=0, restart=0, record=0)
    for _ in range(12):
        act = rng.random((B0, 3))
        ids = full.next.get()
        for s in sides:
            s.step(ids, act)
        full.collect(SHORT_LIMIT); bare.collect(SHORT_LIMIT, next=0, restart=0, record=0)
        mask = full.restart.get()
        for s in sides:
            s.reset(mask=mask)
        full.collect(SHORT_LIMIT); bare.collect(SHORT_LIMIT, next=0, restart=0, record=0)
    a, b = full.get(), bare.get()
    assert a["finished"].sum() > 0
    E.assert_same(b, a, "NULL vectors", keys=[k for k in E.log_shapes(1, 1, 1) if k != "record"])
    assert bare.next.untouched() is False and (bare.next.get() == E.NEXT_FILL).all() and (bare.restart.get() == E.RESTART_FILL).all()
    assert (b["record"] == 0).all() and full.guards_intact() and bare.guards_intact()
    for s in sides:
        s.close()


def test_emulated_ledger_extent_and_null_pointers():
    extent_and_null_pointers(EmuSide)


def bad_arguments(Side):
    """Every WRSN_ERR_ARG case leaves every buffer (and the row states) untouched: the valid call that follows gives the bytes of a run
    that never saw the bad call."""
    from multi_agent_rl_wrsn_amd._lib import WrsnError
    sides = [make_side(Side, 3) for _ in range(2)]
    clean, led = E.Ledger(sides[0], 2, 1), E.Ledger(sides[1], 2, 1)
    for s in sides:
        s.reset()
    req = E.req_ptrs(sides[1])
    cases = [dict(log=None), dict(episodes=0), dict(quota=-1), dict(quota=3), dict(next=req["agent_id"])]
    cases += [dict(**{k: 0}) for k in E.log_shapes(1, 1, 1) if k != "record"]
    cases += [dict(req={k: 0}) for k in ("agent_id", "reward", "now", "status")]
    rng = np.random.default_rng(2)
    for i, over in enumerate(cases):
        before = led.snap()
        with pytest.raises(WrsnError) as ei:
            led.collect(SHORT_LIMIT, **over)
        assert ei.value.code == WRSN_ERR_ARG, over
        R.sync(sides[1])
        assert all(np.array_equal(x, y) for x, y in zip(before, led.snap())), over
        clean.collect(SHORT_LIMIT); led.collect(SHORT_LIMIT)
        E.assert_same(led.get(), clean.get(), over)
        act, ids = rng.random((B0, 3)), clean.next.get()
        for s in sides:
            s.step(ids, act)
        if i % 4 == 3:                                         # now and then a second bad call right after a launch
            with pytest.raises(WrsnError):
                led.collect(SHORT_LIMIT, episodes=0)
        clean.collect(SHORT_LIMIT); led.collect(SHORT_LIMIT)
        E.assert_same(led.get(), clean.get(), (over, "step"))
        mask = clean.restart.get()
        for s in sides:
            s.reset(mask=mask)
    assert clean.get()["finished"].sum() > 0
    lib = sides[0].handle.lib
    assert lib.wrsn_episodes_collect(None, None, None, 0.0, None, None, 1) == WRSN_ERR_ARG
    for s in sides:
        s.close()


def test_emulated_ledger_bad_arguments():
    bad_arguments(EmuSide)
