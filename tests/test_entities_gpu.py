"""Entity observations on a real MI355X: the values against the float64 formula sheet on the reference fixtures and a ragged batch,
every launch mode (the two-stage pipeline included) and the record / pool calls against the standalone wrsn_entities, the extent of
what a call writes, and the VecWRSN surface.  Helpers and tolerances: tests/entity_ref.py."""
import numpy as np
import pytest

from entity_ref import EntBuf, check_extent, check_rows, peeks, reference

pytestmark = pytest.mark.gpu

FIELDS = ("agent_id", "reward", "terminal", "now", "status")
FIXTURES = ("six_m3_zero_length", "hanoi1000n50_m3_s1", "hanoi1000n50_m1_s3", "hanoi1000n50_m3_cap1500_mcdeath", "redundant_m2_deaths",
            "synth300_m3_s27")


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _env(scs, mc, M, **kw):
    """A VecWRSN with guarded, pattern-filled entity buffers registered on its handle."""
    from multi_agent_rl_wrsn_amd import VecWRSN
    env = VecWRSN(scs, mc, M, **kw)
    buf = EntBuf(env.num_env, env.n_node, M, device=env.device)
    env._h.set_entity_out(*buf.ptrs())
    return env, buf


def _host(env):
    env.synchronize()
    return {k: getattr(env, k).cpu().numpy() for k in FIELDS}


def _check_call(env, buf, rendered, agent_id, tag):
    """Extent of what the call wrote, and bit-equality of the rendered rows with wrsn_entities called right after."""
    torch = _torch()
    env.synchronize()
    snap = buf.snap()
    check_extent(buf, snap, rendered, tag)
    agents = np.array([int(agent_id[e]) if e in rendered else -1 for e in range(env.num_env)], dtype=np.int32)
    sbuf = EntBuf(env.num_env, env.n_node, env.num_agent, device=env.device)
    a = torch.as_tensor(agents, device=env.device)
    env._h.entities(a.data_ptr(), *sbuf.ptrs())
    env.synchronize()
    ssnap = sbuf.snap()
    check_extent(sbuf, ssnap, rendered, tag + " (standalone)")
    for k in snap:
        assert np.array_equal(snap[k], ssnap[k]), (tag, k, "rows differ from wrsn_entities")
    return snap


def _rendered(r, touched):
    return {e for e in touched if r["status"][e] != 4 and not r["terminal"][e] and r["agent_id"][e] >= 0}


@pytest.mark.parametrize("name", FIXTURES)
def test_values_on_fixtures(name):
    torch = _torch()
    from conftest import load_golden
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    z = load_golden(name)
    sc, mc = scenario_from_golden(z)
    M = int(z["num_agent"])
    env, buf = _env([sc], mc, M, map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]), render=False)
    env.reset()
    n = 0
    for k in range(-1, len(z["in_action"])):
        if k >= 0:
            buf.fill()
            env.step(torch.tensor([int(z["in_agent"][k])]), torch.tensor(z["in_action"][k][None]))
        r = _host(env)
        if (k >= 0 and z["is_none"][k]) or r["agent_id"][0] < 0:
            check_extent(buf, buf.snap(), set(), "%s decision %d renders nothing" % (name, k))
            break
        snap = _check_call(env, buf, {0}, r["agent_id"], "%s decision %d" % (name, k))
        a = int(r["agent_id"][0])
        check_rows(buf.rows(snap, 0), reference(peeks(env._h), 0, a, sc, mc, env.n_node, M), sc.n_node, "%s decision %d" % (name, k))
        n += 1
    assert n >= 2
    env.close()


def _batch():
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, DEFAULT_NODE_SPEC, synth_scenario
    weak = dict(DEFAULT_NODE_SPEC, capacity=1200.0)          # little above the threshold: the first node dies within a few steps
    scs = [synth_scenario(31 + e, 40, 30, node_spec=(weak if e == 2 else None)) for e in range(5)]
    return scs, DEFAULT_MC_SPEC


def _drive(env, buf, calls, need, tag):
    """Step calls with auto-reset until every kind of row in `need` occurred (at most `calls`); row 1 is left alone in every other call."""
    torch = _torch()
    rng = np.random.RandomState(11)
    seen = set()
    B = env.num_env
    for c in range(calls):
        r = _host(env)
        ids = r["agent_id"].copy()
        ids[r["status"] == 4] = -1
        skip = c % 2 == 1
        if skip:
            ids[1] = -2
        buf.fill()
        env.step(torch.tensor(ids), torch.tensor(rng.rand(B, 3)))
        r = _host(env)
        touched = [e for e in range(B) if not (skip and e == 1)]
        if skip:
            seen.add("-2")
        for e in touched:
            if r["status"][e] == 4:
                seen.add("status 4")
            elif r["terminal"][e]:
                seen.add("terminal")
        rendered = _rendered(r, touched)
        if rendered:
            seen.add("rendered")
        _check_call(env, buf, rendered, r["agent_id"], "%s call %d" % (tag, c))
        if need <= seen and c >= 8:
            break
    assert need <= seen, (tag, seen)


def test_blocking_steps_and_a_masked_reset():
    torch = _torch()
    scs, mc = _batch()
    env, buf = _env(scs, mc, 2, map_size=16, auto_reset=True)
    env.reset(torch.tensor([1, 0, 1, 1, 0]))
    _check_call(env, buf, {0, 2, 3}, _host(env)["agent_id"], "masked reset")
    buf.fill()
    env.reset()
    r = _host(env)
    snap = _check_call(env, buf, set(range(5)), r["agent_id"], "reset")
    pk = peeks(env._h)
    for e in range(5):
        check_rows(buf.rows(snap, e), reference(pk, e, int(r["agent_id"][e]), scs[e], mc, env.n_node, 2), scs[e].n_node, "reset row %d" % e)
    _drive(env, buf, 40, {"-2", "terminal", "rendered"}, "blocking")
    env.close()


def test_step_budget():
    scs, mc = _batch()
    env, buf = _env(scs, mc, 2, render=False, auto_reset=True, step_budget=40)
    env.reset()
    _drive(env, buf, 60, {"-2", "status 4", "rendered"}, "budget 40")
    env.close()


def test_time_sliced_launches():
    from multi_agent_rl_wrsn_amd import synth_scenario
    scs = [synth_scenario(500 + e, 200, 200) for e in range(8)]
    env, buf = _env(scs, None, 3, render=False, auto_reset=True, step_deadline_us=50)
    env.reset()
    _drive(env, buf, 300, {"-2", "status 4", "rendered"}, "time slices")
    env.close()


def test_pipeline_at_its_smallest_size():
    """B = 512 environments of hanoi1000n50, budget 1250 and the image requested: the step call is the two-stage pipeline, the entity
    launches ride on both of its streams."""
    torch = _torch()
    from conftest import load_golden
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    sc, mc = scenario_from_golden(load_golden("hanoi1000n50_m3_s1"))
    B = 512
    env, buf = _env([sc] * B, mc, 3, auto_reset=True, step_budget=1250)
    assert env.state is not None
    env.reset()
    rng = np.random.RandomState(5)
    kinds = set()
    for c in range(6):
        r = _host(env)
        ids = r["agent_id"].copy(); ids[r["status"] == 4] = -1
        touched = [e for e in range(B) if not (c % 2 == 1 and e % 7 == 3)]     # every seventh row is left alone in every other call
        ids[[e for e in range(B) if e not in set(touched)]] = -2
        buf.fill()
        env.step(torch.tensor(ids), torch.tensor(rng.rand(B, 3)))
        r = _host(env)
        rendered = _rendered(r, touched)
        kinds |= {"rendered"} if rendered else set()
        kinds |= {"unrendered"} if len(rendered) < B else set()
        snap = _check_call(env, buf, rendered, r["agent_id"], "pipeline call %d" % c)
    assert kinds == {"rendered", "unrendered"}, kinds
    pk = peeks(env._h)
    for e in sorted(rendered)[:4]:
        check_rows(buf.rows(snap, e), reference(pk, e, int(r["agent_id"][e]), sc, mc, env.n_node, 3), sc.n_node, "pipeline row %d" % e)
    env.close()


def test_load_clone_and_pool_reset():
    torch = _torch()
    scs, mc = _batch()
    env, buf = _env(scs, mc, 2, render=False)
    env.reset()
    rng = np.random.RandomState(4)
    for _ in range(3):
        env.step(torch.where(env.agent_id >= 0, env.agent_id, torch.full_like(env.agent_id, -2)), torch.tensor(rng.rand(5, 3)))   # a finished row is left alone
    r = _host(env)
    assert (r["agent_id"][[0, 3]] >= 0).all()
    rec = env.save_envs([0, 3])
    buf.fill()
    env.load_envs(rec, [1, 4])
    r = _host(env)
    snap = _check_call(env, buf, {1, 4}, r["agent_id"], "load")
    pk = peeks(env._h)
    for dst, src in ((1, 0), (4, 3)):
        check_rows(buf.rows(snap, dst), reference(pk, dst, int(r["agent_id"][dst]), scs[src], mc, env.n_node, 2), scs[src].n_node, "loaded row %d" % dst)
    buf.fill()
    env.clone_envs([0], [2])
    _check_call(env, buf, {2}, _host(env)["agent_id"], "clone")
    env.set_pool(rec, 5)
    buf.fill()
    env.pool_reset(torch.tensor([0, 1, 0, 1, 0]), torch.tensor([9, 1, 9, 0, 9]))
    _check_call(env, buf, {1, 3}, _host(env)["agent_id"], "pool reset")
    env.close()


def test_ragged_batch():
    torch = _torch()
    from conftest import load_golden
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    six, _ = scenario_from_golden(load_golden("six_m3_zero_length"))
    hanoi, mc = scenario_from_golden(load_golden("hanoi1000n50_m3_s1"))
    scs = [six, hanoi]
    env, buf = _env(scs, mc, 3, render=False)
    assert env.n_node == 82
    env.reset()
    rng = np.random.RandomState(2)
    checked = 0
    for c in range(4):
        r = _host(env)
        snap = buf.snap(); pk = peeks(env._h)
        for e in range(2):
            if r["agent_id"][e] < 0:
                continue
            rows = buf.rows(snap, e)
            check_rows(rows, reference(pk, e, int(r["agent_id"][e]), scs[e], mc, 82, 3), scs[e].n_node, "ragged call %d row %d" % (c, e))
            assert not rows[0][scs[e].n_node:].any()
            checked += 1
        ids = np.where(r["agent_id"] >= 0, r["agent_id"], -2).astype(np.int32)
        env.step(torch.tensor(ids), torch.tensor(rng.rand(2, 3)))
    assert checked >= 6
    env.close()


def test_unregistered_handle_writes_nothing_and_requests_are_identical():
    torch = _torch()
    from multi_agent_rl_wrsn_amd import VecWRSN
    scs, mc = _batch()
    env, buf = _env(scs, mc, 2, render=False, auto_reset=True)
    plain = VecWRSN(scs, mc, 2, render=False, auto_reset=True)
    rng = np.random.RandomState(8)
    for c in range(10):
        act = torch.tensor(rng.rand(5, 3))
        for v in (env, plain):
            if c == 0:
                v.reset()
            else:
                v.step(v.agent_id.clone(), act)
        for k in FIELDS:
            assert torch.equal(getattr(env, k), getattr(plain, k)), (c, k)
    env.synchronize()
    snap = buf.snap()
    assert any(buf.full(snap, e) for e in range(5))
    env._h.set_entity_out()
    buf.fill()
    env.reset()
    env.step(env.agent_id.clone(), torch.tensor(rng.rand(5, 3)))
    env.clone_envs([0], [1])
    env.synchronize()
    check_extent(buf, buf.snap(), set(), "unregistered")
    env.close(); plain.close()


@pytest.mark.parametrize("render", [False, True])
def test_vecwrsn_entities(render):
    torch = _torch()
    from multi_agent_rl_wrsn_amd import ENT_ENV, ENT_ENV_F, ENT_MC, ENT_MC_F, ENT_NODE, ENT_NODE_F, VecWRSN
    scs, mc = _batch()
    env = VecWRSN(scs, mc, 2, map_size=16, render=render, entities=True)
    r = env.reset()
    assert (r["state"] is None) == (not render)
    assert tuple(r["nodes"].shape) == (5, 40, ENT_NODE_F) and tuple(r["chargers"].shape) == (5, 2, ENT_MC_F) and tuple(r["env_feat"].shape) == (5, ENT_ENV_F)
    assert all(r[k].dtype == torch.float32 for k in ("nodes", "chargers", "env_feat"))
    rng = np.random.RandomState(1)
    for c in range(4):
        live_in = (r["agent_id"] >= 0) & (r["terminal"] == 0)
        r = env.step(torch.where(live_in, r["agent_id"], torch.full_like(r["agent_id"], -2)), torch.tensor(rng.rand(5, 3)))
        ids = torch.where(r["terminal"] != 0, torch.full_like(r["agent_id"], -1), r["agent_id"])
        live = torch.nonzero(ids >= 0).flatten()
        assert len(live) >= 3
        got = env.entity_state(ids)
        for k in ("nodes", "chargers", "env_feat"):
            assert torch.equal(got[k][live], r[k][live]), (c, k)
        assert torch.equal(r["env_feat"][live, ENT_ENV["agent"]], ids[live].float())
        assert torch.equal(r["chargers"][live, ids[live].long(), ENT_MC["is_self"]], torch.ones(len(live), device=env.device))
        assert (r["nodes"][live][:, :, ENT_NODE["alive"]].sum(1) > 0).all()
    with pytest.raises(ValueError):
        env.entity_state(ids, out={"nodes": got["nodes"][:, :, :4], "chargers": got["chargers"], "env_feat": got["env_feat"]})
    plain = VecWRSN(scs, mc, 2, map_size=16, render=False)   # entity_state without entities=True
    r0 = plain.reset()
    assert "nodes" not in r0
    e0 = plain.entity_state(r0["agent_id"])
    assert float(e0["env_feat"][0, ENT_ENV["n_node"]]) == 40.0
    env.close(); plain.close()
