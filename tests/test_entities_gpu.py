"""Entity observations on a real MI355X: the bodies of tests/test_entities.py on the device -- the values against the float64 formula
sheet on the reference fixtures and a ragged batch, every launch mode and the record / pool calls against the standalone wrsn_entities,
the extent of what a call writes -- and, device only, the two-stage pipeline and the VecWRSN surface.  Helpers and tolerances:
tests/entity_ref.py."""
import numpy as np
import pytest

import test_entities as body
from entity_ref import check_rows, peeks, reference
from sides import VecSide, load_fixture, need_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", body.FIXTURES)
def test_values_on_fixtures(name):
    body.values_on_fixtures(VecSide, name)


def test_blocking_steps_and_a_masked_reset():
    body.blocking_steps_and_a_masked_reset(VecSide)


def test_step_budget():
    body.step_budget(VecSide)


def test_time_sliced_launches():
    body.time_sliced_launches(VecSide)


def test_pipeline_at_its_smallest_size():
    """B = 512 environments of hanoi1000n50, budget 1250 and the image requested: the step call is the two-stage pipeline, the entity
    launches ride on both of its streams."""
    z, sc, mc = load_fixture("hanoi1000n50_m3_s1")
    B = 512
    side = VecSide([sc] * B, mc, 3, auto_reset=True, step_budget=1250)
    assert side.env.state is not None
    buf = body._registered(side)
    side.reset()
    rng = np.random.RandomState(5)
    kinds = set()
    for c in range(6):
        rows = side.rows()
        ids = np.array([-1 if r[4] == 4 else r[0] for r in rows], dtype=np.int32)
        touched = [e for e in range(B) if not (c % 2 == 1 and e % 7 == 3)]     # every seventh row is left alone in every other call
        ids[[e for e in range(B) if e not in set(touched)]] = -2
        buf.fill()
        side.step(ids, rng.rand(B, 3))
        rendered = body._rendered(side.rows(), touched)
        kinds |= {"rendered"} if rendered else set()
        kinds |= {"unrendered"} if len(rendered) < B else set()
        snap = body._check_call(side, buf, rendered, "pipeline call %d" % c)
    assert kinds == {"rendered", "unrendered"}, kinds
    pk = peeks(side.handle); agents = body._agents(side)
    for e in sorted(rendered)[:4]:
        check_rows(buf.rows(snap, e), reference(pk, e, int(agents[e]), sc, mc, side.N, 3), sc.n_node, "pipeline row %d" % e)
    side.close()


def test_load_clone_and_pool_reset():
    body.load_clone_and_pool_reset(VecSide)


def test_ragged_batch():
    body.ragged_batch_values_and_zero_rows(VecSide)


def test_unregistered_handle_writes_nothing_and_requests_are_identical():
    body.unregistering_and_identical_requests(VecSide)


@pytest.mark.parametrize("render", [False, True])
def test_vecwrsn_entities(render):
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import ENT_ENV, ENT_ENV_F, ENT_MC, ENT_MC_F, ENT_NODE, ENT_NODE_F, VecWRSN
    scs, mc = body._batch()
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
