"""Acting from entity rows on the device: the bodies of tests/test_entity_act.py on VecSide, and the fused trainer end to end."""
import numpy as np
import pytest
from sides import VecSide, need_gpu

import test_entity_act as body

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [70, 33, 257])
def test_entity_act_synthetic_rows(N):
    body.synthetic_rows_match(VecSide, N)


def test_entity_act_masks():
    body.masks_are_selects(VecSide)


def test_entity_act_independence():
    body.rows_are_independent(VecSide)


def test_entity_act_extent():
    body.extent_is_respected(VecSide)


def test_entity_act_bad_arguments():
    body.bad_arguments_leave_everything_untouched(VecSide)


def test_entity_actor_layout():
    need_gpu()
    from multi_agent_rl_wrsn_amd import _lib
    body.layout_matches_the_header(_lib.load())


def test_entity_act_on_simulator_rows():
    body.acts_on_the_simulators_rows(VecSide)


def test_fused_entity_trainer_end_to_end():
    """9: B = 64, N = 70, M = 3.  BatchedEntityIPPO(fused_policy=True) rolls out and updates; on the first minibatch of the first update
    |log-ratio| <= 1e-3 (the device bound of the unfused trainer's test), clipfrac is 0 and the actor gradient is non-zero."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, VecWRSN, synth_scenario
    torch.manual_seed(0); np.random.seed(0)
    M = 3
    env = VecWRSN([synth_scenario(300 + e, 70, 60) for e in range(64)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
    algo = BatchedEntityIPPO(dict(batch_size=32, minibatch_size=16, n_updates_per_iteration=2), env, fused_policy=True)
    with torch.no_grad():                                      # a policy that is not the 0.01 head: sigma and mean depend on the rows
        for a in algo.actors:
            a.mean.weight.mul_(30.0); a.log_std.weight.mul_(30.0)
    batches = algo.roll_out(max_launches=100)
    assert algo._packed is not None
    for a in range(M):
        batch = batches[a]
        mb = torch.arange(16, device=env.device)
        with torch.no_grad():
            new, _ = algo.evaluate(a, batch["states"][mb], batch["actions"][mb])
        d = float((new - batch["log_probs"][mb]).abs().max())
        loss, pg, vl, en, kl, clipfrac = algo.minibatch_loss(a, batch, mb)
        print("charger %d: first minibatch |log-ratio| %.3g, clipfrac %g, approx_kl %.3g" % (a, d, clipfrac, float(kl)))
        assert d <= 1e-3, (a, d)
        assert clipfrac == 0.0
        algo.optimizers[a].zero_grad(); loss.backward()
        gn = torch.sqrt(sum((p.grad ** 2).sum() for p in algo.actors[a].parameters() if p.grad is not None))
        assert float(gn) > 0 and bool(torch.isfinite(gn))
        algo.optimizers[a].zero_grad()
    for a in range(M):
        st = algo.update(a, batches[a])
        assert all(np.isfinite(v) for v in st), st
    assert algo._packed is None
    p = algo.packed_actors()
    algo.roll_out(max_launches=100)                           # packs the updated weights again
    assert torch.equal(algo._packed, p)
    env.close()
