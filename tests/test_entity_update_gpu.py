"""The PPO update of the entity policy on the device: the bodies of tests/test_entity_update.py on VecSide, and the fused-update trainer
end to end."""
import numpy as np
import pytest
from sides import VecSide, need_gpu

import test_entity_update as body

pytestmark = pytest.mark.gpu


def test_entity_critic_layout():
    need_gpu()
    from multi_agent_rl_wrsn_amd import _lib
    body.layout_matches_the_header(_lib.load())


@pytest.mark.parametrize("shape", body.FWD_CASES)
def test_entity_eval(shape):
    body.forward_matches(VecSide, shape)


@pytest.mark.parametrize("i", range(len(body.LOSS_HYPERS)))
def test_entity_ppo_loss(i):
    body.loss_matches(VecSide, i)


@pytest.mark.parametrize("shape", list(body.GRAD_CASES))
def test_entity_ppo_grad(shape):
    body.gradient_matches(VecSide, shape)


def test_entity_update_extent():
    body.extent_is_respected(VecSide)


def test_entity_update_bad_arguments():
    body.bad_arguments_leave_everything_untouched(VecSide)


def test_entity_adam():
    body.adam_matches(VecSide)


def test_fused_update_trainer_end_to_end():
    """B = 64, N = 70, M = 3, batch 32, minibatch 16, two epochs, fused_policy and fused_update.  The first minibatch's loss, pg, v_loss,
    entropy and approx_kl from the device table are within 1e-3 of minibatch_loss on the same weights and rows (the device bound of the
    unfused trainer's test), clipfrac is 0, the parameters changed and are finite, and a second roll_out packs the updated actors.  The
    relative L2 distance of the device gradient from torch's float32 autograd on that minibatch is printed, not asserted (kinks: see
    tests/entity_train_ref.py)."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, VecWRSN, pack_entity_actor, pack_entity_critic, synth_scenario
    import entity_train_ref as T
    torch.manual_seed(0); np.random.seed(0)
    M = 3
    env = VecWRSN([synth_scenario(300 + e, 70, 60) for e in range(64)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
    algo = BatchedEntityIPPO(dict(batch_size=32, minibatch_size=16, n_updates_per_iteration=2), env, fused_policy=True, fused_update=True)
    with torch.no_grad():
        for a in algo.actors:
            a.mean.weight.mul_(30.0); a.log_std.weight.mul_(30.0)
    batches = algo.roll_out(max_launches=100)
    for a in range(M):
        batch = batches[a]
        state = np.random.get_state()
        # the reference on the same weights and rows: the first minibatch of the shuffle the update is about to draw
        probe = np.arange(32); np.random.shuffle(probe); np.random.set_state(state)
        mb = torch.as_tensor(probe[:16], device=env.device, dtype=torch.long)
        loss, pg, vl, en, kl, clipfrac = algo.minibatch_loss(a, batch, mb)
        algo.optimizers[a].zero_grad(); loss.backward()
        ga_ref, gc_ref = T_block_grad(algo.actors[a]), T_block_grad(algo.critics[a])
        algo.optimizers[a].zero_grad()
        before = pack_entity_actor(algo.actors[a]).clone()
        # the device gradient of that minibatch, on the blocks as the update will pack them
        ba, bc = pack_entity_actor(algo.actors[a]).contiguous(), pack_entity_critic(algo.critics[a]).contiguous()
        g_dev = torch.zeros(T.P_ACTOR + T.P_CRITIC, dtype=torch.float32, device=env.device); st_dev = torch.zeros(8, dtype=torch.float32, device=env.device)
        f32 = lambda x: x.to(torch.float32).contiguous()
        b = {"actions": f32(batch["actions"]), "log_probs": f32(batch["log_probs"]), "advantages": f32(batch["advantages"]),
             "returns": f32(batch["returns"]), "values": f32(batch["values"])}
        hyper = dict(clip=algo.clip, ent_coef=algo.ent_coef, vf_coef=algo.vf_coef, norm_adv=algo.norm_adv, clip_vloss=algo.clip_vloss)
        env.entity_ppo_grad(ba, bc, f32(batch["states"]), mb.to(torch.int32), b, hyper, g_dev, st_dev)
        diff = torch.cat([g_dev[:ga_ref.numel()] - ga_ref, g_dev[T.P_ACTOR:T.P_ACTOR + gc_ref.numel()] - gc_ref])
        rel = float(diff.norm() / torch.cat([ga_ref, gc_ref]).norm())
        print("charger %d: relative L2 distance of the device gradient from float32 autograd on the first minibatch: %.3g" % (a, rel))
        st = algo.update(a, batch)
        assert all(np.isfinite(v) for v in st), st
        first = algo.first_minibatch_stats[a]
        want = (float(loss), float(pg), float(vl), float(en), float(kl))
        print("charger %d: first minibatch device %s, torch %s" % (a, first, want + (clipfrac,)))
        for k in range(5):
            assert abs(first[k] - want[k]) <= 1e-3, (a, k, first, want)
        assert first[5] == 0.0 and clipfrac == 0.0
        after = pack_entity_actor(algo.actors[a])
        assert not torch.equal(after, before) and bool(torch.isfinite(after).all())
        assert bool(torch.isfinite(pack_entity_critic(algo.critics[a])).all())
    assert algo._packed is None
    p = algo.packed_actors()
    algo.roll_out(max_launches=100)                           # packs the updated weights again
    assert torch.equal(algo._packed, p)
    env.close()


def T_block_grad(net):
    """The gradients of `net` in the layout of its packed block, without the padding (float32, on the net's device)."""
    import torch
    import entity_train_ref as T
    parts = []
    for _, lay in T.named_layers(net):
        parts += [lay.weight.grad.t().reshape(-1), lay.bias.grad.reshape(-1)]
    return torch.cat(parts)
