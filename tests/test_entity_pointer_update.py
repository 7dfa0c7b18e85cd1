"""The PPO gradient of the node-pointer policy (wrsn_entity_pointer_eval, wrsn_entity_pointer_ppo_grad; csrc/wrsn_entity_pointer_train.h)
and the trainer's device_update option, on the emulated library.

The bodies take the side (tests/sides.py): this module runs them on EmuSide, tests/test_entity_pointer_update_gpu.py on VecSide.  Memory,
nets, the reference (the module and PPOLearner.minibatch_loss in float64 on the CPU; bounds 4 * err32 + 1e-6, for a gradient tensor
4 * err32 + 1e-6 * max|g64|) and the kink margins that keep the gradient comparison honest are in tests/entity_pointer_train_ref.py."""
import numpy as np
import pytest
from sides import EmuSide

import entity_act_ref as R
import entity_pointer_ref as P
import entity_pointer_train_ref as Q
import test_entity_act as A

# (n, N, M) -> the first seed whose float64 kink margins clear 1.5 (8 * err32 + 2e-6) (Q.find_seed; the margins themselves are asserted again in every test)
GRAD_CASES = {(8, 70, 3): 2, (8, 33, 3): 1, (2, 257, 3): 3, (4, 33, 8): 0}
HYPERS = [Q.HYPER, dict(Q.HYPER, norm_adv=False, clip_vloss=False)]
_REFS = {}


def grad_case(shape, hyper=Q.HYPER):
    """(nets, rows, batch, Ref) of a case: computed once, shared by every test and both sides, never modified."""
    key = (shape, tuple(sorted(hyper.items())))
    if key not in _REFS:
        _REFS[key] = Q.case(GRAD_CASES[shape], *shape, hyper=hyper)
    return _REFS[key]


def side_for(Side, N, M, B=2, **kw):
    return A.make_side(Side, N, B, M, **kw)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ 1. eval against float64
def eval_matches(Side, shape):
    """logp, entropy, mean, log_std and value against float64 on a batch with: a row with no alive node (0), alive nodes but stored -1 (1),
    a stored node that is dead (2), stored NaN, -2 and N (3, 4, 5: as -1); through index = NULL and through an index with a repeat, whose
    rows keep their bytes (independence); two calls give equal bytes; guards intact; actor = NULL and critic = NULL."""
    n, N, M = shape
    # the actor of the acting tests: its log_std leaves [-4, 1] on both sides by itself and stays inside on most rows
    nets = (P.make_actors(M)[0], Q.make_nets(M)[1])
    rows = Q.make_rows(GRAD_CASES[shape], 8, N, M)
    stored = Q.make_stored(GRAD_CASES[shape], rows, nets[0], M)
    node, mc, env = _split(rows, N, M)
    node[0, :, 7] = 0.0                                       # row 0: no alive node
    alive = node[..., 7] == 1
    dead2 = np.flatnonzero(~alive[2])
    if dead2.size == 0:
        node[2, 0, 7] = 0.0; dead2 = np.array([0]); alive = node[..., 7] == 1
    assert alive[1].any() and alive[2].any()
    stored[0, 0] = -1.0; stored[1, 0] = -1.0; stored[2, 0] = float(dead2[0]); stored[3, 0] = np.nan; stored[4, 0] = -2.0; stored[5, 0] = float(N)
    rows = R.pack_rows(node, mc, env)
    ref = Q.Ref(nets[0], nets[1], rows, stored, None, Q.HYPER, M)
    side = side_for(Side, N, M, B=8)
    job = Q.Job(side, nets, rows, None, N, M, stored=stored)
    got = job.eval()
    first = [o.snap() for o in job.outs]
    assert all(np.isfinite(got[k]).all() for k in ("logp", "entropy", "mean", "log_std", "value"))
    ref.check_forward(got, "%s %s" % (side.name, shape))
    nl = np.where(ref.alive, got["node_logp"], 0.0)
    assert np.isneginf(got["node_logp"][~ref.alive]).all()
    dev = float(np.abs(nl - ref.f64["node_logp"]).max())
    assert dev <= 4.0 * ref.err32["node_logp"] + 1e-6, (dev, ref.err32["node_logp"])
    assert all(o.guards_intact() for o in job.outs)
    job.fill(); job.eval()
    assert all(np.array_equal(a, o.snap()) for a, o in zip(first, job.outs))
    idx = np.random.default_rng(n).permutation(8).astype(np.int32); idx[-1] = idx[0]
    goti = Q.Job(side, nets, rows, None, N, M, index=idx, stored=stored).eval()
    for k in got:
        assert same(goti[k], got[k][idx]), k
    job.fill(); only_c = job.eval(actor=False)
    assert all(job.fwd[k].untouched() for k in job.fwd if k != "value") and same(only_c["value"], got["value"])
    job.fill(); only_a = job.eval(critic=False)
    assert job.fwd["value"].untouched() and all(same(only_a[k], got[k]) for k in got if k != "value")
    side.close()


def _split(rows, N, M):
    n = rows.shape[0]
    return (rows[:, :8 * N].reshape(n, N, 8).copy(), rows[:, 8 * N:8 * N + 12 * M].reshape(n, M, 12).copy(), rows[:, 8 * N + 12 * M:].copy())


@pytest.mark.parametrize("shape", list(GRAD_CASES))
def test_emulated_pointer_eval(shape):
    eval_matches(EmuSide, shape)


# ------------------------------------------------------------------------------------------------------------ 2. eval against act, by bytes
def eval_reproduces_act(Side, shape=(8, 70, 3)):
    """wrsn_entity_pointer_act, sampled, on entity buffers; the same rows packed; eval with the act's `stored`: node_logp, charge_mean and
    charge_log_std have equal bytes, logp is within the bound of act's (act forms it from its own eps)."""
    n, N, M = shape
    ids = np.zeros(n, np.int32)
    node, mc, env = R.synth_rows(GRAD_CASES[shape], n, N, M, ids)
    node[1, :, 7] = 0.0                                       # a row with no alive node: stored -1
    side = side_for(Side, N, M, B=n)
    eps = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    act = P.Call(side, M, node, mc, env, ids, P.gumbel_noise(3, n, N), eps).run()
    assert act["node"][1] == -1 and (act["node"][[0, 2]] >= 0).all()
    nets = (P.make_actors(M)[0], Q.make_nets(M)[1])            # act's block 0
    rows = R.pack_rows(node, mc, env)
    got = Q.Job(side, nets, rows, None, N, M, stored=act["stored"]).eval()
    for k in ("node_logp", "charge_mean", "charge_log_std"):
        assert same(got[k], act[k]), k
    ref = Q.Ref(nets[0], nets[1], rows, act["stored"], None, Q.HYPER, M)
    dev = float(np.abs(got["logp"].astype(np.float64) - act["logp"]).max())
    print("%s logp: eval against act %.3g, err32 %.3g" % (side.name, dev, ref.err32["logp"]))
    assert dev <= 4.0 * ref.err32["logp"] + 1e-6
    side.close()


def test_emulated_pointer_eval_reproduces_act():
    eval_reproduces_act(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 3. / 4. gradients
def gradient_matches(Side, shape, hi=0):
    """Every tensor of both blocks and the eight statistics against float64 autograd, under the kink assertion; padding zero; s_raw beyond
    the clamp on some row, and such a row alone gives exactly zero gradient in the log_std column of `charge`; two calls give equal
    bytes; outputs sit between intact guards; inputs are left as they were."""
    n, N, M = shape
    hyper = HYPERS[hi]
    nets, rows, batch, ref = grad_case(shape, hyper)
    ref.assert_margins(str(shape))
    s_raw = ref.q64["s_raw"]
    out = np.flatnonzero((s_raw < -4) | (s_raw > 1))
    assert out.size and ((s_raw > -4) & (s_raw < 1)).any()
    if n >= 4:
        assert (s_raw < -4).any() and (s_raw > 1).any()
    side = side_for(Side, N, M)
    job = Q.Job(side, nets, rows, batch, N, M, hyper=hyper)
    before = [x.snap() for x in job.inputs]
    ga, gc, stats = job.grad()
    first = [o.snap() for o in (job.ga, job.gc, job.stats)]
    ref.check_stats(stats, "%s %s" % (side.name, shape))
    ref.check_grads(ga, gc, nets, "%s %s" % (side.name, shape))
    assert all(o.guards_intact() for o in job.outs) and all(np.array_equal(a, x.snap()) for a, x in zip(before, job.inputs))
    job.fill(); job.grad()
    assert all(np.array_equal(a, o.snap()) for a, o in zip(first, (job.ga, job.gc, job.stats)))
    if hi == 0:
        j1 = Q.Job(side, nets, rows, batch, N, M, index=[int(out[0])], hyper=dict(hyper, norm_adv=False))
        g1, _, _ = j1.grad()
        sl = Q.block_slices(nets[0])
        w = g1[sl["charge.w"]].reshape(136, 2)
        assert (w[:, 1] == 0).all() and g1[sl["charge.b"]][1] == 0 and np.abs(w[:, 0]).max() > 0
    side.close()


@pytest.mark.parametrize("hi", range(len(HYPERS)))
@pytest.mark.parametrize("shape", list(GRAD_CASES))
def test_emulated_pointer_ppo_grad(shape, hi):
    gradient_matches(EmuSide, shape, hi)


# ------------------------------------------------------------------------------------------------------------ 5. bad arguments
def bad_arguments_leave_everything_untouched(Side):
    """Every WRSN_ERR_ARG case leaves the pattern-filled outputs untouched; the valid call that follows gives the bytes of before."""
    from multi_agent_rl_wrsn_amd._lib import WrsnError
    shape = (8, 33, 3)
    n, N, M = shape
    nets, rows, batch, _ = grad_case(shape)
    side = side_for(Side, N, M)
    job = Q.Job(side, nets, rows, batch, N, M)
    want = job.grad()
    off_a = Q.Guarded(side, (Q.P_ACTOR,), data=Q.pack(nets[0]), shift=4)
    off_r = Q.Guarded(side, rows.shape, data=rows, shift=4)
    off_g = Q.Guarded(side, (Q.P_ACTOR,), shift=4)
    grad_bad = [dict(actor_ptr=0), dict(critic_ptr=0), dict(rows_ptr=0), dict(grad_actor=0), dict(grad_critic=0), dict(stats=0), dict(stored=0),
                dict(logp_old=0), dict(advantage=0), dict(ret=0), dict(value_old=0), dict(actor_ptr=off_a.ptr), dict(critic_ptr=job.critic.ptr + 4),
                dict(rows_ptr=off_r.ptr), dict(grad_actor=off_g.ptr), dict(grad_critic=job.gc.ptr + 4), dict(n=0), dict(n=1), dict(n_mc=0),
                dict(n_mc=9), dict(n_node=0)]
    actor_outs = dict(logp=0, entropy=0, node_logp=0, charge_mean=0, charge_log_std=0)
    eval_bad = [dict(actor_ptr=0, critic_ptr=0), dict(rows_ptr=0), dict(actor_outs), dict(value=0), dict(actor_ptr=0), dict(critic_ptr=0),
                dict(stored=0), dict(actor_ptr=off_a.ptr), dict(critic_ptr=job.critic.ptr + 4), dict(rows_ptr=off_r.ptr), dict(n=0), dict(n_mc=0),
                dict(n_mc=9), dict(n_node=0)]
    for kind, cases in (("grad", grad_bad), ("eval", eval_bad)):
        for over in cases:
            job.fill(); off_g.fill()
            with pytest.raises(WrsnError) as ei:
                (job.grad if kind == "grad" else job.eval)(**over)
            assert ei.value.code == -1, (kind, over)           # WRSN_ERR_ARG
            assert all(o.untouched() for o in job.outs) and off_g.untouched(), (kind, over)
    got = job.grad()
    assert all(same(x, y) for x, y in zip(got, want))
    side.close()


def test_emulated_pointer_update_bad_arguments():
    bad_arguments_leave_everything_untouched(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 6. Adam on the pointer block
def adam_matches(Side):
    """One wrsn_entity_adam step at n_floats = 56 980 on the kernel's own gradient, against float64 (tests/test_entity_update.py's three
    criteria): |delta - delta64| <= 1e-5 |delta64| + one float32 ulp of p; v to 1e-5 relative; m to 1e-5 relative plus one float32 ulp of
    its two terms; the norm against float64, above max_norm."""
    from test_entity_update import adam64
    shape = (8, 33, 3)
    n, N, M = shape
    nets, rows, batch, _ = grad_case(shape)
    side = side_for(Side, N, M)
    job = Q.Job(side, nets, rows, batch, N, M)
    job.grad()
    Pn = Q.P_ACTOR
    assert Pn % 256 != 0
    m, v, nrm = Q.Guarded(side, (Pn,), data=np.zeros(Pn)), Q.Guarded(side, (Pn,), data=np.zeros(Pn)), Q.Guarded(side, (1,))
    lr, eps, b1, b2 = 1e-3, 1e-8, float(np.float32(0.9)), float(np.float32(0.999))
    p0, g0 = job.actor.get().astype(np.float64), job.ga.get().astype(np.float64)
    max_norm = float(np.float32(0.5 * np.sqrt((g0 * g0).sum())))
    side.handle.entity_adam(job.actor.ptr, job.ga.ptr, m.ptr, v.ptr, Pn, 1, lr, b1, b2, eps, max_norm, nrm.ptr)
    R.sync(side)
    p64, m64, v64, norm = adam64(p0, g0, np.zeros(Pn), np.zeros(Pn), 1, lr, b1, b2, eps, max_norm)
    assert norm > max_norm and abs(float(nrm.get()[0]) - norm) <= 1e-6 * norm
    p1, m1, v1 = job.actor.get(), m.get().astype(np.float64), v.get().astype(np.float64)
    d, d64 = p1.astype(np.float64) - p0, p64 - p0
    ulp = np.spacing(np.abs(p0).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(d - d64) - (1e-5 * np.abs(d64) + ulp)).max())
    print("%s adam on the pointer block: largest excess over the bound %.3g, max|delta| %.3g" % (side.name, worst, np.abs(d64).max()))
    assert worst <= 0
    assert (np.abs(v1 - v64) <= 1e-5 * np.abs(v64)).all()
    gs = g0 * min(1.0, max_norm / (norm + 1e-6))
    assert (np.abs(m1 - m64) <= 1e-5 * np.abs(m64) + 2.0 ** -23 * np.abs((1 - b1) * gs)).all()
    assert np.array_equal(job.ga.get().astype(np.float64), g0) and all(x.guards_intact() for x in (job.actor, job.ga, m, v, nrm))
    assert (p1[-2:] == 0).all() and (m1[-2:] == 0).all() and (v1[-2:] == 0).all()       # 56 978 -> 56 980: the padding stays zero
    side.close()


def test_emulated_pointer_adam():
    adam_matches(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 7. trainer
ARGS = dict(batch_size=16, minibatch_size=16, n_updates_per_iteration=1)


def emu_train_env(B=3, M=2):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    side = EmuSide([synth_scenario(300 + e, 70, 60) for e in range(B)], DEFAULT_MC_SPEC, M, map_size=12, render=False, entities=True, auto_reset=True)
    return Q.emu_update_vec(side)


def block_grads(actor, critic):
    """float64 numpy gradients of the two modules in block layout, without the padding."""
    return np.concatenate([Q.grad_block(actor, Q.P_ACTOR)[:56978], Q.grad_block(critic, Q.P_CRITIC)[:48577]])


def trainer_updates_on_the_device(make_env, device, tmp_path):
    """device_update=True with fused_policy=True rolls out and updates.  On the trainer's first minibatch of 16 rows: clipfrac == 0 and
    |approx_kl| <= 1e-6; the device gradient's relative L2 distance from the float64 autograd gradient is at most 4 * d32 + 1e-6, d32 the
    distance of the float32 autograd gradient on the CPU (both printed).  Parameters change and stay finite, the torch optimisers are
    never stepped, checkpoints save and load."""
    import copy
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO, pack_entity_critic, pack_entity_pointer_actor
    torch.set_num_threads(2)
    env = make_env()
    M = env.num_agent
    torch.manual_seed(11); np.random.seed(3)
    algo = BatchedEntityPointerIPPO(ARGS, env, device=device, fused_policy=True, device_update=True)   # the nets as the trainer draws them
    batches = algo.roll_out()
    for a in range(M):
        batch = batches[a]
        state = np.random.get_state()
        probe = np.arange(16); np.random.shuffle(probe); np.random.set_state(state)   # the shuffle the update is about to draw
        cpu = {k: v.detach().cpu() for k, v in batch.items()}
        grads = {}
        for dt in (torch.float64, torch.float32):
            ac, cr = copy.deepcopy(algo.actors[a]).cpu().to(dt), copy.deepcopy(algo.critics[a]).cpu().to(dt)
            L = Q._Learner(ac, cr, dict(clip=algo.clip, ent_coef=algo.ent_coef, vf_coef=algo.vf_coef, norm_adv=algo.norm_adv, clip_vloss=algo.clip_vloss))
            b = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in cpu.items()}
            L.minibatch_loss(0, b, torch.as_tensor(probe))[0].backward()
            grads[dt] = block_grads(ac, cr)
        g64 = grads[torch.float64]
        d32 = float(np.linalg.norm(grads[torch.float32] - g64) / np.linalg.norm(g64))
        f32 = lambda x: x.to(device=env.device, dtype=torch.float32).contiguous()
        ba, bc = f32(pack_entity_pointer_actor(algo.actors[a])), f32(pack_entity_critic(algo.critics[a]))
        g_dev = torch.zeros(Q.P_ACTOR + Q.P_CRITIC, dtype=torch.float32, device=env.device)
        st_dev = torch.zeros(8, dtype=torch.float32, device=env.device)
        bb = {"actions": f32(batch["actions"]).reshape(-1, 2), "log_probs": f32(batch["log_probs"]), "advantages": f32(batch["advantages"]),
              "returns": f32(batch["returns"]), "values": f32(batch["values"])}
        hyper = dict(clip=algo.clip, ent_coef=algo.ent_coef, vf_coef=algo.vf_coef, norm_adv=algo.norm_adv, clip_vloss=algo.clip_vloss)
        env.entity_pointer_ppo_grad(ba, bc, f32(batch["states"]), torch.as_tensor(probe.astype(np.int32), device=env.device), bb, hyper, g_dev, st_dev)
        gd = g_dev.cpu().numpy().astype(np.float64)
        gd = np.concatenate([gd[:56978], gd[Q.P_ACTOR:Q.P_ACTOR + 48577]])
        dist = float(np.linalg.norm(gd - g64) / np.linalg.norm(g64))
        print("charger %d: relative L2 distance from the float64 gradient: device %.3g, float32 autograd %.3g" % (a, dist, d32))
        assert dist <= 4.0 * d32 + 1e-6, (a, dist, d32)
        before = pack_entity_pointer_actor(algo.actors[a]).clone()
        st = algo.update(a, batch)
        assert len(st) == 5 and all(np.isfinite(v) for v in st), st
        first = algo.first_minibatch_stats[a]
        assert all(np.isfinite(v) for v in first) and first[5] == 0.0 and abs(first[4]) <= 1e-6, first
        after = pack_entity_pointer_actor(algo.actors[a])
        assert not torch.equal(after, before) and bool(torch.isfinite(after).all())
        assert bool(torch.isfinite(pack_entity_critic(algo.critics[a])).all()) and algo._adam[a]["step"] == 1
    assert algo._packed is None
    for opt in algo.optimizers:
        assert len(opt.state) == 0                            # the torch optimisers were never stepped
    for a in range(M):
        algo.save_checkpoint(a, str(tmp_path / str(a)))
    other = BatchedEntityPointerIPPO(ARGS, env, device=device, model_path=str(tmp_path), device_update=True)
    assert torch.equal(other.packed_actors(), algo.packed_actors())
    env.side.close() if hasattr(env, "side") else env.close()


def test_emulated_pointer_trainer_updates_on_the_device(tmp_path):
    trainer_updates_on_the_device(emu_train_env, "cpu", tmp_path)


def default_update_is_untouched(make_env, device):
    """device_update=False: nothing of the option is allocated, and `update` gives the bytes of `PPOLearner.update` -- the code path the
    trainer had before the option existed -- called directly on a twin trainer under equal seeds."""
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO, pack_entity_critic
    from multi_agent_rl_wrsn_amd.ippo import PPOLearner
    torch.set_num_threads(2)
    packed = []
    for direct in (False, True):
        env = make_env()
        torch.manual_seed(11); np.random.seed(3)
        algo = BatchedEntityPointerIPPO(dict(batch_size=8, minibatch_size=4, n_updates_per_iteration=1), env, device=device, fused_policy=True)
        assert algo.device_update is False and not hasattr(algo, "_adam") and not hasattr(algo, "_grad")
        batches = algo.roll_out()
        for a in range(env.num_agent):
            PPOLearner.update(algo, a, batches[a]) if direct else algo.update(a, batches[a])
        packed.append((algo.packed_actors().clone(), torch.stack([pack_entity_critic(c) for c in algo.critics])))
        env.side.close() if hasattr(env, "side") else env.close()
    assert torch.equal(packed[0][0], packed[1][0]) and torch.equal(packed[0][1], packed[1][1])


def test_emulated_pointer_default_update_is_untouched():
    default_update_is_untouched(emu_train_env, "cpu")
