"""The PPO update of the entity policy (wrsn_entity_eval, wrsn_entity_ppo_grad, wrsn_entity_adam; csrc/wrsn_entity_train.h) on the
emulated library.

The bodies take the side (tests/sides.py): this module runs them on EmuSide, tests/test_entity_update_gpu.py on VecSide.  Memory, nets, the
reference (the module and PPOLearner.minibatch_loss in float64 on the CPU; bounds 4 * err32 + 1e-6, for a gradient tensor 4 * err32 +
1e-6 * max|g64|) and the kink margins that keep the gradient comparison honest are in tests/entity_train_ref.py."""
import numpy as np
import pytest
from sides import EmuSide

import entity_act_ref as R
import entity_train_ref as T
import test_entity_act as A

# (n, N, M) -> seed of make_rows / make_batch whose float64 kink margins clear 8 * err32 + 2e-6 (T.find_seed; asserted again in every test)
GRAD_CASES = {(8, 70, 3): 2, (8, 33, 3): 1, (2, 257, 3): 3, (4, 33, 8): 0}
FWD_CASES = [(24, 70, 3), (24, 33, 3), (24, 257, 3), (8, 33, 8)]
# One seed for the rows of every forward case.  err32 over 24 rows is a noisy estimate of the error of the 128-long float32 dot products
# behind log_std (1.6e-7 to 3.2e-6 over seeds 40 .. 45 on the CPU, 1e-6 typically); the kernel's own deviation there is that of
# wrsn_entity_act, whose bytes it reproduces.  Seed 40 has a typical err32 at all four shapes.
FWD_SEED = 40

_REFS = {}


def grad_case(shape, hyper=T.HYPER):
    """(nets, rows, batch, Ref) of a gradient case: computed once, shared by every test and both sides, never modified."""
    key = (shape, tuple(sorted(hyper.items())))
    if key not in _REFS:
        n, N, M = shape
        nets = T.make_nets(M)
        rows = T.make_rows(GRAD_CASES[shape], n, N, M)
        batch = T.make_batch(GRAD_CASES[shape], rows, *nets)
        _REFS[key] = (nets, rows, batch, T.Ref(nets[0], nets[1], rows, batch, hyper, M))
    return _REFS[key]


def side_for(Side, N, M, B=2, **kw):
    return A.make_side(Side, N, B, M, **kw)


# ------------------------------------------------------------------------------------------------------------ 1. layout
def layout_matches_the_header(lib):
    """The critic block built by hand from the header's offsets equals pack_entity_critic; 48 580 floats; pack -> unpack -> pack is
    bit-identical for both nets."""
    import torch
    from multi_agent_rl_wrsn_amd import (build_entity_networks, pack_entity_actor, pack_entity_critic, unpack_entity_actor, unpack_entity_critic)
    assert lib.wrsn_entity_critic_floats() == 48580 == T.P_CRITIC and lib.wrsn_entity_actor_floats() == T.P_ACTOR
    actor, critic = T.make_nets(3)
    blk = np.zeros(48580, np.float32)
    t = critic.trunk
    for off, lay in ((0, t.node1), (576, t.node2), (4736, t.mc1), (5152, t.mc2), (6208, t.head1), (31936, t.head2), (48448, critic.value)):
        w, b = lay.weight.detach().numpy(), lay.bias.detach().numpy()
        blk[off:off + w.size] = w.T.reshape(-1); blk[off + w.size:off + w.size + b.size] = b
    assert 48448 + 128 == 48576 and blk[48577:].tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(blk.view(np.uint32), pack_entity_critic(critic).numpy().view(np.uint32))
    Actor, Critic = build_entity_networks(3)
    a2, c2 = Actor(), Critic()
    unpack_entity_actor(pack_entity_actor(actor), a2); unpack_entity_critic(pack_entity_critic(critic), c2)
    assert torch.equal(pack_entity_actor(a2), pack_entity_actor(actor)) and torch.equal(pack_entity_critic(c2), pack_entity_critic(critic))
    for p, q in zip(list(a2.parameters()) + list(c2.parameters()), list(actor.parameters()) + list(critic.parameters())):
        assert torch.equal(p, q)


def test_emulated_entity_critic_layout():
    from emu_env import emu_lib
    layout_matches_the_header(emu_lib())


# ------------------------------------------------------------------------------------------------------------ 2. forward
def forward_matches(Side, shape):
    """Through index = NULL and through a permuting index with repeats: against float64; mean / log_std bit-equal to wrsn_entity_act on the
    same row contents; NaN / inf in dead node rows and a row with no alive node give the bytes zeros give; actor = NULL and critic = NULL."""
    n, N, M = shape
    nets = T.make_nets(M)
    ids = np.zeros(n, np.int32)
    node, mc, env = R.synth_rows(FWD_SEED, n, N, M, ids)
    node[1, :, 7] = 0.0; node[1, :, 2:7] = 0.0                # row 1: no alive node
    rows = R.pack_rows(node, mc, env)
    ref = T.Ref(nets[0], nets[1], rows, None, T.HYPER, M)
    ls = ref.f64["log_std"]
    assert (ls == -4.0).any() and (ls == 1.0).any() and ((ls > -4.0) & (ls < 1.0)).any()
    side = side_for(Side, N, M, B=n)
    job = T.Job(side, nets, rows, None, N, M)
    got = job.eval()
    assert all(np.isfinite(v).all() for v in got.values())
    ref.check_forward(got, "%s %s" % (side.name, shape))
    assert all(o.guards_intact() for o in job.outs)
    # wrsn_entity_act on the same contents (its block 0 is this actor)
    act = R.Call(side, M, node, mc, env, ids, None).run()
    assert np.array_equal(got["mean"].view(np.uint32), act["mean"].view(np.uint32))
    assert np.array_equal(got["log_std"].view(np.uint32), act["log_std"].view(np.uint32))
    # a permuting index with repeats
    idx = np.random.default_rng(n).permutation(n).astype(np.int32); idx[-2:] = idx[:2]
    jobi = T.Job(side, nets, rows, None, N, M, index=idx)
    goti = jobi.eval()
    for k in got:
        assert np.array_equal(goti[k].view(np.uint32), got[k][idx].view(np.uint32)), k
    # dead rows hold NaN and inf
    bad = node.copy()
    dead = bad[..., 7] == 0
    assert dead[0].any() and (~dead[0]).any() and dead[1].all()
    bad[..., :7][dead] = np.where(np.arange(7) % 2 == 0, np.nan, np.inf).astype(np.float32)
    gotb = T.Job(side, nets, R.pack_rows(bad, mc, env), None, N, M).eval()
    for k in got:
        assert np.array_equal(gotb[k].view(np.uint32), got[k].view(np.uint32)), k
    # one net only
    job.fill(); only_c = job.eval(actor=False)
    assert job.mean.untouched() and job.log_std.untouched() and np.array_equal(only_c["value"], got["value"])
    job.fill(); only_a = job.eval(critic=False)
    assert job.value.untouched() and np.array_equal(only_a["mean"], got["mean"]) and np.array_equal(only_a["log_std"], got["log_std"])
    side.close()


@pytest.mark.parametrize("shape", FWD_CASES)
def test_emulated_entity_eval(shape):
    forward_matches(EmuSide, shape)


# ------------------------------------------------------------------------------------------------------------ 3. loss
LOSS_HYPERS = [dict(norm_adv=True, clip_vloss=True, ent_coef=0.01), dict(norm_adv=False, clip_vloss=True, ent_coef=0.0),
               dict(norm_adv=True, clip_vloss=False, ent_coef=0.0), dict(norm_adv=False, clip_vloss=False, ent_coef=0.01)]
_LOSS = {}


def loss_case(i):
    if i not in _LOSS:
        n, N, M = 24, 33, 3
        hyper = dict(T.HYPER); hyper.update(LOSS_HYPERS[i])
        nets = T.make_nets(M)
        rows = T.make_rows(5, n, N, M)
        batch = T.make_batch(5, rows, *nets)
        _LOSS[i] = (nets, rows, batch, hyper, T.Ref(nets[0], nets[1], rows, batch, hyper, M))
    return _LOSS[i]


def loss_matches(Side, i):
    """The statistics against float64 (clipfrac exactly) on 24 rows whose ratios lie below, inside and above the clip range with
    advantages of both signs, where both value terms win somewhere and log_std is clamped at both ends."""
    nets, rows, batch, hyper, ref = loss_case(i)
    clip = hyper["clip"]
    r, adv = ref.q64["ratio"], batch["advantage"]
    for sel in (r < 1 - clip, r > 1 + clip):
        assert (sel & (adv > 0)).any() and (sel & (adv < 0)).any()
    assert ((r > 1 - clip) & (r < 1 + clip)).any()
    assert (ref.q64["v_diff"] > 0).any() and (ref.q64["v_diff"] < 0).any()
    ls = ref.f64["log_std"]
    assert (ls == -4.0).any() and (ls == 1.0).any()
    side = side_for(Side, 33, 3)
    job = T.Job(side, nets, rows, batch, 33, 3, hyper=hyper)
    _, _, stats = job.grad()
    ref.check_stats(stats, "%s loss %d" % (side.name, i))
    side.close()


@pytest.mark.parametrize("i", range(len(LOSS_HYPERS)))
def test_emulated_entity_ppo_loss(i):
    loss_matches(EmuSide, i)


# ------------------------------------------------------------------------------------------------------------ 4. gradient
def gradient_matches(Side, shape):
    """Every tensor of both blocks against float64 autograd, under the kink assertion; padding zero; two calls give equal bytes; outputs
    sit between intact guards; at (8, 33, 3) also: NaN in dead rows gives the bytes zeros give, and the log_std gradients of a clamped
    row are exactly zero."""
    n, N, M = shape
    nets, rows, batch, ref = grad_case(shape)
    ref.assert_margins(str(shape))
    side = side_for(Side, N, M)
    job = T.Job(side, nets, rows, batch, N, M)
    ga, gc, stats = job.grad()
    first = [o.snap() for o in job.outs]
    ref.check_stats(stats, "%s %s" % (side.name, shape))
    ref.check_grads(ga, gc, nets, "%s %s" % (side.name, shape))
    assert all(o.guards_intact() for o in (job.ga, job.gc, job.stats))
    job.fill(); job.grad()
    assert all(np.array_equal(a, o.snap()) for a, o in zip(first, job.outs))             # 5: two calls, equal bytes
    if shape == (8, 33, 3):
        node, mc, env = R.synth_rows(GRAD_CASES[shape], n, N, M, np.zeros(n, np.int32))
        dead = node[..., 7] == 0
        node[..., 2:7][dead] = np.nan
        jb = T.Job(side, nets, R.pack_rows(node, mc, env), batch, N, M)
        gb = jb.grad()
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(gb, (ga, gc, stats)))
        ls = ref.f64["log_std"]
        r, d = np.argwhere((ls == -4.0) | (ls == 1.0))[0]
        hyper = dict(T.HYPER, norm_adv=False)
        j1 = T.Job(side, nets, rows, batch, N, M, index=[int(r)], hyper=hyper)
        g1, _, _ = j1.grad()
        sl = T.block_slices(nets[0])
        assert (g1[sl["log_std.w"]].reshape(128, 3)[:, d] == 0).all() and g1[sl["log_std.b"]][d] == 0
        assert np.abs(g1[sl["mean.w"]]).max() > 0
    side.close()


@pytest.mark.parametrize("shape", list(GRAD_CASES))
def test_emulated_entity_ppo_grad(shape):
    gradient_matches(EmuSide, shape)


# ------------------------------------------------------------------------------------------------------------ 5. extent
def extent_is_respected(Side):
    """A call with n = 5 of 8 rows writes nothing beyond its outputs: rows 5 .. 7 of the forward outputs keep the pattern, every guard is
    intact, and the statistics and gradients are those of the 5-row minibatch."""
    shape = (8, 33, 3)
    n, N, M = shape
    nets, rows, batch, _ = grad_case(shape)
    side = side_for(Side, N, M)
    job = T.Job(side, nets, rows, batch, N, M)
    job.eval(n=5)
    for o in (job.mean, job.log_std, job.value):
        s = o.snap()
        per = o.nbytes // n
        assert (s[T.GUARD + 5 * per:] == T.PATTERN).all() and (s[:T.GUARD] == T.PATTERN).all()
        assert not (s[T.GUARD:T.GUARD + 5 * per] == T.PATTERN).all()
    ga, gc, st = job.grad(n=5)
    assert all(o.guards_intact() for o in job.outs)
    ref5 = T.Ref(nets[0], nets[1], rows[:5], {k: v[:5] for k, v in batch.items()}, T.HYPER, M)
    ref5.check_stats(st, "%s 5 of 8" % side.name)
    side.close()


def test_emulated_entity_update_extent():
    extent_is_respected(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 6. bad arguments
def bad_arguments_leave_everything_untouched(Side):
    """Every WRSN_ERR_ARG case leaves the pattern-filled outputs untouched; the valid call that follows gives the bytes of case 4."""
    from multi_agent_rl_wrsn_amd._lib import WrsnError
    WRSN_ERR_ARG = -1
    shape = (8, 33, 3)
    n, N, M = shape
    nets, rows, batch, _ = grad_case(shape)
    side = side_for(Side, N, M)
    job = T.Job(side, nets, rows, batch, N, M)
    want = job.grad()
    off_a = T.Guarded(side, (T.P_ACTOR,), data=T.pack(nets[0]), shift=4)
    off_r = T.Guarded(side, rows.shape, data=rows, shift=4)
    off_g = T.Guarded(side, (T.P_ACTOR,), shift=4)
    h = side.handle
    grad_bad = [dict(actor_ptr=0), dict(critic_ptr=0), dict(rows_ptr=0), dict(grad_actor=0), dict(grad_critic=0), dict(stats=0), dict(action=0),
                dict(logp_old=0), dict(advantage=0), dict(ret=0), dict(value_old=0), dict(actor_ptr=off_a.ptr), dict(rows_ptr=off_r.ptr),
                dict(grad_actor=off_g.ptr), dict(n=0), dict(n=1), dict(n_mc=0), dict(n_mc=9), dict(n_node=0)]
    eval_bad = [dict(actor_ptr=0, critic_ptr=0), dict(rows_ptr=0), dict(mean=0, log_std=0), dict(value=0), dict(actor_ptr=0), dict(critic_ptr=0),
                dict(critic_ptr=job.critic.ptr + 4), dict(rows_ptr=off_r.ptr), dict(n=0), dict(n_mc=9), dict(n_node=0)]
    for kind, cases in (("grad", grad_bad), ("eval", eval_bad)):
        for over in cases:
            job.fill(); off_g.fill()
            with pytest.raises(WrsnError) as ei:
                (job.grad if kind == "grad" else job.eval)(**over)
            assert ei.value.code == WRSN_ERR_ARG, (kind, over)
            assert all(o.untouched() for o in job.outs) and off_g.untouched(), (kind, over)
            if kind == "grad":
                got = job.grad()
                assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, want)), over
    # adam
    p = T.Guarded(side, (T.P_CRITIC,), data=T.pack(nets[1])); m = T.Guarded(side, (T.P_CRITIC,), data=np.zeros(T.P_CRITIC))
    v = T.Guarded(side, (T.P_CRITIC,), data=np.zeros(T.P_CRITIC)); nrm = T.Guarded(side, (1,))
    before = [x.snap() for x in (p, m, v, nrm)]
    base = dict(param=p.ptr, grad=job.gc.ptr, m=m.ptr, v=v.ptr, n_floats=T.P_CRITIC, step=1, lr=1e-3, norm_out=nrm.ptr)
    for over in (dict(param=0), dict(grad=0), dict(m=0), dict(v=0), dict(step=0), dict(n_floats=0), dict(param=p.ptr + 4), dict(grad=job.gc.ptr + 4)):
        with pytest.raises(WrsnError) as ei:
            h.entity_adam(**dict(base, **over))
        assert ei.value.code == WRSN_ERR_ARG, over
        R.sync(side)
        assert all(np.array_equal(a, x.snap()) for a, x in zip(before, (p, m, v, nrm))), over
    side.close()


def test_emulated_entity_update_bad_arguments():
    bad_arguments_leave_everything_untouched(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 7. Adam
def adam64(p, g, m, v, step, lr, b1, b2, eps, max_norm):
    """float64 clip_grad_norm_ + torch.optim.Adam restarted from (p, m, v) after step - 1 steps: (p', m', v', ||g||)."""
    import torch
    q = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    q.grad = torch.tensor(g, dtype=torch.float64)
    norm = float(torch.nn.utils.clip_grad_norm_([q], max_norm))
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.tensor(m, dtype=torch.float64), exp_avg_sq=torch.tensor(v, dtype=torch.float64))
    opt.step()
    return q.detach().numpy(), opt.state[q]["exp_avg"].numpy(), opt.state[q]["exp_avg_sq"].numpy(), norm


def adam_matches(Side):
    """Three steps on the kernel's own gradients, each compared with float64 restarted from the kernel's previous p, m, v:
    |delta - delta64| <= 1e-5 |delta64| + one float32 ulp of p; v to 1e-5 relative; m to 1e-5 relative plus one float32 ulp of its two
    terms beta1 m and (1 - beta1) g, which cancel where the gradient changes sign (no float32 sum can promise more there); the norm
    against float64.  The actor's norm lies
    above its max_norm, the critic's below; the actor block (49 224 floats) is no multiple of 256."""
    shape = (8, 33, 3)
    n, N, M = shape
    nets, rows, batch, _ = grad_case(shape)
    side = side_for(Side, N, M)
    job = T.Job(side, nets, rows, batch, N, M)
    lr, eps = 1e-3, 1e-8
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))  # what the C-ABI's float arguments hold
    assert T.P_ACTOR % 256 != 0
    mom = {w: (T.Guarded(side, (P,), data=np.zeros(P)), T.Guarded(side, (P,), data=np.zeros(P))) for w, P in (("a", T.P_ACTOR), ("c", T.P_CRITIC))}
    nrm = T.Guarded(side, (1,))
    for step in (1, 2, 3):
        job.grad()
        for w, blk, g, P in (("a", job.actor, job.ga, T.P_ACTOR), ("c", job.critic, job.gc, T.P_CRITIC)):
            p0, g0, m0, v0 = blk.get().astype(np.float64), g.get().astype(np.float64), mom[w][0].get().astype(np.float64), mom[w][1].get().astype(np.float64)
            n64 = float(np.sqrt((g0 * g0).sum()))
            max_norm = 0.5 * n64 if w == "a" else 2.0 * n64
            max_norm = float(np.float32(max_norm))
            side.handle.entity_adam(blk.ptr, g.ptr, mom[w][0].ptr, mom[w][1].ptr, P, step, lr, b1, b2, eps, max_norm, nrm.ptr)
            R.sync(side)
            p64, m64, v64, norm = adam64(p0, g0, m0, v0, step, lr, b1, b2, eps, max_norm)
            assert (norm > max_norm) if w == "a" else (norm < max_norm)
            got_n = float(nrm.get()[0])
            assert abs(got_n - norm) <= 1e-6 * norm, (w, step, got_n, norm)
            p1, m1, v1 = blk.get(), mom[w][0].get().astype(np.float64), mom[w][1].get().astype(np.float64)
            d, d64 = p1.astype(np.float64) - p0, p64 - p0
            ulp = np.spacing(np.abs(p0).astype(np.float32)).astype(np.float64)
            worst = float((np.abs(d - d64) - (1e-5 * np.abs(d64) + ulp)).max())
            print("%s adam step %d %s: norm %.6g, largest excess over the bound %.3g, max|delta| %.3g" % (side.name, step, w, got_n, worst, np.abs(d64).max()))
            assert worst <= 0, (w, step, worst)
            assert (np.abs(v1 - v64) <= 1e-5 * np.abs(v64)).all(), (w, step)
            gs = g0 * min(1.0, max_norm / (norm + 1e-6))
            cancel = 2.0 ** -23 * (np.abs(b1 * m0) + np.abs((1 - b1) * gs))                 # one float32 ulp of the two terms m is the sum of
            assert (np.abs(m1 - m64) <= 1e-5 * np.abs(m64) + cancel).all(), (w, step)
            assert np.array_equal(g.get().astype(np.float64), g0)                         # the gradient is left as it is
            assert all(x.guards_intact() for x in (blk, g, mom[w][0], mom[w][1], nrm))
            pad = 2 if w == "a" else 3                         # 49 222 -> 49 224, 48 577 -> 48 580
            assert (p1[-pad:] == 0).all() and (m1[-pad:] == 0).all() and (v1[-pad:] == 0).all()   # padding stays zero
    side.close()


def test_emulated_entity_adam():
    adam_matches(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 8. trainer
def test_emulated_fused_update_trainer():
    """B = 16, N = 33, batch 8, minibatch 4, one epoch from a fresh reset, through the adapter: finite statistics, the modules equal the
    unpacked blocks bit for bit, first_minibatch_stats shows clipfrac 0 and |approx_kl| <= 1e-6, `_packed` is dropped."""
    import torch
    from multi_agent_rl_wrsn_amd import (DEFAULT_MC_SPEC, BatchedEntityIPPO, pack_entity_actor, pack_entity_critic, synth_scenario)
    torch.set_num_threads(2)
    M = 2
    side = EmuSide([synth_scenario(411 + e, 33, 17) for e in range(16)], DEFAULT_MC_SPEC, M, map_size=12, render=False, entities=True, auto_reset=True)
    env = T.EmuTrainVec(side)
    torch.manual_seed(11); np.random.seed(3)
    algo = BatchedEntityIPPO(dict(batch_size=8, minibatch_size=4, n_updates_per_iteration=1), env, device="cpu", fused_policy=True, fused_update=True)
    batches = algo.roll_out(max_launches=40)
    before = [pack_entity_actor(a).clone() for a in algo.actors]
    calls = []
    inner = env.entity_adam
    env.entity_adam = lambda *a, **kw: (calls.append(a[0]), inner(*a, **kw))[1]    # a[0]: the block the call steps in place
    for a in range(M):
        st = algo.update(a, batches[a])
        assert len(st) == 5 and all(np.isfinite(v) for v in st), st
        first = algo.first_minibatch_stats[a]
        assert all(np.isfinite(v) for v in first), first
        assert first[5] == 0.0 and abs(first[4]) <= 1e-6, first
        assert len(algo.loggers[a]["losses"]) == 2 and all(np.isfinite(v) for v in algo.loggers[a]["losses"])
        assert not torch.equal(pack_entity_actor(algo.actors[a]), before[a])
        assert algo._adam[a]["step"] == 2
    assert algo._packed is None
    assert len(calls) == 2 * 2 * M                            # per minibatch: the actor's and the critic's Adam call
    for opt in algo.optimizers:
        assert len(opt.state) == 0                            # the torch optimisers were never stepped
    # the blocks the last Adam calls left are what the modules hold, bit for bit: pack -> the same bytes
    blk_a, blk_c = calls[-2], calls[-1]
    assert torch.equal(pack_entity_actor(algo.actors[M - 1]), blk_a) and torch.equal(pack_entity_critic(algo.critics[M - 1]), blk_c)
    side.close()


# ------------------------------------------------------------------------------------------------------------ 9. data-parallel
def _dp_worker(rank, port, q):
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=2)
    flat = torch.arange(T.P_ACTOR + T.P_CRITIC, dtype=torch.float32) * (1.0 if rank == 0 else -3.0) + rank
    dist.all_reduce(flat); flat /= 2
    want = (torch.arange(T.P_ACTOR + T.P_CRITIC, dtype=torch.float32) * (1.0 - 3.0) + 1.0) / 2
    q.put((rank, bool(torch.equal(flat, want))))
    dist.destroy_process_group()


def test_flat_gradient_exchange_is_the_mean():
    """World 2, gloo, plain tensors: the exchange of the fused update (one all_reduce of the flat [P_actor + P_critic] tensor, divided by
    the world size) is the hand-computed mean.  No kernel is involved."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_dp_worker, args=(r, port, q)) for r in range(2)]
    for p in ps: p.start()
    res = sorted(q.get(timeout=120) for _ in ps)
    for p in ps: p.join(60)
    assert res == [(0, True), (1, True)]
