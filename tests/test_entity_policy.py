"""The set actor / critic over packed entity rows (`build_entity_networks`) and `EntityPPOLearner` on CPU torch, small sizes."""
import os

import numpy as np

N, M = 12, 2


def _rows(n, seed, dtype=None, n_node=N, n_mc=M):
    """n synthetic packed entity rows: some dead nodes (zeros but the position), some padded rows (all zero), one asking charger."""
    import torch
    from multi_agent_rl_wrsn_amd import ENT_ENV, ENT_MC, ENT_NODE, EntityTransitionBuffers
    g = torch.Generator().manual_seed(seed)
    nodes = torch.rand((n, n_node, 8), generator=g)
    own = torch.randint(n_node // 2, n_node + 1, (n,), generator=g)                  # the environment's own node count
    alive = (torch.rand((n, n_node), generator=g) < 0.7) & (torch.arange(n_node)[None] < own[:, None])
    nodes[..., ENT_NODE["alive"]] = alive.float()
    nodes[..., ENT_NODE["level"]] = torch.randint(1, 6, (n, n_node), generator=g).float()
    nodes[..., 2:] *= alive[..., None]
    nodes *= (torch.arange(n_node)[None] < own[:, None])[..., None]
    mcs = torch.rand((n, n_mc, 12), generator=g)
    asking = torch.randint(0, n_mc, (n,), generator=g)
    mcs[..., ENT_MC["is_self"]] = (torch.arange(n_mc)[None] == asking[:, None]).float()
    mcs[..., ENT_MC["alive"]] = 1.0
    mcs[..., ENT_MC["charging"]] = (torch.rand((n, n_mc), generator=g) < 0.5).float()
    mcs[..., 10:] = 0.0
    env = torch.rand((n, 8), generator=g)
    env[:, ENT_ENV["agent"]] = asking.float(); env[:, ENT_ENV["n_node"]] = own.float(); env[:, 6:] = 0.0
    rows = EntityTransitionBuffers.pack(nodes, mcs, env)
    return rows.to(dtype) if dtype is not None else rows


def _nets(dtype, seed=0):
    import torch
    from multi_agent_rl_wrsn_amd import build_entity_networks
    torch.manual_seed(seed)
    Actor, Critic = build_entity_networks(M)
    actor, critic = Actor().to(dtype), Critic().to(dtype)
    with torch.no_grad():                                      # the 0.01 heads would hide the trunk behind 1e-2: widen them for the comparison
        for lin in (actor.mean, actor.log_std, critic.value):
            lin.weight.mul_(30.0)
    return actor, critic


def _out(actor, critic, rows):
    import torch
    with torch.no_grad():
        mean, log_std = actor(rows)
        return torch.cat([mean, log_std, critic(rows)], 1)


def test_split_and_pack_are_inverse_views():
    import torch
    from multi_agent_rl_wrsn_amd import EntityTransitionBuffers, entity_row_elems
    rows = _rows(5, 1)
    assert rows.shape == (5, entity_row_elems(N, M)) == (5, 8 * N + 12 * M + 8)
    nodes, mcs, env = EntityTransitionBuffers.split(rows, M)
    assert nodes.shape == (5, N, 8) and mcs.shape == (5, M, 12) and env.shape == (5, 8)
    assert torch.equal(EntityTransitionBuffers.pack(nodes, mcs, env), rows)
    assert nodes.data_ptr() == rows.data_ptr()                 # views, not copies


def test_set_semantics_permutation_dead_rows_and_batch_independence():
    """7: in float64, permuting node rows, or charger rows together with is_self, moves actor and critic outputs by <= 1e-10; whatever
    dead and padded node rows hold besides the alive flag changes nothing, exactly; a row's output is bit-identical alone and inside a
    batch of 7."""
    import torch
    from multi_agent_rl_wrsn_amd import ENT_NODE, EntityTransitionBuffers
    torch.set_num_threads(2)
    actor, critic = _nets(torch.float64)
    rows = _rows(7, 3, torch.float64)
    base = _out(actor, critic, rows)
    assert base.abs().max() > 1e-2 and torch.isfinite(base).all()
    nodes, mcs, env = EntityTransitionBuffers.split(rows, M)
    g = torch.Generator().manual_seed(5)
    pn = torch.randperm(N, generator=g)
    assert not torch.equal(pn, torch.arange(N))
    d = (_out(actor, critic, EntityTransitionBuffers.pack(nodes[:, pn], mcs, env)) - base).abs().max()
    assert d <= 1e-10, float(d)
    pm = torch.tensor([1, 0])
    d = (_out(actor, critic, EntityTransitionBuffers.pack(nodes, mcs[:, pm], env)) - base).abs().max()   # is_self travels with its row
    assert d <= 1e-10, float(d)
    # the networks do look at what they are given: another live node feature moves the output
    live = nodes.clone(); live[..., ENT_NODE["energy_frac"]] += 0.25 * live[..., ENT_NODE["alive"]]
    assert (_out(actor, critic, EntityTransitionBuffers.pack(live, mcs, env)) - base).abs().max() > 1e-6
    # dead / padded rows: every feature but the alive flag overwritten, NaN and inf included
    dead = nodes[..., ENT_NODE["alive"]] != 1
    assert dead.any() and (~dead).any()
    for fill in (123.456, -1e30, float("inf"), float("nan")):
        junk = nodes.clone()
        for f in range(8):
            if f != ENT_NODE["alive"]:
                junk[..., f] = torch.where(dead, torch.full_like(junk[..., f], fill), junk[..., f])
        assert torch.equal(_out(actor, critic, EntityTransitionBuffers.pack(junk, mcs, env)), base), fill
    # a row with no live node pools to zeros: finite output
    none = nodes.clone(); none[0, :, ENT_NODE["alive"]] = 0.0
    assert torch.isfinite(_out(actor, critic, EntityTransitionBuffers.pack(none, mcs, env))).all()
    # alone == inside the batch of 7, bit for bit
    for k in range(7):
        assert torch.equal(_out(actor, critic, rows[k:k + 1]), base[k:k + 1]), k


_ARGS = dict(batch_size=48, minibatch_size=8, n_updates_per_iteration=2, lr=1e-3)


def _learner(seed=0, args=_ARGS, **kw):
    import torch
    from multi_agent_rl_wrsn_amd import EntityPPOLearner
    torch.manual_seed(seed)
    return EntityPPOLearner(args, M, "cpu", **kw)


def test_rollout_and_update_log_probabilities_agree():
    """8: at initial weights, get_action over 50 rows in chunks of 16 (the last one padded) against evaluate over shuffled minibatches
    of 8: |log-ratio| <= 1e-4 -- float32 GEMM rounding at sigma ~ 1 (log_std starts near 0); the first minibatch_loss has clipfrac 0,
    approx_kl <= 1e-6 and a non-zero actor gradient."""
    import torch
    torch.set_num_threads(2)
    lr = _learner(infer_chunk=16, min_bucket=16)
    rows = _rows(50, 11)
    torch.manual_seed(4)
    act, logp = lr.get_action(0, rows)
    assert act.shape == (50, 3) and logp.shape == (50,) and act.dtype == torch.float32
    with torch.no_grad():
        assert lr.actors[0](rows)[1].abs().max() < 0.5         # log_std near 0
    order = np.random.RandomState(2).permutation(50)
    worst = 0.0
    with torch.no_grad():
        for s in range(0, 50, 8):
            mb = torch.as_tensor(order[s:s + 8], dtype=torch.long)
            new, ent = lr.evaluate(0, rows[mb], act[mb])
            assert new.shape == (len(mb),) and ent.shape == (len(mb),)
            worst = max(worst, float((new - logp[mb]).abs().max()))
    print("max |log-ratio| over shuffled minibatches: %.3g" % worst)
    assert worst <= 1e-4, worst
    g = torch.Generator().manual_seed(9)
    batch = dict(states=rows[:48], actions=act[:48], log_probs=logp[:48], advantages=torch.randn(48, generator=g),
                 returns=torch.randn(48, generator=g), values=torch.randn(48, generator=g))
    mb = torch.as_tensor(order[order < 48][:8], dtype=torch.long)
    loss, pg, vl, en, kl, clipfrac = lr.minibatch_loss(0, batch, mb)
    print("first minibatch: clipfrac %g approx_kl %.3g" % (clipfrac, float(kl)))
    assert clipfrac == 0.0 and float(kl) <= 1e-6
    lr.optimizers[0].zero_grad(); loss.backward()
    gn = torch.sqrt(sum((p.grad ** 2).sum() for p in lr.actors[0].parameters() if p.grad is not None))
    assert float(gn) > 0 and torch.isfinite(gn)


def _batch(seed, n):
    import torch
    g = torch.Generator().manual_seed(seed)
    return dict(states=_rows(n, seed), actions=torch.randn((n, 3), generator=g), log_probs=torch.randn(n, generator=g) - 3.0,
                advantages=torch.randn(n, generator=g), returns=torch.randn(n, generator=g), values=torch.randn(n, generator=g))


def _flat(lr):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in list(lr.actors[0].parameters()) + list(lr.critics[0].parameters())]).clone()


def test_update_returns_finite_statistics_and_moves_both_networks():
    """9: EntityPPOLearner.update on a seeded synthetic batch."""
    import torch
    torch.set_num_threads(2)
    lr = _learner()
    a0 = [p.detach().clone() for p in lr.actors[0].parameters()]; c0 = [p.detach().clone() for p in lr.critics[0].parameters()]
    st = lr.update(0, _batch(21, 48), shuffle=np.random.RandomState(3).shuffle)
    assert len(st) == 5 and all(np.isfinite(v) for v in st)
    assert any(not torch.equal(p, q) for p, q in zip(lr.actors[0].parameters(), a0))
    assert any(not torch.equal(p, q) for p, q in zip(lr.critics[0].parameters(), c0))
    assert all(torch.isfinite(p).all() for p in list(lr.actors[0].parameters()) + list(lr.critics[0].parameters()))


_DP_ARGS = dict(batch_size=8, minibatch_size=4, n_updates_per_iteration=2, lr=1e-3)


def _dp_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    torch.set_num_threads(2)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from multi_agent_rl_wrsn_amd import EntityPPOLearner
    torch.manual_seed(100 + rank)                              # different initial weights per rank: the broadcast must equalise them
    lr = EntityPPOLearner(_DP_ARGS, M, "cpu")
    p0 = _flat(lr)
    lr.update(0, _batch(7 + rank, 8), shuffle=np.random.RandomState(3).shuffle)      # a different local batch per rank
    q.put((rank, p0.numpy(), _flat(lr).numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_update_leaves_both_ranks_with_identical_parameters_gloo_world2():
    """9: two gloo ranks with different initial seeds and different local batches: broadcast at construction, one all-reduce per minibatch."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps: p.start()
    (_, a0, a1), (_, b0, b1) = sorted([q.get(timeout=300) for _ in ps], key=lambda t: t[0])
    for p in ps: p.join(timeout=60)
    assert all(p.exitcode == 0 for p in ps)
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    assert np.abs(a1 - a0).max() > 1e-4                        # four Adam steps of lr 1e-3


# state_dict keys and shapes of the image learner's networks at map size 12, as the parent commit constructs them
_IMAGE_ACTOR = {"log_std": (1, 1, 12, 12), "inc.conv.weight": (64, 4, 3, 3), "inc.conv.bias": (64,), "inc.bn.weight": (64,), "inc.bn.bias": (64,),
                "inc.bn.running_mean": (64,), "inc.bn.running_var": (64,), "inc.bn.num_batches_tracked": (),
                "down1.conv_block.conv.weight": (128, 64, 3, 3), "down1.conv_block.conv.bias": (128,), "down1.conv_block.bn.weight": (128,),
                "down1.conv_block.bn.bias": (128,), "down1.conv_block.bn.running_mean": (128,), "down1.conv_block.bn.running_var": (128,),
                "down1.conv_block.bn.num_batches_tracked": (),
                "down2.conv_block.conv.weight": (256, 128, 3, 3), "down2.conv_block.conv.bias": (256,), "down2.conv_block.bn.weight": (256,),
                "down2.conv_block.bn.bias": (256,), "down2.conv_block.bn.running_mean": (256,), "down2.conv_block.bn.running_var": (256,),
                "down2.conv_block.bn.num_batches_tracked": (),
                "up1.conv_block.conv.weight": (128, 384, 3, 3), "up1.conv_block.conv.bias": (128,), "up1.conv_block.bn.weight": (128,),
                "up1.conv_block.bn.bias": (128,), "up1.conv_block.bn.running_mean": (128,), "up1.conv_block.bn.running_var": (128,),
                "up1.conv_block.bn.num_batches_tracked": (),
                "up2.conv_block.conv.weight": (64, 192, 3, 3), "up2.conv_block.conv.bias": (64,), "up2.conv_block.bn.weight": (64,),
                "up2.conv_block.bn.bias": (64,), "up2.conv_block.bn.running_mean": (64,), "up2.conv_block.bn.running_var": (64,),
                "up2.conv_block.bn.num_batches_tracked": (),
                "out_mean.conv.weight": (1, 64, 3, 3), "out_mean.conv.bias": (1,)}
_IMAGE_CRITIC = {"conv1.weight": (16, 4, 5, 5), "conv1.bias": (16,), "conv2.weight": (32, 16, 5, 5), "conv2.bias": (32,),
                 "conv3.weight": (64, 32, 5, 5), "conv3.bias": (64,), "fc1.weight": (100, 256), "fc1.bias": (100,), "fc2.weight": (1, 100), "fc2.bias": (1,)}


def test_image_learner_keeps_its_state_dict_and_its_initial_weights():
    """9: PPOLearner (image) after the refactor: the keys and shapes recorded from the parent commit, the same modules as
    build_networks gives, and -- under one seed -- the weights a direct construction in the parent's order (actors, then critics) draws."""
    import torch
    from multi_agent_rl_wrsn_amd import EntityPPOLearner, PPOLearner, build_networks
    torch.manual_seed(5)
    lr = PPOLearner(dict(batch_size=8, minibatch_size=4), 2, 12, "cpu")
    assert PPOLearner._logp_dims == (1, 2) and EntityPPOLearner._logp_dims == (1,)
    for net, want in ((lr.actors[0], _IMAGE_ACTOR), (lr.critics[1], _IMAGE_CRITIC)):
        got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        assert got == want
    torch.manual_seed(5)
    UNet, CNNCritic = build_networks(12)
    actors = [UNet() for _ in range(2)]; critics = [CNNCritic() for _ in range(2)]
    for mine, ref in zip(lr.actors + lr.critics, actors + critics):
        a, b = mine.state_dict(), ref.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
