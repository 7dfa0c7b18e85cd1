"""The node-pointer entity policy (build_entity_pointer_networks, wrsn_entity_pointer_act, BatchedEntityPointerIPPO, PointerPolicy) on the
emulated library.

The bodies take the side (tests/sides.py): this module runs them on EmuSide, tests/test_entity_pointer_gpu.py on VecSide.  The reference (the
module in float64 on the CPU), the bound b = 4 * err32 + 1e-6, the actors and the memory handling are in tests/entity_pointer_ref.py; the
shapes are those of tests/test_entity_act.py: B = 96, M = 3 and M = 8, N = 33 (one full tile plus one node), 70 (a ragged third tile), 257
(more tiles than waves)."""
import os

import numpy as np
import pytest
from sides import EmuSide

import entity_act_ref as R
import entity_pointer_ref as P
from test_entity_act import B1, M1, case1_ids, make_side

_CASE = {}


def case(N, M=M1, sampled=True):
    """(ids, gumbel, eps, node, mc, env, Ref) at N nodes and M chargers: computed once, shared by every test and both sides."""
    key = (N, M, sampled)
    if key not in _CASE:
        ids = case1_ids() if M == M1 else (np.arange(B1) % M).astype(np.int32)
        node, mc, env = R.synth_rows(5 + N + M, B1, N, M, ids)
        g = P.gumbel_noise(40 + N, B1, N) if sampled else None
        eps = np.random.default_rng(2).standard_normal(B1).astype(np.float32) if sampled else None
        _CASE[key] = (ids, g, eps, node, mc, env, P.Ref(P.make_actors(M), R.pack_rows(node, mc, env), ids, g, eps))
    return _CASE[key]


def case_call(side, N, M=M1, sampled=True):
    ids, g, eps, node, mc, env, ref = case(N, M, sampled)
    return P.Call(side, M, node, mc, env, ids, g, eps), ref


SHAPES = [(70, 3), (33, 3), (257, 3), (33, 8)]


# ------------------------------------------------------------------------------------------------------------ 1. scores, 2. choice
@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("sampled", [True, False])
def test_reference_separates_the_nodes(N, M, sampled):
    """On the reference alone: logits spread by several units, log_std hits both clamps, and on at least 90 % of the rows the best
    perturbed score leads the runner-up by more than 2 b -- so the choice test is not vacuous."""
    ref = case(N, M, sampled)[6]
    l = ref.f64["logits"]
    spread = np.array([np.ptp(row[np.isfinite(row)]) for row in l])
    print("N=%d M=%d: median logit spread %.2f, b %s" % (N, M, np.median(spread), ref.b))
    assert np.median(spread) > 3.0
    ls = ref.f64["log_std"]
    assert (ls == -4.0).any() and (ls == 1.0).any() and ((ls > -4.0) & (ls < 1.0)).any()
    sc = ref.perturbed()
    top2 = -np.sort(-sc, axis=1)[:, :2]
    assert ((top2[:, 0] - top2[:, 1]) > 2.0 * ref.b["logits"]).mean() >= 0.9


def scores_and_choice_match(Side, N, M, sampled):
    side = make_side(Side, N, B1, M)
    call, ref = case_call(side, N, M, sampled)
    assert ref.rows_in == list(range(B1))
    got = call.run()
    tag = "%s N=%d M=%d %s" % (side.name, N, M, "sampled" if sampled else "mode")
    ref.check_scores(got, tag)
    share = ref.check_choice(got, tag)
    assert share >= 0.9
    assert call.out.guards_intact(call.out.snap())
    side.close()


@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("sampled", [True, False])
def test_emulated_pointer_scores_and_choice(N, M, sampled):
    scores_and_choice_match(EmuSide, N, M, sampled)


# ------------------------------------------------------------------------------------------------------------ 3. ties
def ties_go_to_the_lower_index(Side):
    """N = 257: two alive nodes with identical features and equal noise, in different tiles and waves (node 3: tile 0, wave 0; node 200:
    tile 6, wave 2; and 70 / 133: tiles 2 and 4).  Their logits are bit-equal, so node_logp is, and when the noise makes the pair the
    global maximum the lower index is chosen."""
    N, B, M = 257, 8, 3
    side = make_side(Side, N, B, M)
    ids = (np.arange(B) % M).astype(np.int32)
    node, mc, env = R.synth_rows(91, B, N, M, ids)
    pairs = [(3, 200), (70, 133), (200, 256), (31, 32)]
    g = P.gumbel_noise(92, B, N)
    for e in range(B):
        lo, hi = pairs[e % 4]
        node[e, lo, 2:] = node[e, hi, 2:] = node[e, 5, 2:]; node[e, lo, 7] = node[e, hi, 7] = 1.0
        node[e, hi, :2] = node[e, lo, :2]                      # identical eight features
        g[e, hi] = g[e, lo]
        if e >= 4:
            g[e, lo] = g[e, hi] = 50.0                         # the planted pair is the global maximum
    got = P.Call(side, M, node, mc, env, ids, g, None).run()
    for e in range(B):
        lo, hi = pairs[e % 4]
        assert got["node_logp"][e, lo].tobytes() == got["node_logp"][e, hi].tobytes(), e
        if e >= 4:
            assert got["node"][e] == lo, (e, got["node"][e])
        else:
            assert got["node"][e] != hi, e
    side.close()


def test_emulated_pointer_ties():
    ties_go_to_the_lower_index(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 4. masks
def masks_are_selects(Side):
    """M = 8, N = 33.  Row 0: dead nodes hold NaN and inf; row 1: no alive node; row 2: no alive charger; row 3: is_self on another
    charger than agent_id; row 4: no alive node and no is_self (own position = row agent_id); rows 5, 9: skipped."""
    B, M, N = 16, 8, 33
    side = make_side(Side, N, B, M)
    ids = (np.arange(B) % M).astype(np.int32)
    ids[5], ids[9] = -1, M
    node, mc, env = R.synth_rows(77, B, N, M, ids)
    dead = node[0, :, 7] == 0
    assert dead.any() and (~dead).any()
    node[0, dead, :7] = np.where(np.arange(7) % 2 == 0, np.nan, np.inf).astype(np.float32)
    node[1, :, 7] = 0.0; node[1, :, :7] = np.nan
    mc[2, :, 4] = 0.0
    mc[3, :, 3] = 0.0; mc[3, (int(ids[3]) + 2) % M, 3] = 1.0
    node[4, :, 7] = 0.0; mc[4, :, 3] = 0.0
    node[6, :, 7] = 0.0; mc[6, :, 3] = 0.0; mc[6, 2, 3] = mc[6, 5, 3] = 1.0     # two is_self rows: the lower one
    g = P.gumbel_noise(78, B, N)
    eps = np.random.default_rng(3).standard_normal(B).astype(np.float32)
    ref = P.Ref(P.make_actors(M), R.pack_rows(node, mc, env), ids, g, eps)
    call = P.Call(side, M, node, mc, env, ids, g, eps)
    got = call.run()
    snap = call.out.snap()
    assert call.out.guards_intact(snap)
    for e in range(B):
        assert call.out.row_untouched(snap, e) == (e in (5, 9)), e
    ref.check_scores(got, "%s masks" % side.name)
    ref.check_choice(got, "%s masks" % side.name)
    asked = ref.rows_in
    for k in ("stored", "action", "logp", "charge_mean", "charge_log_std"):
        assert np.isfinite(got[k][asked]).all(), k
    assert not np.isnan(got["node_logp"][asked]).any()
    for e, own in ((1, int(ids[1])), (4, int(ids[4])), (6, 2)):
        assert got["node"][e] == -1 and got["stored"][e, 0] == -1.0 and np.isneginf(got["node_logp"][e]).all(), e
        assert np.array_equal(got["action"][e, :2], mc[e, own, :2]), e
    assert got["node"][0] >= 0 and not dead[got["node"][0]]
    side.close()


def test_emulated_pointer_masks():
    masks_are_selects(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 5. independence
def rows_are_independent(Side):
    side = make_side(Side, 70, B1, M1)
    ids, g, eps, node, mc, env, _ = case(70)
    call, _ = case_call(side, 70)
    call.run()
    first = call.out.snap()
    call.out.fill(); call.run()
    second = call.out.snap()
    assert all(np.array_equal(first[k], second[k]) for k in first)
    base = call.out.arrays(first)
    e, e2 = 5, 77
    ids_b = ((ids + 1) % M1).astype(np.int32); ids_b[e] = ids[e]
    node_b, mc_b, env_b = R.synth_rows(991, B1, 70, M1, ids_b)
    g_b = P.gumbel_noise(992, B1, 70)
    eps_b = np.random.default_rng(8).standard_normal(B1).astype(np.float32)
    for dst, src in ((node_b, node), (mc_b, mc), (env_b, env), (g_b, g), (eps_b, eps)):
        dst[e] = src[e]
    got_b = P.Call(side, M1, node_b, mc_b, env_b, ids_b, g_b, eps_b).run()
    ids_c = ids_b.copy(); ids_c[e2] = ids[e]; ids_c[e] = (ids[e] + 1) % M1
    for dst, src in ((node_b, node), (mc_b, mc), (env_b, env), (g_b, g), (eps_b, eps)):
        dst[e2] = src[e]; dst[e] = src[e2]
    got_c = P.Call(side, M1, node_b, mc_b, env_b, ids_c, g_b, eps_b).run()
    bits = lambda x: np.atleast_1d(x).copy().view(np.uint8)
    for k in P.OUTS:
        assert np.array_equal(bits(base[k][e]), bits(got_b[k][e])), ("other batch", k)
        assert np.array_equal(bits(base[k][e]), bits(got_c[k][e2])), ("other index", k)
    assert not np.array_equal(base["node_logp"][e2], got_b["node_logp"][e2])
    side.close()


def test_emulated_pointer_independence():
    rows_are_independent(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 6. arguments
def bad_arguments_leave_everything_untouched(Side):
    import ctypes as C
    from multi_agent_rl_wrsn_amd import _lib
    side = make_side(Side, 70, B1, M1)
    call, ref = case_call(side, 70)
    call.run()
    want = call.out.snap()
    ent = call.ent.ptrs()
    bad = [dict(actors_ptr=0), dict(agent_ptr=0), dict(node=0), dict(stored=0), dict(action=0), dict(logp=0),
           dict(actors_ptr=R.addr(call.actors) + 4), dict(ent_ptrs=None),
           dict(min_charge=float("nan")), dict(min_charge=-0.1), dict(min_charge=1.0), dict(min_charge=float("inf"))]
    for k in range(3):
        bad.append(dict(ent_ptrs=tuple(0 if j == k else p for j, p in enumerate(ent))))
        bad.append(dict(ent_ptrs=tuple(p + 4 if j == k else p for j, p in enumerate(ent))))

    def out_null():
        h = side.handle
        e = _lib.WrsnEntityOut(*ent)
        _lib.check(h.lib, h.lib.wrsn_entity_pointer_act(h._h, C.c_void_p(R.addr(call.actors)), C.c_void_p(R.addr(call.ids)), None, None, 0.02,
                                                        C.byref(e), None))

    for c in bad + [out_null]:
        call.out.fill()
        before = call.out.snap()
        with pytest.raises(_lib.WrsnError) as ei:
            out_null() if c is out_null else call.run(ent=c.get("ent_ptrs", "own"), **{k: v for k, v in c.items() if k != "ent_ptrs"})
        R.sync(side)
        assert ei.value.code == -1, c
        after = call.out.snap()
        assert all(np.array_equal(before[k], after[k]) for k in before), c
    call.run()
    again = call.out.snap()
    assert all(np.array_equal(want[k], again[k]) for k in want)
    # the optional outputs may be left out
    call.out.fill()
    got = call.run(action_f64=0, node_logp=0, charge_mean=0, charge_log_std=0)
    snap = call.out.snap()
    assert all((snap[k] == R.PATTERN).all() for k in ("action_f64", "node_logp", "charge_mean", "charge_log_std"))
    base = call.out.arrays(want)
    assert all(np.array_equal(got[k], base[k]) for k in ("node", "stored", "action", "logp"))
    side.close()


def test_emulated_pointer_bad_arguments():
    bad_arguments_leave_everything_untouched(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 7. wrsn_entity_act unchanged
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entity_act", "case1.npz")


@pytest.mark.parametrize("N", [70, 33, 257])
def test_emulated_entity_act_is_unchanged(N):
    """wrsn_entity_act on case 1 of tests/test_entity_act.py gives, bit for bit, the bytes recorded from the emulated build of the commit
    before its trunk kernel took the block stride as an argument (tools/gen_entity_act_golden.py)."""
    import test_entity_act as T
    z = np.load(GOLDEN)
    side = T.make_side(EmuSide, N, T.B1, T.M1)
    call, _ = T.case1_call(side, N)
    got = call.run()
    for k in R.OUTS:
        assert got[k].tobytes() == z["n%d_%s" % (N, k)].tobytes(), (N, k)
    side.close()


# ------------------------------------------------------------------------------------------------------------ 8. module
def test_pointer_pack_round_trip_and_layout():
    import torch
    from multi_agent_rl_wrsn_amd import _lib, build_entity_pointer_networks, pack_entity_pointer_actor, unpack_entity_pointer_actor
    from emu_env import emu_lib
    a = P.make_actors(M1)[1]
    blk = pack_entity_pointer_actor(a)
    assert blk.dtype == torch.float32 and blk.numel() == 56980 == int(emu_lib().wrsn_entity_pointer_floats()) == _lib.ENTITY_POINTER_FLOATS
    assert (blk[56978:] == 0).all()
    from test_entity_act import hand_built_block
    trunk = hand_built_block(R.make_actors(M1)[0])             # only to borrow the trunk's offsets: compare layer by layer below
    sd = a.state_dict()
    assert np.array_equal(blk[6208:6208 + 200 * 128].numpy(), sd["trunk.head1.weight"].t().reshape(-1).numpy()) and trunk.size == 49224
    assert np.array_equal(blk[48448:56640].numpy(), sd["query.weight"].t().reshape(-1).numpy())
    assert np.array_equal(blk[56640:56704].numpy(), sd["query.bias"].numpy())
    assert np.array_equal(blk[56704:56976].numpy(), sd["charge.weight"].t().reshape(-1).numpy())
    assert np.array_equal(blk[56976:56978].numpy(), sd["charge.bias"].numpy())
    Actor, _ = build_entity_pointer_networks(M1)
    b = Actor()
    unpack_entity_pointer_actor(blk, b)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in sd.items())
    assert torch.equal(pack_entity_pointer_actor(b), blk)
    fresh = Actor()
    assert float(fresh.query.weight.detach().abs().max()) < 0.05 and float(fresh.charge.weight.detach().abs().max()) < 0.05   # orthogonal, std 0.01


def test_pointer_gradcheck():
    """float64 autograd at N = 5, M = 2, with a row that has no alive node: finite and equal to the numerical gradient."""
    import copy
    import torch
    M, N, n = 2, 5, 3
    ids = np.array([0, 1, 0], np.int32)
    node, mc, env = R.synth_rows(13, n, N, M, ids, p_alive=0.7)
    node[1, :, 7] = 0.0
    node[0, :2, 7] = 1.0; node[2, 3, 7] = 1.0
    rows = torch.from_numpy(R.pack_rows(node, mc, env)).double()
    net = copy.deepcopy(P.make_actors(M)[0]).double()
    with torch.no_grad():
        net.charge.weight[1] *= 0.2                            # log_std strictly inside the clamp: a kink is no place for a numerical gradient
        net.charge.bias[1] += 1.0
    k = torch.tensor([int(np.nonzero(node[0, :, 7])[0][0]), -1, 3])
    x = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    params = [p for p in net.parameters()]
    lp, ent = net(rows, k, x)
    assert torch.isfinite(lp).all() and torch.isfinite(ent).all()
    (lp.sum() + ent.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    # the numerical gradient over x, over the parameters named here in full, and over the first eight output rows of query.weight
    # (1 024 of its 8 192 numbers; every row enters the scores in the same way)
    names = ["charge.weight", "charge.bias", "query.bias", "trunk.node1.weight", "trunk.node2.bias", "trunk.head2.bias"]
    sd = dict(net.named_parameters())
    qw = sd["query.weight"].detach()

    def f(x_, q8, *ps):
        over = dict(zip(names, ps)); over["query.weight"] = torch.cat([q8, qw[8:]], 0)
        return torch.func.functional_call(net, over, (rows, k, x_))

    ins = [x.clone().requires_grad_(True), qw[:8].clone().requires_grad_(True)] + [sd[n].detach().clone().requires_grad_(True) for n in names]
    with torch.no_grad():
        ls = net.charge_head(net.scores(rows)[0], net.scores(rows)[4], k)[1]
    assert ((ls > -3.9) & (ls < 0.9)).all()
    assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-6, rtol=1e-4)
    # every parameter at once: the analytic directional derivative against a central difference along four random directions
    allnames = list(sd)
    base = {n: sd[n].detach().clone() for n in allnames}
    total = lambda ps: sum(o.sum() for o in torch.func.functional_call(net, ps, (rows, k, x)))
    gen = torch.Generator().manual_seed(1)
    for _ in range(4):
        v = {n: torch.randn(base[n].shape, generator=gen, dtype=torch.float64) for n in allnames}
        want = sum((sd[n].grad * v[n]).sum() for n in allnames)
        h = 1e-8                                              # 57 000 numbers move at once: a short step, so that no ReLU or maximum switches
        with torch.no_grad():
            num = (total({n: base[n] + h * v[n] for n in allnames}) - total({n: base[n] - h * v[n] for n in allnames})) / (2 * h)
        assert abs(float(num - want)) <= 1e-4 * max(1.0, abs(float(want))), (float(num), float(want))


def test_pointer_evaluate_reproduces_get_action():
    import torch
    from multi_agent_rl_wrsn_amd import EntityPointerPPOLearner
    torch.set_num_threads(2)
    torch.manual_seed(0)
    lr = EntityPointerPPOLearner(dict(batch_size=48, minibatch_size=8), 2, "cpu", infer_chunk=16)
    for a, src in zip(lr.actors, P.make_actors(2)):
        a.load_state_dict(src.state_dict())
    ids = np.zeros(40, np.int32)
    node, mc, env = R.synth_rows(17, 40, 33, 2, ids)
    node[7, :, 7] = 0.0
    rows = torch.from_numpy(R.pack_rows(node, mc, env))
    stored, lp = lr.get_action(1, rows)
    assert stored.shape == (40, 2) and stored[7, 0] == -1 and len(set(stored[:, 0].tolist())) > 5
    with torch.no_grad():
        new, ent = lr.evaluate(1, rows, stored)
    d = float((new - lp).abs().max())
    print("max |evaluate - get_action logp| %.3g" % d)
    assert d <= 1e-4 and torch.isfinite(ent).all()            # float32 rounding: the CPU bound of tests/test_entity_policy.py
    assert lr.packed_actors().shape == (2, 56980)


# ------------------------------------------------------------------------------------------------------------ 9. trainer
ARGS = dict(batch_size=8, minibatch_size=4, n_updates_per_iteration=1)


def emu_train_env(B=3, M=2):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    side = EmuSide([synth_scenario(300 + e, 70, 60) for e in range(B)], DEFAULT_MC_SPEC, M, map_size=12, render=False, entities=True, auto_reset=True)
    return P.emu_pointer_vec(side)


def fused_roll_out_stores_what_evaluate_recomputes(make_env, device):
    """One roll_out with fused_policy=True: `evaluate` on the stored (state, action) rows at unchanged weights reproduces the stored logp
    within b, b from the module's float32 error on those very rows."""
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO
    torch.set_num_threads(2)
    env = make_env()
    torch.manual_seed(11)
    algo = BatchedEntityPointerIPPO(ARGS, env, device=device, fused_policy=True)
    for a, src in zip(algo.actors, P.make_actors(env.num_agent)):
        a.load_state_dict(src.state_dict())
    algo.roll_out()
    assert algo.buffers.action.shape[-1] == 2 and algo._packed is not None
    for a in range(env.num_agent):
        n = min(int(algo.buffers.count[a]), algo.buffers.capacity)
        assert n >= ARGS["batch_size"]
        st, ac, lp = algo.buffers.state[a, :n], algo.buffers.action[a, :n], algo.buffers.logp[a, :n]
        assert (ac[:, 0] == ac[:, 0].round()).all() and (ac[:, 0] >= -1).all()
        with torch.no_grad():
            new, _ = algo.evaluate(a, st, ac)
            ref, _ = algo.actors[a].double()(st.double(), ac[:, 0].double(), ac[:, 1].double())
            algo.actors[a].float()
        b = 4.0 * float((new.double() - ref).abs().max()) + 1e-6
        d = float((lp.double() - ref).abs().max())
        print("charger %d: %d transitions, |stored - float64| %.3g, b %.3g" % (a, n, d, b))
        assert d <= b, (a, d, b)
    env.side.close() if hasattr(env, "side") else env.close()


def device_action_is_the_stored_decisions_action(make_env, device):
    """With fused_policy the launch takes the device's own 3-vector; `stored_action3`, the PyTorch rule the unfused path uses on what the
    buffers store, gives the same: destinations exactly (both read them from the rows), the charge within float32 rounding of the sigmoid."""
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO
    env = make_env()
    torch.manual_seed(3)
    algo = BatchedEntityPointerIPPO(ARGS, env, device=device, fused_policy=True)
    for a, src in zip(algo.actors, P.make_actors(env.num_agent)):
        a.load_state_dict(src.state_dict())
    algo.buffers.clear(); algo._req = env.reset()
    for _ in range(4):
        r = algo._req
        ids = r["agent_id"].clone()
        stored, logp, handed = algo._choose(r, ids)
        mine = algo.stored_action3(stored)
        assert algo._action3(ids, stored) is handed
        ask = (ids >= 0).cpu()
        assert ask.any()
        assert torch.equal(mine[:, :2].double().cpu()[ask], handed[:, :2].cpu()[ask])
        assert float((mine[:, 2].double().cpu()[ask] - handed[:, 2].cpu()[ask]).abs().max()) <= 1e-6
        algo.step_batch()
    env.side.close() if hasattr(env, "side") else env.close()


def test_emulated_device_action_is_the_stored_decisions_action():
    device_action_is_the_stored_decisions_action(emu_train_env, "cpu")


def test_emulated_fused_roll_out_stores_what_evaluate_recomputes():
    fused_roll_out_stores_what_evaluate_recomputes(emu_train_env, "cpu")


def trainer_trains(make_env, device, fused):
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO
    torch.set_num_threads(2)
    env = make_env()
    torch.manual_seed(5); np.random.seed(5)
    algo = BatchedEntityPointerIPPO(ARGS, env, device=device, fused_policy=fused)
    before = algo.packed_actors().clone()
    rows = algo.train(1)                                       # `train(n)` runs n + 1 iterations
    assert len(rows) == 2 * env.num_agent
    for r in rows:
        assert all(np.isfinite(r[k]) for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac", "mean_reward")), r
    after = algo.packed_actors()
    assert all(not torch.equal(before[a], after[a]) for a in range(env.num_agent))
    env.side.close() if hasattr(env, "side") else env.close()


@pytest.mark.parametrize("fused", [False, True])
def test_emulated_pointer_trainer_trains(fused):
    trainer_trains(emu_train_env, "cpu", fused)


def test_pointer_trainer_refuses_the_fused_update():
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO
    env = emu_train_env()
    for k in ("fused_update", "joint_update", "fused_prepare"):
        with pytest.raises(ValueError, match=k):
            BatchedEntityPointerIPPO(ARGS, env, device="cpu", **{k: True})
    env.side.close()


# ------------------------------------------------------------------------------------------------------------ 10. it cannot stand still
TIME_LIMIT = 250.0      # the mode of the fresh Gaussian actors comes to a stand between 190 s and 240 s of simulated time on these networks


def cannot_stand_still(make_env):
    """Eight 33-node networks of 1 000 J nodes (tests/test_evaluate.py), time_limit 250 s.  Every decision of PointerPolicy(min_charge=0.02)
    spends at least 0.02 * charging_time_max seconds of its charger's time, so an episode holds at most
    ceil(M * time_limit / (0.02 * charging_time_max)) + M + 1 launches: the run ends under that cap.  The mode of fresh Gaussian actors
    hits the same cap with standing rows."""
    import math
    import torch
    from multi_agent_rl_wrsn_amd import EntityPolicy, PointerPolicy, build_entity_pointer_networks, evaluate_policy, pack_entity_pointer_actor
    from multi_agent_rl_wrsn_amd.evaluate import LaunchCapReached
    env = make_env()
    M = env.num_agent
    t_max = float(env._h.env_info()["charging_time_max"].min())
    cap = int(math.ceil(M * TIME_LIMIT / (0.02 * t_max))) + M + 1
    print("charging_time_max %.1f s, cap %d launches" % (t_max, cap))
    assert 100 <= cap < 1000
    from test_evaluate import fresh_actors
    gauss = fresh_actors(env)                                  # the freshly built Gaussian actors tests/test_evaluate.py evaluates
    PA, _ = build_entity_pointer_networks(M)
    pointer = torch.stack([pack_entity_pointer_actor(PA()) for _ in range(M)]).to(env.device).contiguous()
    res = evaluate_policy(env, PointerPolicy(pointer, deterministic=True, min_charge=0.02), 1, time_limit=TIME_LIMIT, max_launches=cap)
    assert int(res["launches"]) < cap and (res["lifetime"] > 0).all()
    print("pointer: %d launches, lifetimes %s" % (int(res["launches"]), res["lifetime"].ravel()))
    with pytest.raises(LaunchCapReached) as ei:
        evaluate_policy(env, EntityPolicy(gauss, deterministic=True), 1, time_limit=TIME_LIMIT, max_launches=cap)
    assert ei.value.result["standing"].sum() > 0
    env.side.close() if hasattr(env, "side") else env.close()


def emu_eval_env(B=2):
    """The first two of the eight networks: the Gaussian run takes `cap` launches by construction, and the emulator runs every block of every
    launch as 256 fibers; the device test runs all eight."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    from test_evaluate import scenarios
    return P.emu_pointer_vec(EmuSide(scenarios(B), DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True, auto_reset=False))


def test_emulated_pointer_cannot_stand_still():
    cannot_stand_still(emu_eval_env)


# ------------------------------------------------------------------------------------------------------------ 11. the comparison tool
def test_emulated_eval_tool_pointer_rows(tmp_path):
    """tools/eval_entity_policy.py --policy pointer on emulated batches (two training and two held-out 33-node networks, two iterations
    of batch 8): the baselines, the four pointer rows and the training record are written, and no pointer row stands still."""
    import importlib.util
    import json
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    from test_evaluate import scenarios
    spec = importlib.util.spec_from_file_location("eval_entity_policy", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools",
                                                                                      "eval_entity_policy.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    made = []

    def make_envs(args):
        tr = P.emu_pointer_vec(EmuSide(scenarios(2, seed=700), DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True, auto_reset=True))
        ev = P.emu_pointer_vec(EmuSide(scenarios(2, seed=800), DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True, auto_reset=False))
        made.extend([tr, ev])
        return tr, ev

    device_envs, tool.device_envs = tool.device_envs, make_envs
    out = str(tmp_path / "eval.json")
    try:
        real = tool.compare
        tool.compare = lambda args: real(args, make_envs)
        tool.main(["--policy", "pointer", "--iters", "2", "--batch-size", "8", "--minibatch-size", "4", "--max-launches", "120", "--out", out])
    finally:
        tool.device_envs, tool.compare = device_envs, real
    res = json.load(open(out))
    assert res["policy"] == "pointer" and res["min_charge"] == 0.02 and res["training"]["iterations"] == 2
    for name in ("uniform", "heuristic", "heuristic_min_charge", "untrained_mode", "untrained_sampled", "trained_mode", "trained_sampled"):
        assert name in res["policies"], name
    for name in ("untrained_mode", "untrained_sampled", "trained_mode", "trained_sampled"):
        row = res["policies"][name]
        assert not row["launch_cap_reached"] and row["episodes"] == 2 and row["lifetime_mean"] > 0, (name, row)
    for env in made:
        env.side.close()
