"""The candidate mask of the node-pointer policy (wrsn_set_entity_pointer_mask, WRSN_POINTER_MASK_CLAIMED; build_entity_pointer_networks(M,
mask_claimed=True); BatchedEntityPointerIPPO / PointerPolicy(mask_claimed=True)) on the emulated library.

The bodies take the side (tests/sides.py): this module runs them on EmuSide, tests/test_entity_pointer_mask_gpu.py on VecSide.  Helpers,
reference and bounds: tests/entity_pointer_mask_ref.py.  Every body sets the mode through the new call."""
import os

import numpy as np
import pytest
from sides import EmuSide

import entity_act_ref as R
import entity_pointer_joint_ref as J
import entity_pointer_mask_ref as K
import entity_pointer_ref as P
import entity_pointer_train_ref as Q
import test_entity_pointer as T
import test_entity_pointer_joint as TJ
import test_entity_pointer_update as U
from test_entity_act import B1, M1, make_side
from test_entity_pointer import SHAPES, case, case_call

bits = lambda x: np.ascontiguousarray(x).view(np.uint8)


def run_mode(call, mode, **kw):
    call.side.handle.set_entity_pointer_mask(mode)
    call.out.fill()
    return call.run(**kw)


def same_outputs(a, b, rows=None):
    return all(np.array_equal(bits(a[k] if rows is None else a[k][rows]), bits(b[k] if rows is None else b[k][rows])) for k in P.OUTS)


# ------------------------------------------------------------------------------------------------------------ 1. mask bits, 2. arithmetic
@pytest.mark.parametrize("N,M", SHAPES)
def test_planted_rows_change_the_decision(N, M):
    """On the reference alone: every claimer's destination sits on an alive node, in every second row on the node the unmasked float64
    reference picks in the mode -- which the mask removes, so the masked reference picks another --, between 10 % and 60 % of every row's
    alive nodes are claimed, and at least 90 % of the rows keep a gap above 2 b between best and runner-up, sampled and mode."""
    ids, g, eps, node, mc, env, pick = K.planted_case(N, M)
    cand, alive = K.torch_mask(node, mc, env)
    share = 1.0 - cand.sum(1) / alive.sum(1)
    print("N=%d M=%d: claimed share of the alive nodes %.2f .. %.2f" % (N, M, share.min(), share.max()))
    assert (share >= 0.1).all() and (share <= 0.6).all()
    assert np.array_equal(pick, K.unmasked_pick(node, mc, env, ids, M))
    for e in range(B1):
        claimers = [o for o in range(M) if mc[e, o, 4] == 1 and mc[e, o, 3] != 1]
        assert len(claimers) == M - 1
        for o in claimers:
            on = np.flatnonzero((node[e, :, :2] == mc[e, o, 6:8]).all(1) & alive[e])
            assert on.size, (e, o)
        if e % 2 == 0:
            assert np.array_equal(mc[e, claimers[0], 6:8], node[e, pick[e], :2]) and not cand[e, pick[e]], e
    for sampled in (True, False):
        ref = masked_ref(N, M, sampled)
        if not sampled:
            assert (ref.f64["node"][::2] != pick[::2]).all()
        sc = ref.perturbed()
        top2 = -np.sort(-sc, axis=1)[:, :2]
        assert ((top2[:, 0] - top2[:, 1]) > 2.0 * ref.b["logits"]).mean() >= 0.9


_REF = {}


def masked_ref(N, M, sampled):
    """P.Ref of the masked float64 / float32 modules on the planted rows: computed once, shared by every test and both sides."""
    key = (N, M, sampled)
    if key not in _REF:
        ids, g, eps, node, mc, env, _ = K.planted_case(N, M, sampled)
        _REF[key] = P.Ref(K.masked_actors(M), R.pack_rows(node, mc, env), ids, g, eps)
    return _REF[key]


def mask_bits_match(Side, N, M):
    """Mode 1: the set {i : node_logp[i] > -inf} of every row equals the float32 torch mask exactly."""
    ids, g, eps, node, mc, env, _ = K.planted_case(N, M)
    cand, alive = K.torch_mask(node, mc, env)
    assert ((cand.sum(1) >= 0.4 * alive.sum(1)) & (cand.sum(1) <= 0.9 * alive.sum(1))).all()      # asserted before the kernel runs
    side = make_side(Side, N, B1, M)
    call = P.Call(side, M, node, mc, env, ids, g, eps)
    got = run_mode(call, K.CLAIMED)
    assert np.array_equal(got["node_logp"] > -np.inf, cand)
    assert not np.isnan(got["node_logp"]).any()
    off = run_mode(call, K.NONE)
    assert np.array_equal(off["node_logp"] > -np.inf, alive)
    side.close()


@pytest.mark.parametrize("N,M", SHAPES)
def test_emulated_mask_bits(N, M):
    mask_bits_match(EmuSide, N, M)


def masked_scores_and_choice_match(Side, N, M, sampled):
    """Scores, node_logp, charge head, logp and action within b of the float64 masked module at the kernel's node; the node is a candidate
    in every row and the reference's arg-max where the gap exceeds 2 b."""
    ids, g, eps, node, mc, env, _ = K.planted_case(N, M, sampled)
    ref = masked_ref(N, M, sampled)
    side = make_side(Side, N, B1, M)
    call = P.Call(side, M, node, mc, env, ids, g, eps)
    got = run_mode(call, K.CLAIMED)
    tag = "%s masked N=%d M=%d %s" % (side.name, N, M, "sampled" if sampled else "mode")
    ref.check_scores(got, tag)
    assert ref.check_choice(got, tag) >= 0.9
    cand, _ = K.torch_mask(node, mc, env)
    assert cand[np.arange(B1), got["node"]].all()
    assert call.out.guards_intact(call.out.snap())
    side.close()


@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("sampled", [True, False])
def test_emulated_masked_scores_and_choice(N, M, sampled):
    masked_scores_and_choice_match(EmuSide, N, M, sampled)


# ------------------------------------------------------------------------------------------------------------ 3. a net-free check
def zero_query_picks_the_first_candidate(Side):
    """query.weight = query.bias = 0: l_i = 0 for every candidate, so with gumbel = NULL the node is the lowest-index alive unclaimed
    node and node_logp is -log(number of candidates) within b."""
    import torch
    from multi_agent_rl_wrsn_amd import pack_entity_pointer_actor
    N, M = 70, M1
    ids, g, eps, node, mc, env, _ = K.planted_case(N, M)
    actors = [K.masked_module(a) for a in P.make_actors(M)]
    with torch.no_grad():
        for a in actors:
            a.query.weight.zero_(); a.query.bias.zero_()
    ref = P.Ref(actors, R.pack_rows(node, mc, env), ids)
    cand, _ = K.torch_mask(node, mc, env)
    side = make_side(Side, N, B1, M)
    call = P.Call(side, M, node, mc, env, ids, None, None)
    call.actors = R.to_side(side, torch.stack([pack_entity_pointer_actor(a) for a in actors]).numpy().copy())
    got = run_mode(call, K.CLAIMED)
    assert np.array_equal(got["node"], np.argmax(cand, 1))
    want = -np.log(cand.sum(1).astype(np.float64))
    dev = np.abs(np.where(cand, got["node_logp"].astype(np.float64) - want[:, None], 0.0)).max()
    print("%s zero query: node_logp deviates from -log(candidates) by %.3g, b %.3g" % (side.name, dev, ref.b["node_logp"]))
    assert dev <= ref.b["node_logp"] and np.isneginf(got["node_logp"][~cand]).all()
    side.close()


def test_emulated_zero_query():
    zero_query_picks_the_first_candidate(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 4. edges, planted
def edge_rows():
    """B = 8, N = 33, M = 3, every request by charger 0, env[0] = env[1] = 0.25, every destination far away, then per row:
    0: claimer 1 exactly at distance 1 (0.25 along u) of alive node 4;  1: the same with the sum the next float above 1;
    2: claimer 1's destination NaN;  3: claimer 1 on node 4 but with slot 4 = 0;  4: the is_self charger on node 4;
    5: env = 10, claimer 1 in the field: every alive node claimed;  6: no alive node;  7: claimer 2 on node 4 (claimed)."""
    B, N, M = 8, 33, 3
    ids = np.zeros(B, np.int32)
    node, mc, env = R.synth_rows(501, B, N, M, ids)
    K.far_chargers(mc, ids)
    env[:, :2] = 0.25
    node[:, 4, 7] = 1.0; node[:, 4, :2] = 0.5; node[:, 4, 2:7] = node[:, 9, 2:7]
    node[:, 9, 7] = 1.0                                        # node 9 alive too; rows where it would sit near node 4 are checked below
    mc[0, 1, 6:8] = (0.75, 0.5)
    mc[1, 1, 6:8] = (0.75, np.float32(0.5) - np.float32(5.0 * 2.0 ** -16))
    mc[2, 1, 6:8] = np.nan
    mc[3, 1, 6:8] = 0.5; mc[3, 1, 4] = 0.0
    mc[4, 0, 6:8] = 0.5
    env[5, :2] = 10.0; mc[5, 1, 6:8] = 0.5
    node[6, :, 7] = 0.0
    mc[7, 2, 6:8] = 0.5
    return ids, node, mc, env


def test_edge_rows_on_the_reference():
    ids, node, mc, env = edge_rows()
    one = np.float32(1.0)
    assert K.claimed_f32(0.5, 0.5, *mc[0, 1, 6:8], 0.25, 0.25) == one
    assert K.claimed_f32(0.5, 0.5, *mc[1, 1, 6:8], 0.25, 0.25) == np.nextafter(one, np.float32(2.0))
    cand, alive = K.torch_mask(node, mc, env)
    assert not cand[0, 4] and cand[0].any() and cand[1, 4]
    for e in (2, 3, 4, 5):
        assert np.array_equal(cand[e], alive[e]) and alive[e].any(), e
    assert not alive[6].any() and not cand[6].any()
    assert not cand[7, 4] and cand[7].any()


def edges_hold(Side):
    """The rows of `edge_rows` under mode 1 against the float32 torch mask, the masked float64 module and mode 0's bytes.  Row 2 is left
    out of every comparison of outputs: a NaN destination of an ALIVE charger also enters that charger's embedding, hence z, and every
    output of the row is NaN-born in kernel and module alike (the node-pointer contract promises nothing for weights or inputs that are
    not finite), so "a NaN claims nothing" cannot be seen through wrsn_entity_pointer_act; test_edge_rows_on_the_reference holds the
    rule's float32 form to it, and the kernel's comparison is the same `<=` of wrsn_eh_claims."""
    ids, node, mc, env = edge_rows()
    B, N, M = node.shape[0], node.shape[1], mc.shape[1]
    cand, alive = K.torch_mask(node, mc, env)
    side = make_side(Side, N, B, M)
    g = P.gumbel_noise(502, B, N)
    eps = np.random.default_rng(503).standard_normal(B).astype(np.float32)
    call = P.Call(side, M, node, mc, env, ids, g, eps)
    off = run_mode(call, K.NONE)
    got = run_mode(call, K.CLAIMED)
    seen = [0, 1, 3, 4, 5, 6, 7]
    assert np.array_equal((got["node_logp"] > -np.inf)[seen], cand[seen])
    assert same_outputs(got, off, [3, 4, 5, 6])                # nothing claimed, everything claimed, nothing alive: the bytes of mode 0
    assert not same_outputs(got, off, [0]) and not same_outputs(got, off, [7])
    assert got["node"][6] == -1 and got["stored"][6, 0] == -1.0 and np.isneginf(got["node_logp"][6]).all()
    assert np.array_equal(got["action"][6, :2], mc[6, 0, :2])
    for k in ("stored", "action", "logp", "charge_mean", "charge_log_std"):
        assert np.isfinite(got[k][seen]).all(), k
    assert not np.isnan(got["node_logp"][seen]).any()
    ids_ref = ids.copy(); ids_ref[2] = -1                      # the reference leaves row 2 out
    ref = P.Ref(K.masked_actors(M), R.pack_rows(node, mc, env), ids_ref, g, eps)
    ref.check_scores(got, "%s edges" % side.name); ref.check_choice(got, "%s edges" % side.name)
    side.close()
    # M = 8: seven claimers, each on an alive node of its own
    B, N, M = 4, 33, 8
    ids = (np.arange(B) % M).astype(np.int32)
    node, mc, env = R.synth_rows(511, B, N, M, ids)
    K.far_chargers(mc, ids)
    env[:, :2] = 0.02
    spots = []
    for e in range(B):
        al = np.flatnonzero(node[e, :, 7] == 1)[:M - 1]
        spots.append(al)
        for o, k in zip([o for o in range(M) if o != ids[e]], al):
            mc[e, o, 6:8] = node[e, k, :2]
    cand, alive = K.torch_mask(node, mc, env)
    assert all(not cand[e, spots[e]].any() and cand[e].any() for e in range(B))
    side = make_side(Side, N, B, M)
    got = run_mode(P.Call(side, M, node, mc, env, ids, P.gumbel_noise(512, B, N), None), K.CLAIMED)
    assert np.array_equal(got["node_logp"] > -np.inf, cand) and cand[np.arange(B), got["node"]].all()
    side.close()


def test_emulated_edges():
    edges_hold(EmuSide)


def claims_across_tiles_keep_ties(Side):
    """N = 257: claimed nodes in tiles 0, 3 (wave 3), 4 (wave 0, second round) and 8 (the ragged last tile); tests/test_entity_pointer.py's
    planted pairs of identical nodes in different tiles and waves still have bit-equal node_logp, and the lower index wins."""
    N, B, M = 257, 8, 3
    ids = (np.arange(B) % M).astype(np.int32)
    node, mc, env = R.synth_rows(91, B, N, M, ids)
    K.far_chargers(mc, ids)
    env[:, :2] = 0.03
    pairs = [(3, 200), (70, 133), (200, 256), (31, 32)]
    g = P.gumbel_noise(92, B, N)
    planted = [5, 100, 130, 255]
    for e in range(B):
        lo, hi = pairs[e % 4]
        node[e, lo, 2:] = node[e, hi, 2:] = node[e, 5, 2:]; node[e, lo, 7] = node[e, hi, 7] = 1.0
        node[e, hi, :2] = node[e, lo, :2]
        g[e, hi] = g[e, lo]
        if e >= 4:
            g[e, lo] = g[e, hi] = 50.0
        claimers = [o for o in range(M) if o != ids[e]]
        for j, k in enumerate(planted):
            node[e, k, 7] = 1.0
        mc[e, claimers[0], 6:8] = node[e, planted[e % 2], :2]; mc[e, claimers[1], 6:8] = node[e, planted[2 + e % 2], :2]
    cand, alive = K.torch_mask(node, mc, env)
    for e in range(B):
        lo, hi = pairs[e % 4]
        assert cand[e, lo] and cand[e, hi] and not cand[e, planted[e % 2]] and not cand[e, planted[2 + e % 2]], e   # on the reference alone
    side = make_side(Side, N, B, M)
    got = run_mode(P.Call(side, M, node, mc, env, ids, g, None), K.CLAIMED)
    assert np.array_equal(got["node_logp"] > -np.inf, cand)
    for e in range(B):
        lo, hi = pairs[e % 4]
        assert got["node_logp"][e, lo].tobytes() == got["node_logp"][e, hi].tobytes(), e
        if e >= 4:
            assert got["node"][e] == lo, (e, got["node"][e])
        else:
            assert got["node"][e] != hi, e
    side.close()


def test_emulated_claims_across_tiles():
    claims_across_tiles_keep_ties(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 5. mode 0 and no-ops, by bytes
def no_op_masks_give_mode_0_bytes(Side):
    """Mode 1 with M = 1, and mode 1 with every other charger dead, give the bytes of mode 0 for all eight outputs; 1 then 0 restores."""
    N = 70
    side = make_side(Side, N, B1, 1)
    ids = np.zeros(B1, np.int32)
    node, mc, env = R.synth_rows(601, B1, N, 1, ids)
    g, eps = P.gumbel_noise(602, B1, N), np.random.default_rng(603).standard_normal(B1).astype(np.float32)
    call = P.Call(side, 1, node, mc, env, ids, g, eps)
    off = run_mode(call, K.NONE)
    assert same_outputs(run_mode(call, K.CLAIMED), off)
    side.close()
    ids, g, eps, node, mc, env, _ = case(N)
    mc = mc.copy()
    mc[..., 4] = np.where(mc[..., 3] == 1, mc[..., 4], 0.0)
    side = make_side(Side, N, B1, M1)
    call = P.Call(side, M1, node, mc, env, ids, g, eps)
    off = run_mode(call, K.NONE)
    assert same_outputs(run_mode(call, K.CLAIMED), off)
    side.close()
    side = make_side(Side, N, B1, M1)
    call, _ = case_call(side, N)
    off = call.run()                                           # the handle's default
    on = run_mode(call, K.CLAIMED)
    assert not same_outputs(on, off)
    assert same_outputs(run_mode(call, K.NONE), off)
    side.close()


def test_emulated_no_op_masks():
    no_op_masks_give_mode_0_bytes(EmuSide)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entity_pointer_act", "case1.npz")


@pytest.mark.parametrize("N", [70, 33, 257])
@pytest.mark.parametrize("touched", [False, True])
def test_emulated_mode_0_is_the_recorded_bytes(N, touched):
    """wrsn_entity_pointer_act with the mask off gives, bit for bit, the bytes recorded from the emulated build of the commit before the
    mask existed (tools/gen_entity_pointer_act_golden.py): on a fresh handle, and after the mode was 1 and is 0 again."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_entity_pointer_act_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools",
                                                                                               "gen_entity_pointer_act_golden.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    z = np.load(GOLDEN)
    side = make_side(EmuSide, N, tool.ROWS, M1)
    call = tool.golden_call(side, N)
    if touched:
        run_mode(call, K.CLAIMED)
    got = run_mode(call, K.NONE) if touched else call.run()
    for k in P.OUTS:
        assert got[k].tobytes() == z["n%d_%s" % (N, k)].tobytes(), (N, k)
    side.close()


# ------------------------------------------------------------------------------------------------------------ 6. independence, determinism, guards
def masked_rows_are_independent(Side):
    """Mode 1: two calls give equal bytes; a row's outputs do not change when the other rows' chargers are NaN-laden or the batch is
    reversed; skipped rows keep every byte; a bad mode is WRSN_ERR_ARG, leaves the mode as it was, and a valid call follows."""
    from multi_agent_rl_wrsn_amd._lib import WrsnError
    N, M = 70, M1
    ids, g, eps, node, mc, env, _ = K.planted_case(N, M)
    ids = ids.copy(); ids[5], ids[9] = -1, M
    side = make_side(Side, N, B1, M)
    call = P.Call(side, M, node, mc, env, ids, g, eps)
    base = run_mode(call, K.CLAIMED)
    snap = call.out.snap()
    assert call.out.guards_intact(snap)
    for e in range(B1):
        assert call.out.row_untouched(snap, e) == (e in (5, 9)), e
    assert same_outputs(run_mode(call, K.CLAIMED), base)
    e = 12
    mc_b = J.nan_like(mc); mc_b[e] = mc[e]
    got_b = run_mode(P.Call(side, M, node, mc_b, env, ids, g, eps), K.CLAIMED)
    assert same_outputs(got_b, base, [e])
    rev = lambda a: np.ascontiguousarray(a[::-1])
    got_c = run_mode(P.Call(side, M, rev(node), rev(mc), rev(env), rev(ids), rev(g), rev(eps)), K.CLAIMED)
    asked = [r for r in range(B1) if r not in (5, 9)]
    assert all(np.array_equal(bits(got_c[k][::-1][asked]), bits(base[k][asked])) for k in P.OUTS)
    for bad in (2, -1, 1 << 20):
        with pytest.raises(WrsnError) as ei:
            side.handle.set_entity_pointer_mask(bad)
        assert ei.value.code == -1
    call.out.fill()
    assert same_outputs(call.run(), base)                      # still mode 1
    assert not same_outputs(run_mode(call, K.NONE), base, asked)
    side.close()


def test_emulated_masked_independence():
    masked_rows_are_independent(EmuSide)


def test_null_handle_is_refused():
    from emu_env import emu_lib
    assert emu_lib().wrsn_set_entity_pointer_mask(None, 1) == -1


# ------------------------------------------------------------------------------------------------------------ 7. eval against act
def masked_eval_reproduces_act(Side):
    """tests/test_entity_pointer_update.py's body under mode 1: eval writes the bytes act writes for node_logp, charge_mean and
    charge_log_std, logp within b.  Then a stored node that is claimed while an unclaimed alive node is there: logp and entropy are the
    float64 masked module's -- the node term is 0."""
    U.eval_reproduces_act(K.masked(Side))
    n, N, M = 8, 70, 3
    ids = np.zeros(n, np.int32)
    node, mc, env = R.synth_rows(701, n, N, M, ids)
    K.far_chargers(mc, ids)
    env[:, :2] = 0.1
    stored = np.zeros((n, 2), np.float32)
    for e in range(n):
        k = int(np.flatnonzero(node[e, :, 7] == 1)[e])
        mc[e, 1 + e % 2, 6:8] = node[e, k, :2]
        stored[e] = (k, 0.1 * e - 0.3)
    cand, alive = K.torch_mask(node, mc, env)
    k = stored[:, 0].astype(int)
    assert alive[np.arange(n), k].all() and not cand[np.arange(n), k].any() and cand.any(1).all()
    rows = R.pack_rows(node, mc, env)
    nets = (K.masked_module(P.make_actors(M)[0]), Q.make_nets(M)[1])
    ref = Q.Ref(nets[0], nets[1], rows, stored, None, Q.HYPER, M)
    t = (stored[:, 1].astype(np.float64) - ref.f64["mean"]) / np.exp(ref.f64["log_std"])
    assert np.abs(ref.f64["logp"] - (-0.5 * t * t - ref.f64["log_std"] - Q.LOG_SQRT_2PI)).max() <= 1e-12      # the reference alone: no node term
    side = make_side(K.masked(Side), N, n, M)
    got = Q.Job(side, nets, rows, None, N, M, stored=stored).eval()
    ref.check_forward(got, "%s claimed stored node" % side.name)
    assert np.array_equal(got["node_logp"] > -np.inf, cand)
    side.close()


def test_emulated_masked_eval():
    masked_eval_reproduces_act(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 8. gradient
# (n, N, M) -> the first seed, counted from the unmasked case's (U.GRAD_CASES), whose float64 kink margins clear 1.5 (8 * err32 + 2e-6) under
# both settings of U.HYPERS and whose err32 is representative (`err32_is_representative`) -- `find_mask_seed`, CPU only; both are asserted
# again in every test
MASK_GRAD_CASES = {(8, 70, 3): 33, (8, 33, 3): 15, (2, 257, 3): 3, (4, 33, 8): 0}
_GRAD = {}


def mask_grad_case(shape, hyper=Q.HYPER, seed=None):
    """(nets, rows, batch, Ref, kinds): tests/entity_pointer_train_ref.py's `case` -- `clamp_rows` included, so s_raw sits beyond the clamp
    on row 0 (and 1) as there -- with the masked actor, and with every input in the range the simulator writes.  The last row has no
    alive node (stored -1).  One row keeps alive only the nodes inside the disc around claimer 1's destination, an alive node's position:
    every alive node is claimed and the candidates are the alive nodes (row n - 2; with fewer than eight rows a clamp row, whose stored node is dead).  With
    four rows or more one row has claimer 1 on the stored ALIVE node while other alive nodes stay unclaimed: no node term (row n - 3 of
    eight, row 2 of four).  With n = 2 there is room for the first two kinds only."""
    n, N, M = shape
    key = (shape, tuple(sorted(hyper.items())), seed)
    if key in _GRAD:
        return _GRAD[key]
    s = MASK_GRAD_CASES[shape] if seed is None else seed
    actor, critic = K.masked_module(Q.make_nets(M)[0]), Q.make_nets(M)[1]
    node, mc, env = U._split(Q.make_rows(s, n, N, M), N, M)
    mc[:, 1, 4] = 1.0
    r_none = n - 1
    r_all = n - 2 if n >= 8 else (1 if n >= 4 else 0)
    r_claim = n - 3 if n >= 8 else (2 if n >= 4 else None)
    node[r_none, :, 7] = 0.0; node[r_none, :, 2:7] = 0.0
    env[r_all, :2] = 0.35                                      # the widest disc of the synthetic rows, around the alive node nearest the centre:
    al = np.flatnonzero(node[r_all, :, 7] == 1)               # as many alive nodes as an all-claimed row can keep
    k_all = int(al[np.argmin(((node[r_all, al, :2] - 0.5) ** 2).sum(1))])
    mc[r_all, 1, 6:8] = node[r_all, k_all, :2]
    inside = np.array([K.claimed_f32(*node[r_all, i, :2], *mc[r_all, 1, 6:8], *env[r_all, :2]) <= 1 for i in range(N)])
    node[r_all, ~inside, 2:] = 0.0                             # dead as the simulator writes a dead node: position kept, zeros elsewhere
    k_claim = None
    if r_claim is not None:
        env[r_claim, :2] = 0.08
        k_claim = int(np.flatnonzero(node[r_claim, :, 7] == 1)[2])
        mc[r_claim, 1, 6:8] = node[r_claim, k_claim, :2]
    rows, force = Q.clamp_rows(R.pack_rows(node, mc, env), actor, N, M)
    node, mc, env = U._split(rows, N, M)
    cand, alive = K.torch_mask(node, mc, env)
    assert not alive[r_none].any() and alive[r_all].any() and np.array_equal(cand[r_all], alive[r_all])
    if r_claim is not None:
        force[r_claim] = k_claim
        assert alive[r_claim, k_claim] and not cand[r_claim, k_claim] and cand[r_claim].any()
    stored = Q.make_stored(s, rows, actor, M, force)
    assert stored[r_none, 0] == -1.0
    batch = Q.make_batch(s, rows, stored, actor, critic, M)
    node, mc, env = U._split(rows, N, M)                     # the same case with the nodes of every row in four other orders
    other = []
    for perm in (np.arange(N)[::-1], np.roll(np.arange(N), 1), np.roll(np.arange(N), N // 2), np.random.default_rng(s).permutation(N)):
        inv = np.argsort(perm)                                 # node perm[j] moves to place j: stored k is found at inv[k]
        st2 = stored.copy(); st2[:, 0] = np.where(stored[:, 0] >= 0, inv[np.maximum(stored[:, 0], 0).astype(int)], stored[:, 0])
        other.append(Q.Ref(actor, critic, R.pack_rows(np.ascontiguousarray(node[:, perm]), mc, env), st2, dict(batch, stored=st2), hyper, M))
    _GRAD[key] = ((actor, critic), rows, batch, Q.Ref(actor, critic, rows, stored, batch, hyper, M), other)
    return _GRAD[key]


def err32_is_representative(ref, other, nets, tag="", share=1.0):
    """On the reference alone.  err32 of a gradient tensor is ONE draw of a float32 rounding error -- for value.b a single number -- and a
    draw can land near zero by luck, which would turn 4 * err32 + 1e-6 max|g64| into a bound that float32 arithmetic in another, equally
    long summation order cannot meet, the module's own included.  `other` holds the same case with the nodes of every row in four other
    orders (reversed, rolled by one, rolled by half, a seeded permutation; a set policy: the gradient of every parameter is the same
    function, the pools and the softmax sum in another order): their float64 gradient is `ref`'s, their float32 gradients are the
    module's own in other orders.  The case is fit when each of them stays within `share` of every tensor's bound.  The tests assert the
    whole bound (share 1: what the module's own arithmetic cannot meet in another order, no kernel can be asked to); the seed search asks
    for half of it, as it asks for one and a half times the kink margins: err32 moves a little from host to host."""
    fit = True
    for j, o in enumerate(other):
        assert all(np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(a).max()) for a, b in zip(ref.g64, o.g64))
        for which, net in ((0, nets[0]), (1, nets[1])):
            for name, sl in Q.block_slices(net).items():
                e, mx = float(np.abs(ref.g32[which][sl] - ref.g64[which][sl]).max()), float(np.abs(ref.g64[which][sl]).max())
                dev = float(np.abs(o.g32[which][sl] - ref.g64[which][sl]).max())
                if dev > share * (4.0 * e + 1e-6 * mx):
                    print("%s %s %s: the float32 module in node order %d deviates by %.3g, err32 %.3g, max|g| %.3g" %
                          (tag, ("actor", "critic")[which], name, j, dev, e, mx))
                    fit = False
    return fit


def find_mask_seed(shape, tries=40):
    """The first seed, from the seed of the unmasked case of tests/test_entity_pointer_update.py on, whose case clears the kink margins one
    and a half times over under both hyper settings (CPU only)."""
    for seed in range(U.GRAD_CASES[shape], U.GRAD_CASES[shape] + tries):
        cases = [mask_grad_case(shape, h, seed) for h in U.HYPERS]
        if all(all(mg > 1.5 * (8.0 * e + 2e-6) for mg, e in c[3].margins.values()) and err32_is_representative(c[3], c[4], c[0], share=0.5) for c in cases):
            return seed
    return None


def masked_gradient_matches(Side, shape, hi):
    """wrsn_entity_pointer_ppo_grad under mode 1: every tensor of both blocks and the statistics against float64 autograd of the masked
    module, under the kink assertion; two calls give equal bytes; mode 0 on the same buffers gives another gradient."""
    n, N, M = shape
    hyper = U.HYPERS[hi]
    nets, rows, batch, ref, other = mask_grad_case(shape, hyper)
    ref.assert_margins(str(shape))
    assert err32_is_representative(ref, other, nets, str(shape))
    side = U.side_for(K.masked(Side), N, M)
    job = Q.Job(side, nets, rows, batch, N, M, hyper=hyper)
    ga, gc, stats = job.grad()
    first = [o.snap() for o in (job.ga, job.gc, job.stats)]
    ref.check_stats(stats, "%s masked %s" % (side.name, shape))
    ref.check_grads(ga, gc, nets, "%s masked %s" % (side.name, shape))
    assert all(o.guards_intact() for o in job.outs)
    job.fill(); job.grad()
    assert all(np.array_equal(a, o.snap()) for a, o in zip(first, (job.ga, job.gc, job.stats)))
    if n >= 4:
        side.handle.set_entity_pointer_mask(K.NONE)
        g0, _, _ = job.grad()
        assert not U.same(g0, ga)
    side.close()


@pytest.mark.parametrize("hi", range(len(U.HYPERS)))
@pytest.mark.parametrize("shape", list(MASK_GRAD_CASES))
def test_emulated_masked_ppo_grad(shape, hi):
    masked_gradient_matches(EmuSide, shape, hi)


def test_masked_gradcheck():
    """float64 autograd of the masked module at N = 6, M = 2 against the numerical gradient, with a claimed stored node, a row where all
    alive nodes are claimed and a row without an alive node."""
    import copy
    import torch
    M, N, n = 2, 6, 3
    ids = np.zeros(n, np.int32)
    node, mc, env = R.synth_rows(13, n, N, M, ids, p_alive=0.7)
    K.far_chargers(mc, ids)
    node[0, :4, 7] = 1.0; node[1, :3, 7] = 1.0; node[2, :, 7] = 0.0
    env[:, :2] = 0.05
    mc[0, 1, 6:8] = node[0, 1, :2]                             # row 0: node 1 claimed, stored
    env[1, :2] = 10.0; mc[1, 1, 6:8] = 0.5                     # row 1: everything claimed
    cand, alive = K.torch_mask(node, mc, env)
    assert not cand[0, 1] and cand[0].any() and np.array_equal(cand[1], alive[1]) and not alive[2].any()
    rows = torch.from_numpy(R.pack_rows(node, mc, env)).double()
    net = K.masked_module(P.make_actors(M)[0]).double()
    with torch.no_grad():
        net.charge.weight[1] *= 0.2; net.charge.bias[1] += 1.0  # log_std strictly inside the clamp
    k = torch.tensor([1, 0, -1])
    x = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    lp, ent = net(rows, k, x)
    plain = copy.deepcopy(net); plain.mask_claimed = False
    lp0, ent0 = plain(rows, k, x)
    assert torch.isfinite(lp).all() and torch.isfinite(ent).all()
    assert lp[0] != lp0[0] and ent[0] != ent0[0] and lp[1] == lp0[1] and ent[1] == ent0[1] and lp[2] == lp0[2]
    names = ["charge.weight", "charge.bias", "query.bias", "trunk.node1.weight", "trunk.node2.bias", "trunk.head2.bias"]
    sd = dict(net.named_parameters())
    qw = sd["query.weight"].detach()

    def f(x_, q8, *ps):
        over = dict(zip(names, ps)); over["query.weight"] = torch.cat([q8, qw[8:]], 0)
        return torch.func.functional_call(net, over, (rows, k, x_))

    ins = [x.clone().requires_grad_(True), qw[:8].clone().requires_grad_(True)] + [sd[n_].detach().clone().requires_grad_(True) for n_ in names]
    assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-6, rtol=1e-4)


# ------------------------------------------------------------------------------------------------------------ 9. joint
def masked_joint_calls_match(Side):
    """wrsn_entity_pointer_ppo_grad_multi at G = 3 and wrsn_entity_pointer_ppo_update (batch 10 / minibatch 4 / two epochs) under mode 1
    give the bytes of the single-group calls under mode 1: the bodies of tests/test_entity_pointer_joint.py on masked handles."""
    TJ.gradient_matches(K.masked(Side), (3, 8, 12, 33, 3, "repeat", 0))
    TJ.update_matches(K.masked(Side))


def test_emulated_masked_joint_calls():
    masked_joint_calls_match(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 10. trainer and policy
ARGS = dict(batch_size=8, minibatch_size=4, n_updates_per_iteration=1)


def emu_train_env():
    return K.mask_vec(T.emu_train_env().side)


def masked_trainer_recomputes_what_acting_stored(make_env, device, fused_policy, device_update, joint=False):
    """BatchedEntityPointerIPPO(mask_claimed=True): on a fresh roll-out the first minibatch of every charger's update shows clipfrac 0 and
    |approx_kl| <= 1e-6: the update recomputes under the mask what acting stored.  The stored rows are checked to hold claimed alive
    nodes, so an update that forgot the mask would see other log-probabilities."""
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO
    torch.set_num_threads(2)
    env = make_env()
    torch.manual_seed(11); np.random.seed(3)
    algo = BatchedEntityPointerIPPO(ARGS, env, device=device, fused_policy=fused_policy, device_update=device_update, joint_update=joint,
                                    fused_prepare=joint, mask_claimed=True)
    assert all(a.mask_claimed for a in algo.actors)
    for a, src in zip(algo.actors, P.make_actors(env.num_agent)):   # weights whose softmax is far from uniform
        a.load_state_dict(src.state_dict())
    first, inner = {}, algo.minibatch_loss

    def minibatch_loss(id, batch, mb):
        res = inner(id, batch, mb)
        first.setdefault(id, (float(res[4]), float(res[5])))
        return res

    algo.minibatch_loss = minibatch_loss
    batches = algo.roll_out()
    met = 0
    for a in range(env.num_agent):
        nd, mcs, ev = U._split(batches[a]["states"].detach().cpu().float().numpy(), env.n_node, env.num_agent)
        cand, alive = K.torch_mask(nd, mcs, ev)
        met += int((cand != alive).any(1).sum())
    print("stored rows with a claimed alive node: %d" % met)
    assert met > 0
    if joint:
        algo.update_all(batches)
    else:
        for a in range(env.num_agent):
            algo.update(a, batches[a])
    for a in range(env.num_agent):
        kl, cf = (algo.first_minibatch_stats[a][4], algo.first_minibatch_stats[a][5]) if device_update else first[a]
        print("charger %d: first minibatch approx_kl %.3g, clipfrac %g" % (a, kl, cf))
        assert cf == 0.0 and abs(kl) <= 1e-6, (a, kl, cf)
    env.side.close() if hasattr(env, "side") else env.close()


@pytest.mark.parametrize("fused_policy", [False, True])
@pytest.mark.parametrize("device_update", [False, True])
def test_emulated_masked_trainer(fused_policy, device_update):
    masked_trainer_recomputes_what_acting_stored(emu_train_env, "cpu", fused_policy, device_update)


def test_emulated_masked_trainer_joint():
    masked_trainer_recomputes_what_acting_stored(emu_train_env, "cpu", True, True, joint=True)


def masked_policy_cannot_stand_still(make_env):
    """PointerPolicy(mask_claimed=True) finishes the episodes of tests/test_entity_pointer.py's `cannot_stand_still` under the same launch
    cap."""
    import math
    import torch
    from multi_agent_rl_wrsn_amd import PointerPolicy, build_entity_pointer_networks, evaluate_policy, pack_entity_pointer_actor
    env = make_env()
    M = env.num_agent
    t_max = float(env._h.env_info()["charging_time_max"].min())
    cap = int(math.ceil(M * T.TIME_LIMIT / (0.02 * t_max))) + M + 1
    PA, _ = build_entity_pointer_networks(M, mask_claimed=True)
    pointer = torch.stack([pack_entity_pointer_actor(PA()) for _ in range(M)]).to(env.device).contiguous()
    res = evaluate_policy(env, PointerPolicy(pointer, deterministic=True, min_charge=0.02, mask_claimed=True), 1, time_limit=T.TIME_LIMIT,
                          max_launches=cap)
    assert int(res["launches"]) < cap and (res["lifetime"] > 0).all()
    print("masked pointer: %d launches, lifetimes %s" % (int(res["launches"]), res["lifetime"].ravel()))
    env.side.close() if hasattr(env, "side") else env.close()


def emu_eval_env():
    return K.mask_vec(T.emu_eval_env().side)


def test_emulated_masked_policy_cannot_stand_still():
    masked_policy_cannot_stand_still(emu_eval_env)
