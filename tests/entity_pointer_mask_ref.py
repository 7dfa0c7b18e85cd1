"""Shared helpers of the candidate-mask tests of the node-pointer policy (tests/test_entity_pointer_mask.py on the emulator,
tests/test_entity_pointer_mask_gpu.py on the device): sides whose handle has wrsn_set_entity_pointer_mask(WRSN_POINTER_MASK_CLAIMED) set,
the masked modules, the float32 torch mask, and planted entity rows.

Reference and tolerance are those of tests/entity_pointer_ref.py and tests/entity_pointer_train_ref.py, by import: the module built with
mask_claimed=True in float64 on the CPU, b = 4 * err32 + 1e-6 (a gradient tensor: 4 * err32 + 1e-6 * max|g64|).  The mask itself has no
tolerance: it is formed in float32 by the module (`EntityPointerActor.candidates`) and the kernel's set of finite node_logp equals it."""
import copy

import numpy as np

import entity_act_ref as R
import entity_pointer_ref as P

NONE, CLAIMED = 0, 1
_ACTORS, _PLANTED = {}, {}


def masked(Side, mode=CLAIMED):
    """`Side` with the mode set on every handle it makes: the bodies of the other pointer test modules, which build their own side, run
    under the mask when they are handed this."""
    def make(*a, **kw):
        side = Side(*a, **kw)
        side.handle.set_entity_pointer_mask(mode)
        return side
    return make


def masked_module(actor):
    """A copy of an EntityPointerActor that chooses among candidates (the flag is all `build_entity_pointer_networks(M, True)` adds)."""
    a = copy.deepcopy(actor)
    a.mask_claimed = True
    return a


def masked_actors(M, seed=7):
    """tests/entity_pointer_ref.py's actors -- the weights `P.Call` packs -- with mask_claimed=True; the class is checked to be what
    `build_entity_pointer_networks(M, mask_claimed=True)` builds."""
    key = (M, seed)
    if key not in _ACTORS:
        from multi_agent_rl_wrsn_amd import build_entity_pointer_networks
        assert build_entity_pointer_networks(M, mask_claimed=True)[0]().mask_claimed is True
        assert build_entity_pointer_networks(M)[0]().mask_claimed is False
        _ACTORS[key] = [masked_module(a) for a in P.make_actors(M, seed)]
    return _ACTORS[key]


def torch_mask(node, mc, env):
    """(cand, alive) bool [B, N]: the module's float32 mask of entity arrays node [B,N,8], mc [B,M,12], env [B,8]."""
    import torch
    from multi_agent_rl_wrsn_amd import build_entity_pointer_networks
    Actor = build_entity_pointer_networks(mc.shape[1], mask_claimed=True)[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    alive = t(node)[..., 7] == 1
    return Actor.candidates(alive, t(node), t(mc), t(env)).numpy(), alive.numpy()


def claimed_f32(u, v, cx, cy, hx, hy):
    """The sum the rule compares with 1, in float32, every operation rounded on its own."""
    f = np.float32
    dx, dy = (f(u) - f(cx)) / f(hx), (f(v) - f(cy)) / f(hy)
    return f(dx * dx) + f(dy * dy)


def far_chargers(mc, ids):
    """Every charger alive, is_self on charger ids[e] alone, every destination far outside the field: nobody claims anything yet."""
    mc[..., 4] = 1.0
    mc[..., 3] = 0.0
    for e in range(mc.shape[0]):
        mc[e, int(ids[e]), 3] = 1.0
    mc[..., 6:8] = 50.0
    return mc


def unmasked_pick(node, mc, env, ids, M):
    """The node [B] the unmasked float64 module picks in the mode (P.Ref's f64["node"] without the rest of it)."""
    import torch
    rows, out = R.pack_rows(node, mc, env), np.full(len(ids), -2, np.int64)
    with torch.no_grad():
        for a, actor in enumerate(P.make_actors(M)):
            idx = np.flatnonzero(np.asarray(ids) == a)
            if idx.size:
                net = copy.deepcopy(actor).double()
                _, l, _, alive, _, _, _ = net.scores(torch.from_numpy(rows[idx]).double())
                out[idx] = net.choose(l, alive).numpy()
    return out


def planted_case(N, M, sampled=True, rounds=8):
    """(ids, gumbel, eps, node, mc, env, unmasked float64 mode pick [B]) for test 1 and 2: the rows of test_entity_pointer.case(N, M) with
    every charger alive, each claimer's destination planted on an alive node -- in every second row the first claimer's on the node the
    UNMASKED float64 reference picks in the mode --, and env[0] = env[1] = h chosen per row so that between 10 % and 60 % of the alive
    nodes are claimed.  Destinations and h enter z, so the pick moves with them: plant, re-evaluate, repeat until the picks stand (the
    caller asserts the outcome on the reference alone)."""
    import test_entity_pointer as T
    ids, g, eps, node, mc, env, _ = T.case(N, M, sampled)
    if (N, M) in _PLANTED:
        return (ids, g, eps) + _PLANTED[(N, M)]
    node, mc, env = node.copy(), mc.copy(), env.copy()
    B = node.shape[0]
    rng = np.random.default_rng(1000 + N + M)
    mc[..., 4] = 1.0
    alive = node[..., 7] == 1
    spots = np.stack([rng.choice(np.flatnonzero(alive[e]), M) for e in range(B)])      # [B, M] an alive node per charger
    pick = None
    for _ in range(rounds):
        for e in range(B):
            claimers = [o for o in range(M) if mc[e, o, 3] != 1]
            for j, o in enumerate(claimers):
                k = pick[e] if (pick is not None and e % 2 == 0 and j == 0) else spots[e, o]
                mc[e, o, 6:8] = node[e, k, :2]
        best_gap, best_h = np.full(B, np.inf), np.zeros(B, np.float32)   # h: the grid value whose claimed share is nearest 30 %
        for h in np.linspace(0.04, 0.7, 34, dtype=np.float32):
            env[:, :2] = h
            cand, al = torch_mask(node, mc, env)
            gap = np.abs(1.0 - cand.sum(1) / al.sum(1) - 0.3)
            better = gap < best_gap
            best_gap[better], best_h[better] = gap[better], h
        env[:, :2] = best_h[:, None]
        new = unmasked_pick(node, mc, env, ids, M)
        if pick is not None and np.array_equal(new[::2], pick[::2]):
            break
        pick = new
    _PLANTED[(N, M)] = (node, mc, env, pick)                   # the rows do not depend on `sampled`: computed once, never modified
    return ids, g, eps, node, mc, env, pick


def mask_vec(side):
    """tests/entity_pointer_joint_ref.py's adapter (every call the trainer's options use) plus `set_entity_pointer_mask`, as VecWRSN
    offers it."""
    import entity_pointer_joint_ref as J
    from multi_agent_rl_wrsn_amd import VecWRSN
    base = type(J.emu_joint_vec(side))

    class EmuPointerMaskVec(base):
        def set_entity_pointer_mask(self, mode): return VecWRSN.set_entity_pointer_mask(self, mode)

    return EmuPointerMaskVec(side)
