"""Shared helpers of the lookahead tests (tests/test_lookahead.py on the emulator, tests/test_lookahead_gpu.py on the device): the calls
wrsn_clone_envs_from, wrsn_lookahead_candidates, wrsn_lookahead_collect and wrsn_lookahead_pick on a side, their host references, and
the adapters that let `LookaheadPolicy` reach them on the emulator.

References, all compared by bytes:
  candidates  `ranking` is the header's order in numpy: the alive unclaimed nodes by (score descending, index ascending), then the alive
              claimed ones; `claimed` and the score are the float32 statements of tests/episode_ref.py's `heuristic_ref`.  node,
              sim_agent_id, sim_action (float32 operations, widened; the min_charge clamp in float64), stored[., 0] and every state slot
              come from numpy.  stored[., 1] runs through expf and logf, which are not correctly rounded and differ between a host libm
              and the device (tests/entity_pointer_bc_ref.py holds it to float64 within a bound for that reason), so candidate k's is held,
              by bytes, to wrsn_entity_heuristic_label ON THE SAME SIDE on rows in which the k nodes ranked before it are marked dead:
              there the label's pick IS candidate k.
  collect     `HostLook`: the header's rules as a host loop over the request rows, float64 adds in the same order; the row states are
              what the test knows of the last environment call (tests/episode_ref.py's `RowStates`).
  pick        `pick_ref`: the lexicographic rule over Python floats.
  end to end  `reference_policy`: the lookahead built only from calls that existed before it -- save_envs / load_envs for the fan-out,
              the numpy ranking, entity_heuristic_act, step -- with the bookkeeping in Python."""
import numpy as np

import entity_act_ref as R
import entity_pointer_bc_ref as BC
import entity_train_ref as T
import episode_ref as E
from multi_agent_rl_wrsn_amd import _lib

same = E.same
F64, U8 = _lib.LOOKAHEAD_F64, _lib.LOOKAHEAD_U8
X_CLIP = 4.0


# ------------------------------------------------------------------------------------------------------------ sides
def out_ptrs(side, with_obs=None):
    """Addresses of the request rows (and the observation) the side's environment calls write."""
    return dict(side._ptrs(with_obs) if side.device is None else side.env._out_ptrs())


def req_only(side):
    p = out_ptrs(side, False); p.pop("obs", None)
    return p


def ent_rows(side):
    """(node, mc, env) host copies of the entity rows the side's handle writes."""
    R.sync(side)
    if side.device is None:
        return tuple(a.copy() for a in side.ent.rows(side.ent.snap(), slice(None)))
    return tuple(x.cpu().numpy() for x in (side.env.nodes_feat, side.env.chargers_feat, side.env.env_feat))


def clone_from(dst, src, src_idx, dst_idx, **over):
    """wrsn_clone_envs_from of side `src` into side `dst` through the handles."""
    p = dict(src_handle=src.handle, src_idx=src_idx, dst_idx=dst_idx, src_req=req_only(src))
    p.update(over)
    outs = p.pop("out", None)
    dst.handle.clone_envs_from(p["src_handle"], p["src_idx"], p["dst_idx"], p["src_req"], **(out_ptrs(dst) if outs is None else outs))
    R.sync(dst)


# ------------------------------------------------------------------------------------------------------------ candidates
def row_parts(node, mc, env, a):
    """(self, alive, claimed, score) of one row, as `heuristic_ref` forms them (float32, every operation rounded on its own)."""
    f = np.float32
    N, M = node.shape[0], mc.shape[0]
    with np.errstate(all="ignore"):
        selfs = [o for o in range(M) if mc[o, 3] == f(1)]
        me = selfs[0] if selfs else a
        u, v, w = node[:, 0], node[:, 1], node[:, 2]
        alive = node[:, 7] == f(1)
        claimed = np.zeros(N, bool)
        for o in range(M):
            if o == me or mc[o, 4] != f(1):
                continue
            dx = ((u - mc[o, 6]) / env[0]).astype(f); dy = ((v - mc[o, 7]) / env[1]).astype(f)
            claimed |= ((dx * dx).astype(f) + (dy * dy).astype(f)).astype(f) <= f(1)
        score = np.where(w > f(-np.inf), w, f(-np.inf)).astype(f)
    return me, alive, claimed, score


def ranking(node, mc, env, a):
    """(self, the alive nodes in the heuristic's order): unclaimed first, score descending, index ascending."""
    me, alive, claimed, score = row_parts(node, mc, env, a)
    order = sorted(np.flatnonzero(alive).tolist(), key=lambda n: (bool(claimed[n]), -float(score[n]), n))
    return me, order, claimed


SHAPES = lambda K, B: dict(node=((K, B), np.int32), sim_agent_id=((K, B), np.int32), sim_action=((K, B, 3), np.float64),
                           stored=((K, B, 2), np.float32), t0=((K, B), np.float64), t_end=((K, B), np.float64), last_now=((K, B), np.float64),
                           ret=((K, B), np.float64), survived=((K, B), np.float64), done=((K, B), np.uint8), died=((K, B), np.uint8))


def pattern(shape, dt):
    return np.frombuffer(bytes([T.PATTERN]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()


def candidates_ref(node, mc, env, ids, now, K, horizon, charge_scale=1.0, min_charge=0.0, x_clip=X_CLIP, start=None):
    """What wrsn_lookahead_candidates must leave in buffers that held `start` (default: the fill pattern), but for stored[., 1] of the
    slots with a node, which is NaN here and listed in the returned `x_slots` [(k, e, the nodes ranked before it)]."""
    f = np.float32
    B, M = node.shape[0], mc.shape[1]
    out = {k: pattern(sh, dt) for k, (sh, dt) in SHAPES(K, B).items()} if start is None else {k: v.copy() for k, v in start.items()}
    x_slots = []
    for e in range(B):
        a = int(ids[e])
        if not 0 <= a < M:
            continue
        me, order, _ = ranking(node[e], mc[e], env[e], a)
        for k in range(K):
            valid = k < len(order) or k == 0
            if k < len(order):
                n = order[k]
                c = BC.charge_of(charge_scale, node[e, n, 3:4], f)[0]
                out["node"][k, e] = n; out["sim_agent_id"][k, e] = a
                out["sim_action"][k, e] = (np.float64(node[e, n, 0]), np.float64(node[e, n, 1]), max(np.float64(c), np.float64(min_charge)))
                out["stored"][k, e] = (f(n), f(np.nan))
                x_slots.append((k, e, order[:k]))
            elif k == 0:
                out["node"][k, e] = -1; out["sim_agent_id"][k, e] = a
                out["sim_action"][k, e] = (np.float64(mc[e, me, 0]), np.float64(mc[e, me, 1]), max(np.float64(0), np.float64(min_charge)))
                out["stored"][k, e] = (f(-1), f(-x_clip))
            else:
                out["node"][k, e] = -1; out["sim_agent_id"][k, e] = -2
            out["t0"][k, e] = now[e]; out["t_end"][k, e] = np.float64(now[e]) + np.float64(horizon); out["last_now"][k, e] = now[e]
            out["ret"][k, e] = 0.0; out["died"][k, e] = 0; out["done"][k, e] = 0 if valid else 1
    return out, x_slots


class LookBuf:
    """A wrsn_lookahead_state for K x B slots plus the k-major candidate arrays and the choice arrays, every array between guard bytes
    and pattern-filled, in the side's memory."""

    def __init__(self, side, K, B):
        self.side, self.K, self.B = side, K, B
        self.buf = {k: T.Guarded(side, sh, dt) for k, (sh, dt) in SHAPES(K, B).items()}
        self.next = T.Guarded(side, (K * B,), np.int32)
        self.choice = T.Guarded(side, (B,), np.int32)
        self.action_f64, self.action, self.chosen = T.Guarded(side, (B, 3), np.float64), T.Guarded(side, (B, 3), np.float32), T.Guarded(side, (B, 2), np.float32)
        self.all = list(self.buf.values()) + [self.next, self.choice, self.action_f64, self.action, self.chosen]

    def raw(self, **over):
        f = dict(K=self.K, B=self.B, **{k: self.buf[k].ptr for k in F64 + U8})
        f.update(over)
        return _lib.WrsnLookaheadState(f["K"], f["B"], *(f[k] or None for k in F64 + U8))

    def set(self, **arrays):
        for k, a in arrays.items():
            (self.buf[k] if k in self.buf else getattr(self, k)).set(a)

    def get(self):
        g = {k: b.get() for k, b in self.buf.items()}
        g.update(next=self.next.get(), choice=self.choice.get(), action_f64=self.action_f64.get(), action=self.action.get(), chosen=self.chosen.get())
        return g

    def fill(self):
        for b in self.all:
            b.fill()

    def untouched(self):
        return all(b.untouched() for b in self.all)

    def guards_intact(self):
        return all(b.guards_intact() for b in self.all)


class CandCall:
    """One wrsn_lookahead_candidates on a side: entity rows, ids, now and a LookBuf in the side's memory."""

    def __init__(self, side, node, mc, env, ids, now, K):
        B, N, M = node.shape[0], node.shape[1], mc.shape[1]
        self.side, self.B, self.K = side, B, K
        self.rows = (node, mc, env, np.asarray(ids, np.int32), np.asarray(now, np.float64))
        self.ent = R.EntBuf(B, N, M, device=side.device)
        R.fill_entities(self.ent, node, mc, env)
        self.ids = T.Guarded(side, (B,), np.int32, data=self.rows[3])
        self.now = T.Guarded(side, (B,), np.float64, data=self.rows[4])
        self.look = LookBuf(side, K, B)

    def run(self, horizon=30.0, charge_scale=1.0, min_charge=0.0, x_clip=X_CLIP, ent="own", state="own", **over):
        b = self.look.buf
        p = dict(agent_ptr=self.ids.ptr, now_ptr=self.now.ptr, state=self.look.raw() if isinstance(state, str) else state, horizon=horizon,
                 charge_scale=charge_scale, min_charge=min_charge, x_clip=x_clip, ent_ptrs=self.ent.ptrs() if isinstance(ent, str) else ent,
                 node=b["node"].ptr, sim_agent_id=b["sim_agent_id"].ptr, sim_action=b["sim_action"].ptr, stored=b["stored"].ptr)
        p.update(over)
        self.side.handle.lookahead_candidates(**p)
        R.sync(self.side)
        return self.look.get()

    def label(self, node, charge_scale, min_charge, x_clip):
        """wrsn_entity_heuristic_label and _act of this side on `node` (the call's other rows): (stored, action, action_f64)."""
        _, mc, env, ids, _ = self.rows
        call = BC.LabelCall(self.side, node, mc, env, ids)
        return call.run(charge_scale, min_charge, x_clip), call.heuristic(charge_scale)

    def check(self, horizon=30.0, charge_scale=1.0, min_charge=0.0, x_clip=X_CLIP, tag=""):
        """Run on pattern-filled buffers and hold every byte to the reference; returns (got, want)."""
        node, mc, env, ids, now = self.rows
        self.look.fill()
        got = self.run(horizon, charge_scale, min_charge, x_clip)
        want, x_slots = candidates_ref(node, mc, env, ids, now, self.K, horizon, charge_scale, min_charge, x_clip)
        for k in range(self.K):                               # stored[., 1] of pass k: the label on rows whose k best nodes are dead
            mine = [(e, before) for kk, e, before in x_slots if kk == k]
            if not mine:
                continue
            masked = node.copy()
            for e, before in mine:
                masked[e, before, 7] = 0
            (stored, act, act64), (h_act, h_act64) = self.label(masked, charge_scale, min_charge, x_clip)
            for e, _ in mine:
                assert stored[e, 0] == want["stored"][k, e, 0], (tag, k, e)
                want["stored"][k, e, 1] = stored[e, 1]
                if k == 0:                                    # candidate 0: the heuristic's own bytes, but for the clamp
                    assert same(act64[e], h_act64[e]) and same(act64[e, :2], got["sim_action"][0, e, :2]), (tag, e)
                    assert got["sim_action"][0, e, 2] == max(act64[e, 2], np.float64(min_charge)), (tag, e)
                    if min_charge == 0.0:
                        assert same(got["sim_action"][0, e], h_act64[e]), (tag, e)
        assert self.look.guards_intact() and self.ids.guards_intact() and self.now.guards_intact() and self.ent.guards_intact(self.ent.snap()), tag
        for k in SHAPES(self.K, self.B):
            assert same(got[k], want[k]), (tag, k, got[k], want[k])
        for k in ("next", "choice", "action_f64", "action", "chosen"):
            assert (got[k].view(np.uint8) == T.PATTERN).all(), (tag, k)
        return got, want


# ------------------------------------------------------------------------------------------------------------ collect and pick
class HostLook:
    """The rules of wrsn_lookahead_collect as a host loop (include/wrsn_hip.h) on arrays shaped like the device's, flat over the slots."""

    def __init__(self, arrays, nxt):
        self.a = {k: np.array(arrays[k]).reshape(-1).copy() for k in F64 + U8}
        self.a["next"] = np.array(nxt).reshape(-1).copy()

    def collect(self, states, req, close_all=False):
        a = self.a
        for r in range(len(a["done"])):
            st = int(states.st[r])
            if a["done"][r]:
                a["next"][r] = -2
                continue
            close = False
            if st == 3:
                a["next"][r] = -1
            elif st == 1:
                a["ret"][r] = a["ret"][r] + np.float64(req["reward"][r]); a["last_now"][r] = req["now"][r]
                if req["status"][r] == 1 or req["now"][r] >= a["t_end"][r]:
                    close = True
                else:
                    a["next"][r] = req["agent_id"][r]
            elif st == 4:
                a["died"][r] = 1; a["last_now"][r] = req["now"][r]
                close = True
            if close or close_all:
                a["survived"][r] = min(a["last_now"][r], a["t_end"][r]) - a["t0"][r]
                a["done"][r] = 1; a["next"][r] = -2
        states.consumed()

    def get(self, K, B):
        g = {k: self.a[k].reshape(K, B).copy() for k in F64 + U8}
        g["next"] = self.a["next"].copy()
        return g


def collect(side, look, close_all=False, state="own", nxt="own", req=None, **req_over):
    """One wrsn_lookahead_collect of the LookBuf `look` on the (simulation) side; req: request addresses instead of the side's own."""
    p = dict(req) if req is not None else req_only(side)
    p.update(req_over)
    side.handle.lookahead_collect(look.raw() if isinstance(state, str) else state, look.next.ptr if isinstance(nxt, str) else nxt, close_all, **p)
    R.sync(side)


def pick(side, look, ids_ptr, state="own", **over):
    """One wrsn_lookahead_pick of the LookBuf `look` on the (real) side."""
    b = look.buf
    p = dict(agent_ptr=ids_ptr, state=look.raw() if isinstance(state, str) else state, sim_agent_id=b["sim_agent_id"].ptr, sim_action=b["sim_action"].ptr,
             cand_stored=b["stored"].ptr, choice=look.choice.ptr, action_f64=look.action_f64.ptr, action=look.action.ptr, stored=look.chosen.ptr)
    p.update(over)
    side.handle.lookahead_pick(**p)
    R.sync(side)


def pick_ref(sim_agent_id, done, survived, ret):
    """The slot wrsn_lookahead_pick chooses for one row: arrays [K]."""
    ninf = -np.inf
    best, bs, br = -1, ninf, ninf
    for k in range(len(done)):
        if sim_agent_id[k] < 0 or not done[k]:
            continue
        s = float(survived[k]) if survived[k] > ninf else ninf
        q = float(ret[k]) if ret[k] > ninf else ninf
        if best < 0 or s > bs or (s == bs and q > br):
            best, bs, br = k, s, q
    return max(best, 0)


# ------------------------------------------------------------------------------------------------------------ LookaheadPolicy on the emulator
def emu_look_vec(side):
    """tests/episode_ref.py's adapter plus what `LookaheadPolicy` uses of a VecWRSN: the cross-handle clone and the three lookahead calls,
    as VecWRSN offers them."""
    from multi_agent_rl_wrsn_amd import VecWRSN
    base = type(E.emu_eval_vec(side))

    class EmuLookVec(base):
        def load_envs(self, records, envs=None):
            self.side.load_envs(records.numpy(), envs, with_obs=False); return self._result()

        def clone_envs_from(self, *a, **kw): return VecWRSN.clone_envs_from(self, *a, **kw)
        def new_lookahead(self, *a, **kw): return VecWRSN.new_lookahead(self, *a, **kw)
        def lookahead_candidates(self, *a, **kw): return VecWRSN.lookahead_candidates(self, *a, **kw)
        def lookahead_collect(self, *a, **kw): return VecWRSN.lookahead_collect(self, *a, **kw)
        def lookahead_pick(self, *a, **kw): return VecWRSN.lookahead_pick(self, *a, **kw)

    return EmuLookVec(side)


def sync(env):
    if hasattr(env, "synchronize"):
        env.synchronize()


def reference_policy(env, sim, ids, K, horizon, charge_scale=1.0, min_charge=0.02, max_launches=64):
    """What LookaheadPolicy(sim, K, horizon, ...)(env, ids) must decide, from calls that existed before it: records of `env` loaded into
    `sim` for the fan-out, the numpy ranking on env's entity rows, `entity_heuristic_act` and `step` for the roll-forward, the bookkeeping
    in Python from the request rows.  `sim` runs without a step budget, so a launch answers every slot it is asked.  Returns a dict:
    choice [B], action [B, 3] float64, ret / survived / died / valid [K, B], launches."""
    t = env.torch
    B, M = env.num_env, env.num_agent
    sync(env)
    ids_h = ids.cpu().numpy()
    node, mc, envf = (x.cpu().numpy() for x in (env.nodes_feat, env.chargers_feat, env.env_feat))
    now = env._result()["now"].cpu().numpy().copy()
    want, _ = candidates_ref(node, mc, envf, ids_h, now, K, horizon, charge_scale, min_charge,
                             start={k: np.zeros(sh, dt) for k, (sh, dt) in SHAPES(K, B).items()})
    valid = np.zeros((K, B), bool)
    for e in range(B):
        if 0 <= ids_h[e] < M:
            valid[:, e] = want["sim_agent_id"][:, e] >= 0
    rec = env.save_envs()
    sim.load_envs(t.cat([rec] * K), np.arange(K * B))
    sim_ids = np.where(valid, want["sim_agent_id"], -2).astype(np.int32).reshape(-1)
    act = want["sim_action"].reshape(-1, 3).copy()
    t0 = np.tile(now, K); t_end = t0 + np.float64(horizon); last = t0.copy()
    ret = np.zeros(K * B); died = np.zeros(K * B, bool); done = ~valid.reshape(-1); survived = np.zeros(K * B)
    launches = 0
    while not done.all() and launches < max_launches:
        r = sim.step(t.from_numpy(sim_ids).to(env.device), t.from_numpy(act).to(env.device))
        sync(sim)
        launches += 1
        req = {k: r[k].cpu().numpy().copy() for k in ("agent_id", "reward", "terminal", "now", "status")}
        nxt = np.full(K * B, -2, np.int32)
        for s in np.flatnonzero(sim_ids != -2):
            assert req["status"][s] != 4
            close = False
            if req["terminal"][s]:
                died[s] = True; last[s] = req["now"][s]; close = True
            else:
                ret[s] = ret[s] + np.float64(req["reward"][s]); last[s] = req["now"][s]
                if req["status"][s] == 1 or req["now"][s] >= t_end[s]:
                    close = True
                else:
                    nxt[s] = req["agent_id"][s]
            if close:
                survived[s] = min(last[s], t_end[s]) - t0[s]; done[s] = True
        sim_ids = nxt
        a64 = sim.entity_heuristic_act(t.from_numpy(sim_ids).to(env.device), charge_scale)[1]
        sync(sim)
        act = a64.cpu().numpy().copy()
        act[:, 2] = np.maximum(act[:, 2], min_charge)
    for s in np.flatnonzero(~done):
        survived[s] = min(last[s], t_end[s]) - t0[s]; done[s] = True
    ret, survived, died = ret.reshape(K, B), survived.reshape(K, B), died.reshape(K, B)
    choice = np.zeros(B, np.int32); action = np.zeros((B, 3))
    for e in range(B):
        if 0 <= ids_h[e] < M:
            choice[e] = pick_ref(want["sim_agent_id"][:, e], np.ones(K, bool), survived[:, e], ret[:, e])
            action[e] = want["sim_action"][choice[e], e]
    return dict(choice=choice, action=action, ret=ret, survived=survived, died=died, valid=valid, launches=launches)
