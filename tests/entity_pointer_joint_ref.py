"""Shared helpers of the node-pointer joint-update tests (tests/test_entity_pointer_joint.py on the emulator,
tests/test_entity_pointer_joint_gpu.py on the device): groups of guarded buffers in a side's memory, the three multi-group calls
(wrsn_entity_pointer_ppo_grad_multi, wrsn_entity_pointer_adam_multi, wrsn_entity_pointer_ppo_update), their single-group reference on the
same buffers, and the adapter that lets the trainer reach the calls on the emulator.

The reference is the single-group calls (wrsn_entity_pointer_ppo_grad, wrsn_entity_adam on the actor block of 56 980 floats and on the
critic block) on the same side, which tests/test_entity_pointer_update*.py hold to float64.  Every comparison is of bytes (`same`): there
is no tolerance."""
import numpy as np

import entity_act_ref as R
import entity_joint_ref as J
import entity_pointer_train_ref as Q
import entity_train_ref as T

same, ADAM, BLOCKS, hyper_of = J.same, J.ADAM, J.BLOCKS, J.hyper_of
P_ACTOR, P_CRITIC = Q.P_ACTOR, Q.P_CRITIC
_SIZE = dict(actor=P_ACTOR, critic=P_CRITIC, m_actor=P_ACTOR, v_actor=P_ACTOR, m_critic=P_CRITIC, v_critic=P_CRITIC, grad_actor=P_ACTOR,
             grad_critic=P_CRITIC)
_BATCH = ("action", "logp_old", "advantage", "ret", "value_old")        # `action`: the [*, 2] stored pairs
_DATA = {}


def group_data(g, n_all, N, M):
    """(nets, rows [n_all, R], batch) of group g: its own actor (`make_nets` under its own seed) and critic, its own rows and batch;
    computed once, never modified.  The rows hold, through `clamp_rows`, a stored dead node whose features put s_raw beyond the clamp
    (row 0; with four rows or more row 0 below -4 and row 1 above 1), and one row with no alive node, whose stored node is -1 (row 2; the
    last row when there are fewer than four)."""
    key = (g, n_all, N, M)
    if key not in _DATA:
        actor, critic = Q.make_nets(M, seed=23 + g)[0], T.make_nets(M, seed=11 + g)[1]
        seed = 100 + 7 * g
        rows = Q.make_rows(seed, n_all, N, M).copy()
        none_alive = 2 if n_all >= 4 else n_all - 1
        rows[none_alive, 7:8 * N:8] = 0.0
        rows, force = Q.clamp_rows(rows, actor, N, M)
        stored = Q.make_stored(seed, rows, actor, M, force)
        assert stored[none_alive, 0] == -1.0 and all(stored[r, 0] == 0.0 for r in force)
        b = Q.make_batch(seed, rows, stored, actor, critic, M)
        b["action"] = b.pop("stored")
        _DATA[key] = ((actor, critic), rows, b)
    return _DATA[key]


def make_index(G, n, n_all, seed=0):
    """[G][n] int32: per group its own order of n of the n_all rows that keeps the special rows 0, 1, 2 of `group_data` among them; the last
    entry repeats the first where n > 2 (two equal rows have equal advantages, which norm_adv at n = 2 turns into zeros: there the index
    is a plain permutation)."""
    out = []
    for g in range(G):
        r = np.random.default_rng(seed + g)
        if n <= 3:
            out.append(r.permutation(n_all)[:n])
            continue
        body = r.permutation(np.concatenate([np.arange(3), 3 + r.permutation(n_all - 3)[:n - 4]]))
        out.append(np.concatenate([body, body[:1]]))
    return np.stack(out).astype(np.int32)


def nan_like(a):
    """An array of a's shape laden with NaN and infinities."""
    bad = np.array(a, np.float32).reshape(-1).copy()
    bad[::3] = np.nan
    bad[1::5] = np.inf
    return bad.reshape(np.shape(a))


class Group:
    """One group in the side's memory: pointer block, critic block, moments (zero unless given), gradient buffers (pattern-filled), rows
    and batch, each between guard bytes.  `state`: name -> array replaces the initial content of a block, moment or gradient buffer;
    `rows` / `batch`: replace the rows / arrays of the batch."""

    def __init__(self, side, data, adam_step=0, rows=None, state=None, batch=None):
        nets, rows0, batch0 = data
        self.side, self.adam_step = side, int(adam_step)
        init = dict(actor=Q.pack(nets[0]), critic=Q.pack(nets[1]))
        for k in ("m_actor", "v_actor", "m_critic", "v_critic"):
            init[k] = np.zeros(_SIZE[k], np.float32)
        init.update(state or {})
        self.buf = {k: T.Guarded(side, (_SIZE[k],), data=init.get(k)) for k in BLOCKS}
        rows = rows0 if rows is None else rows
        self.rows = T.Guarded(side, rows.shape, data=rows)
        b = dict(batch0); b.update(batch or {})
        self.batch = {k: T.Guarded(side, b[k].shape, data=b[k]) for k in _BATCH}

    raw, get, snap, guards_intact = J.Group.raw, J.Group.get, J.Group.snap, J.Group.guards_intact


# ------------------------------------------------------------------------------------------------ the calls
def grad_multi(side, groups, n, N, M, index, hyper, stats, over=None):
    """wrsn_entity_pointer_ppo_grad_multi on `groups`; index: Guarded int32 [G][n] or None; stats: Guarded [G][8].  over: keyword -> value
    of the RawHandle method to replace (the bad-argument cases); likewise below."""
    p = dict(groups=[g.raw() for g in groups], n=n, n_node=N, n_mc=M, index=0 if index is None else index.ptr, hyper=hyper, stats=stats.ptr)
    p.update(over or {})
    side.handle.entity_pointer_ppo_grad_multi(**p)
    R.sync(side)


def adam_multi(side, groups, adam=ADAM, over=None):
    p = dict(groups=[g.raw() for g in groups], adam=adam)
    p.update(over or {})
    side.handle.entity_pointer_adam_multi(**p)
    R.sync(side)


def ppo_update(side, groups, N, M, index, batch_size, minibatch, epochs, hyper, stats, adam=ADAM, over=None):
    """wrsn_entity_pointer_ppo_update; index: Guarded int32 [G][epochs][batch_size], stats: Guarded [G][steps][8]."""
    p = dict(groups=[g.raw() for g in groups], n_node=N, n_mc=M, index=index.ptr, batch_size=batch_size, minibatch=minibatch, epochs=epochs,
             hyper=hyper, adam=adam, stats=stats.ptr)
    p.update(over or {})
    side.handle.entity_pointer_ppo_update(**p)
    R.sync(side)


def grad_single(side, grp, n, N, M, index, hyper, stats_ptr):
    """wrsn_entity_pointer_ppo_grad on one group; index: Guarded int32 [n] or None."""
    p = dict(actor_ptr=grp.buf["actor"].ptr, critic_ptr=grp.buf["critic"].ptr, rows_ptr=grp.rows.ptr, index_ptr=0 if index is None else index.ptr,
             n=n, n_node=N, n_mc=M, grad_actor=grp.buf["grad_actor"].ptr, grad_critic=grp.buf["grad_critic"].ptr, stats=stats_ptr)
    p.update({("stored" if k == "action" else k): b.ptr for k, b in grp.batch.items()})
    p.update(hyper)
    side.handle.entity_pointer_ppo_grad(**p)
    R.sync(side)


def adam_single(side, grp, step, adam=ADAM):
    """wrsn_entity_adam on the actor block (56 980 floats), then on the critic block of one group, at `step`."""
    for w, P in (("actor", P_ACTOR), ("critic", P_CRITIC)):
        side.handle.entity_adam(grp.buf[w].ptr, grp.buf["grad_" + w].ptr, grp.buf["m_" + w].ptr, grp.buf["v_" + w].ptr, P, step, adam["lr"],
                                adam["beta1"], adam["beta2"], adam["eps"], adam["max_norm"], 0)
    R.sync(side)


def update_single(side, groups, N, M, index, batch_size, minibatch, epochs, hyper, adam=ADAM):
    """The steps of wrsn_entity_pointer_ppo_update issued through the single-group calls, group by group within a step; index: numpy int32
    [G][epochs][batch_size].  Returns the table [G][steps][8]."""
    per_epoch = (batch_size + minibatch - 1) // minibatch
    table = np.zeros((len(groups), epochs * per_epoch, 8), np.float32)
    row = T.Guarded(side, (8,))
    k = 0
    for e in range(epochs):
        for start in range(0, batch_size, minibatch):
            for g, grp in enumerate(groups):
                sl = np.ascontiguousarray(index[g, e, start:start + minibatch])
                grad_single(side, grp, len(sl), N, M, T.Guarded(side, sl.shape, np.int32, data=sl), hyper, row.ptr)
                table[g, k] = row.get()
                adam_single(side, grp, grp.adam_step + 1 + k, adam)
            k += 1
    return table


# ------------------------------------------------------------------------------------------------ the trainer on the emulator
def emu_joint_vec(side):
    """tests/entity_pointer_train_ref.py's adapter plus the multi-group calls and `entity_prepare`, as VecWRSN offers them: what
    BatchedEntityPointerIPPO(device_update=True, joint_update=True, fused_prepare=True) uses on the emulator."""
    from multi_agent_rl_wrsn_amd import VecWRSN
    base = type(Q.emu_update_vec(side))

    class EmuPointerJointVec(base):
        def _entity_groups(self, *a, **kw): return VecWRSN._entity_groups(self, *a, **kw)
        def _entity_index(self, *a): return VecWRSN._entity_index(self, *a)
        def entity_pointer_ppo_grad_multi(self, *a, **kw): return VecWRSN.entity_pointer_ppo_grad_multi(self, *a, **kw)
        def entity_pointer_adam_multi(self, *a, **kw): return VecWRSN.entity_pointer_adam_multi(self, *a, **kw)
        def entity_pointer_ppo_update(self, *a, **kw): return VecWRSN.entity_pointer_ppo_update(self, *a, **kw)
        def entity_prepare(self, *a, **kw): return VecWRSN.entity_prepare(self, *a, **kw)

    return EmuPointerJointVec(side)
