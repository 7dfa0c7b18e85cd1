"""Shared helpers of the joint-update tests (tests/test_entity_update_joint.py on the emulator, tests/test_entity_update_joint_gpu.py on the
device): groups of guarded buffers in a side's memory, the multi-group calls and their single-group reference on them, and the adapter
that lets the trainer reach the multi-group calls on the emulator.

The reference is the single-group calls (wrsn_entity_ppo_grad, wrsn_entity_adam) on the same side, which tests/test_entity_update.py holds
to float64.  Every comparison is bit for bit: `same` compares the bytes."""
import numpy as np

import entity_act_ref as R
import entity_train_ref as T

ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.5)
BLOCKS = ("actor", "critic", "m_actor", "v_actor", "m_critic", "v_critic", "grad_actor", "grad_critic")
_SIZE = dict(actor=T.P_ACTOR, critic=T.P_CRITIC, m_actor=T.P_ACTOR, v_actor=T.P_ACTOR, m_critic=T.P_CRITIC, v_critic=T.P_CRITIC,
             grad_actor=T.P_ACTOR, grad_critic=T.P_CRITIC)
_BATCH = ("action", "logp_old", "advantage", "ret", "value_old")
_DATA = {}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def group_data(g, n_all, N, M):
    """(nets, rows [n_all, R], batch) of group g: its own actor, critic, rows and batch; computed once, never modified."""
    key = (g, n_all, N, M)
    if key not in _DATA:
        actor = R.make_actors(M)[g % M]
        critic = T.make_nets(M, seed=11 + g)[1]
        rows = T.make_rows(100 + 7 * g, n_all, N, M)
        _DATA[key] = ((actor, critic), rows, T.make_batch(100 + 7 * g, rows, actor, critic))
    return _DATA[key]


def nan_rows(rows):
    """Rows of the same shape laden with NaN: in every node, charger and environment slot."""
    bad = rows.copy()
    bad[:, ::3] = np.nan
    bad[:, 1::5] = np.inf
    return bad


class Group:
    """One group in the side's memory: blocks, moments (zero unless given), gradient buffers (pattern-filled), rows and batch, each between
    guard bytes.  `state`: name -> array replaces the initial content of a block, moment or gradient buffer."""

    def __init__(self, side, data, adam_step=0, rows=None, state=None):
        nets, rows0, batch = data
        self.side, self.adam_step = side, int(adam_step)
        init = dict(actor=T.pack(nets[0]), critic=T.pack(nets[1]))
        for k in ("m_actor", "v_actor", "m_critic", "v_critic"):
            init[k] = np.zeros(_SIZE[k], np.float32)
        init.update(state or {})
        self.buf = {k: T.Guarded(side, (_SIZE[k],), data=init.get(k)) for k in BLOCKS}
        rows = rows0 if rows is None else rows
        self.rows = T.Guarded(side, rows.shape, data=rows)
        self.batch = {k: T.Guarded(side, batch[k].shape, data=batch[k]) for k in _BATCH}

    def raw(self, **over):
        """The dict RawHandle._groups takes."""
        q = {k: b.ptr for k, b in self.buf.items()}
        q.update({k: b.ptr for k, b in self.batch.items()})
        q.update(rows=self.rows.ptr, adam_step=self.adam_step)
        q.update(over)
        return q

    def get(self):
        return {k: b.get() for k, b in self.buf.items()}

    def snap(self):
        return [b.snap() for b in self.buf.values()]

    def guards_intact(self):
        return all(b.guards_intact() for b in list(self.buf.values()) + [self.rows] + list(self.batch.values()))


def hyper_of(over=None):
    h = dict(T.HYPER); h.update(over or {})
    return h


# ------------------------------------------------------------------------------------------------ the calls
def grad_multi(side, groups, n, N, M, index, hyper, stats, over=None):
    """wrsn_entity_ppo_grad_multi on `groups`; index: Guarded int32 [G][n] or None; stats: Guarded [G][8].  over: keyword -> value of
    RawHandle.entity_ppo_grad_multi to replace (the bad-argument cases); likewise below."""
    p = dict(groups=[g.raw() for g in groups], n=n, n_node=N, n_mc=M, index=0 if index is None else index.ptr, hyper=hyper, stats=stats.ptr)
    p.update(over or {})
    side.handle.entity_ppo_grad_multi(**p)
    R.sync(side)


def adam_multi(side, groups, adam=ADAM, over=None):
    p = dict(groups=[g.raw() for g in groups], adam=adam)
    p.update(over or {})
    side.handle.entity_adam_multi(**p)
    R.sync(side)


def ppo_update(side, groups, N, M, index, batch_size, minibatch, epochs, hyper, stats, adam=ADAM, over=None):
    """wrsn_entity_ppo_update; index: Guarded int32 [G][epochs][batch_size], stats: Guarded [G][steps][8]."""
    p = dict(groups=[g.raw() for g in groups], n_node=N, n_mc=M, index=index.ptr, batch_size=batch_size, minibatch=minibatch, epochs=epochs,
             hyper=hyper, adam=adam, stats=stats.ptr)
    p.update(over or {})
    side.handle.entity_ppo_update(**p)
    R.sync(side)


def grad_single(side, grp, n, N, M, index, hyper, stats_ptr):
    """wrsn_entity_ppo_grad on one group; index: Guarded int32 [n] or None."""
    p = dict(actor_ptr=grp.buf["actor"].ptr, critic_ptr=grp.buf["critic"].ptr, rows_ptr=grp.rows.ptr, index_ptr=0 if index is None else index.ptr,
             n=n, n_node=N, n_mc=M, grad_actor=grp.buf["grad_actor"].ptr, grad_critic=grp.buf["grad_critic"].ptr, stats=stats_ptr)
    p.update({k: b.ptr for k, b in grp.batch.items()})
    p.update(hyper)
    side.handle.entity_ppo_grad(**p)
    R.sync(side)


def adam_single(side, grp, step, adam=ADAM):
    """wrsn_entity_adam on the actor, then on the critic of one group, at `step`."""
    for w, P in (("actor", T.P_ACTOR), ("critic", T.P_CRITIC)):
        side.handle.entity_adam(grp.buf[w].ptr, grp.buf["grad_" + w].ptr, grp.buf["m_" + w].ptr, grp.buf["v_" + w].ptr, P, step, adam["lr"],
                                adam["beta1"], adam["beta2"], adam["eps"], adam["max_norm"], 0)
    R.sync(side)


def update_single(side, groups, N, M, index, batch_size, minibatch, epochs, hyper, adam=ADAM):
    """The steps of wrsn_entity_ppo_update issued through the single-group calls, group by group within a step; index: numpy int32
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
class EmuJointVec(T.EmuTrainVec):
    """tests/entity_train_ref.py's EmuTrainVec plus the multi-group calls, as VecWRSN offers them: what
    BatchedEntityIPPO(fused_update=True, joint_update=True) uses."""

    def _entity_groups(self, *a):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN._entity_groups(self, *a)

    def _entity_index(self, *a):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN._entity_index(self, *a)

    def entity_ppo_grad_multi(self, *a, **kw):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN.entity_ppo_grad_multi(self, *a, **kw)

    def entity_adam_multi(self, *a, **kw):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN.entity_adam_multi(self, *a, **kw)

    def entity_ppo_update(self, *a, **kw):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN.entity_ppo_update(self, *a, **kw)
