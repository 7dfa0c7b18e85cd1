"""Shared helpers of the batch-preparation tests (tests/test_entity_prepare.py on the emulator, tests/test_entity_prepare_gpu.py on the
device): groups of guarded buffers in a side's memory, wrsn_entity_prepare on them, its references, and the adapter that lets the
trainer reach the call on the emulator.

References.  The values are wrsn_entity_eval's on the same side for the same rows and block (tests/test_entity_update.py holds them to
float64); advantages and returns are `gae`, the float32 recurrence of include/wrsn_hip.h in numpy -- every operation a numpy float32
operation, hence rounded on its own; the gathers are numpy indexing.  Every comparison is of bytes (`same`): there is no tolerance.
One exception is written down in `same_nan`: WHICH NaN 0 * inf gives is the processor's choice (x86 sets the sign bit, gfx950 does
not), so where the recurrence makes a NaN the test asks for a NaN at the same position and for equal bytes everywhere else."""
import numpy as np

import entity_act_ref as R
import entity_joint_ref as J
import entity_train_ref as T

same = J.same
GAMMA, LAMBDA = 0.99, 0.95
INPUTS = ("critic", "state", "next_state", "reward", "terminal", "action", "logp")
REQUIRED_OUT = ("value", "advantage", "ret")
OPTIONAL_OUT = ("out_state", "out_next_state", "out_action", "out_logp", "out_reward")
OUTPUTS = REQUIRED_OUT + OPTIONAL_OUT
_DATA = {}


def same_nan(a, b):
    """`same`, except that a NaN in `a` matches any NaN in `b` at the same position."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8), b[~nb].view(np.uint8)))


def gae(reward, value, next_value, tm, gamma=GAMMA, gae_lambda=LAMBDA):
    """(advantage, ret) of PPOLearner.cal_rt_adv (gae=True) over float32 arrays in selection order, in the operation order of
    include/wrsn_hip.h."""
    f = np.float32
    g, c = f(gamma), f(np.float64(f(gamma)) * np.float64(f(gae_lambda)))
    n = len(reward)
    adv = np.zeros(n, f)
    last = f(0)
    with np.errstate(all="ignore"):
        for t in range(n - 1, -1, -1):
            delta = f(f(reward[t] + f(f(g * next_value[t]) * tm[t])) - value[t])
            last = f(delta + f(f(c * tm[t]) * last))
            adv[t] = last
        return adv, (adv + value).astype(f)


def group_data(g, n_all, N, M):
    """Group g's inputs over n_all stored transitions: its own critic, state and next_state rows, rewards, bootstrap factors (about 80 %
    ones), actions and log-probabilities; computed once, never modified."""
    key = (g, n_all, N, M)
    if key not in _DATA:
        r = np.random.default_rng(900 + 13 * g)
        f = lambda a: np.ascontiguousarray(a, np.float32)
        _DATA[key] = dict(critic=T.pack(T.make_nets(M, seed=11 + g)[1]), state=T.make_rows(200 + 7 * g, n_all, N, M),
                          next_state=T.make_rows(300 + 7 * g, n_all, N, M), reward=f(r.standard_normal(n_all) * 3.0),
                          terminal=f(r.random(n_all) < 0.8), action=f(r.random((n_all, 3))), logp=f(-r.random(n_all) * 4.0))
    return _DATA[key]


def make_index(G, n, n_all, seed=0):
    """[G][n] int32 into n_all rows, a different draw per group, with a repeat where n > 1 and out of order."""
    idx = np.stack([np.random.default_rng(seed + g).integers(0, n_all, n) for g in range(G)]).astype(np.int32)
    if n > 2:
        idx[:, -1] = idx[:, 0]
    return idx


class Group:
    """One group in the side's memory: every input and every output between guard bytes, outputs pattern-filled.  `over`: name -> array
    replaces an input; `without`: inputs / optional outputs that are not handed to the call (NULL)."""

    def __init__(self, side, data, n, over=None, without=()):
        self.side, self.n, self.without = side, n, tuple(without)
        d = dict(data); d.update(over or {})
        self.data = d
        self.inp = {k: T.Guarded(side, d[k].shape, data=d[k]) for k in INPUTS}
        R_ = d["state"].shape[1]
        shapes = dict(value=(n,), advantage=(n,), ret=(n,), out_state=(n, R_), out_next_state=(n, R_), out_action=(n, 3), out_logp=(n,), out_reward=(n,))
        self.out = {k: T.Guarded(side, shapes[k]) for k in OUTPUTS}

    def raw(self, **over):
        q = {k: b.ptr for k, b in self.inp.items()}
        q.update({k: b.ptr for k, b in self.out.items()})
        for k in self.without:
            q[k] = 0
        q.update(over)
        return q

    def get(self):
        return {k: b.get() for k, b in self.out.items()}

    def snap(self):
        return [b.snap() for b in self.out.values()]

    def untouched(self, keys=OUTPUTS):
        return all(self.out[k].untouched() for k in keys)

    def guards_intact(self):
        return all(b.guards_intact() for b in list(self.inp.values()) + list(self.out.values()))


def prepare(side, groups, n, N, M, index, gamma=GAMMA, gae_lambda=LAMBDA, over=None):
    """wrsn_entity_prepare on `groups`; index: Guarded int32 [G][n] or None.  over: keyword -> value of RawHandle.entity_prepare to replace."""
    p = dict(groups=[g.raw() for g in groups], n=n, n_node=N, n_mc=M, index=0 if index is None else index.ptr, gamma=gamma, gae_lambda=gae_lambda)
    p.update(over or {})
    side.handle.entity_prepare(**p)
    R.sync(side)


def values_of(side, critic, rows, idx, N, M):
    """wrsn_entity_eval's value of rows[idx] (idx None: every row in order) under the block `critic`."""
    n = rows.shape[0] if idx is None else len(idx)
    c, r, v = T.Guarded(side, critic.shape, data=critic), T.Guarded(side, rows.shape, data=rows), T.Guarded(side, (n,))
    i = None if idx is None else T.Guarded(side, (n,), np.int32, data=np.asarray(idx, np.int32))
    side.handle.entity_eval(0, c.ptr, r.ptr, 0 if i is None else i.ptr, n, N, M, 0, 0, v.ptr)
    R.sync(side)
    return v.get()


def expected(side, d, idx, n, N, M, terminal=True, gamma=GAMMA, gae_lambda=LAMBDA):
    """What the call must write for a group with inputs `d` under the selection idx (None: rows 0 .. n - 1): name -> array."""
    sel = np.arange(n) if idx is None else np.asarray(idx)
    v, nv = values_of(side, d["critic"], d["state"], sel, N, M), values_of(side, d["critic"], d["next_state"], sel, N, M)
    tm = d["terminal"][sel] if terminal else np.zeros(n, np.float32)
    adv, ret = gae(d["reward"][sel], v, nv, tm, gamma, gae_lambda)
    return dict(value=v, advantage=adv, ret=ret, out_state=d["state"][sel], out_next_state=d["next_state"][sel], out_action=d["action"][sel],
                out_logp=d["logp"][sel], out_reward=d["reward"][sel])


# ------------------------------------------------------------------------------------------------ the trainer on the emulator
class EmuPrepareVec(J.EmuJointVec):
    """tests/entity_joint_ref.py's EmuJointVec plus `entity_prepare`, as VecWRSN offers it: what BatchedEntityIPPO(fused_prepare=True) uses."""

    def entity_prepare(self, *a, **kw):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN.entity_prepare(self, *a, **kw)
