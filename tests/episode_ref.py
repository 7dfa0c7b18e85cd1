"""Shared helpers of the episode tests (tests/test_episodes.py, tests/test_entity_heuristic.py and tests/test_evaluate.py on the emulator,
their `_gpu` modules on the device): the side adapters of wrsn_episodes_collect and wrsn_entity_heuristic_act, the host references and
the adapter that lets `evaluate_policy` and the trainer reach the new calls on the emulator.

References.  The ledger's is `HostLedger`: the rules of include/wrsn_hip.h as a host loop over the request rows the side hands back,
with float64 adds in the same order (one add per request), so every field and every next_agent_id / restart vector is compared bit
for bit.  The row states it goes by are what the test itself knows of the last environment call (`RowStates`): which rows a reset or a
pool swap selected, which rows a step was told to leave alone, and the status / terminal rows of the step.  The heuristic's is
`heuristic_ref`: numpy float32, every operation a numpy float32 operation in the stated order, compared bit for bit as well."""
import numpy as np

import entity_act_ref as R
import entity_train_ref as T
from multi_agent_rl_wrsn_amd import _lib

same = lambda a, b: (np.ascontiguousarray(a).shape == np.ascontiguousarray(b).shape and np.asarray(a).dtype == np.asarray(b).dtype and
                     np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))
NEXT_FILL, RESTART_FILL = -7, 9                               # what next_agent_id / restart hold before the first call
NONE = 0x7fffffff


def log_shapes(B, M, E):
    f8, i4 = np.float64, np.int32
    return dict(run_return=((B, M), f8), run_decisions=((B, M), i4), finished=((B,), i4), dropped=((B,), i4), lifetime=((E, B), f8),
                ep_return=((E, B, M), f8), decisions=((E, B, M), i4), ended=((E, B), i4), record=((E, B), i4))


def req_ptrs(side):
    """Addresses of the request rows the side's environment calls write (no observation)."""
    p = dict(side._ptrs(False) if side.device is None else side.env._out_ptrs())
    p.pop("obs", None)
    return p


class Ledger:
    """A wrsn_episode_log in the side's memory, every array between guard bytes and zeroed, plus next_agent_id / restart vectors."""

    def __init__(self, side, E, quota=0):
        self.side, self.E, self.quota = side, E, quota
        B, M = side.B, side.M
        self.buf = {k: T.Guarded(side, sh, dt, data=np.zeros(sh, dt)) for k, (sh, dt) in log_shapes(B, M, E).items()}
        self.next = T.Guarded(side, (B,), np.int32, data=np.full(B, NEXT_FILL, np.int32))
        self.restart = T.Guarded(side, (B,), np.uint8, data=np.full(B, RESTART_FILL, np.uint8))

    def raw(self, **over):
        f = dict(episodes=self.E, quota=self.quota, **{k: b.ptr for k, b in self.buf.items()})
        f.update(over)
        return _lib.WrsnEpisodeLog(f["episodes"], f["quota"], *(f[k] or None for k in _lib.EPISODE_LOG_ARRAYS))

    def collect(self, time_limit=0.0, consume=True, log="own", next="own", restart="own", req=None, **log_over):
        """One wrsn_episodes_collect; log None: NULL; next / restart: "own", 0 (NULL) or an address; req: request addresses to replace."""
        p = req_ptrs(self.side); p.update(req or {})
        self.side.handle.episodes_collect(self.raw(**log_over) if log == "own" else log, time_limit, self.next.ptr if next == "own" else next,
                                          self.restart.ptr if restart == "own" else restart, consume, **p)
        R.sync(self.side)

    def get(self):
        g = {k: b.get() for k, b in self.buf.items()}
        g.update(next=self.next.get(), restart=self.restart.get())
        return g

    def snap(self):
        return [b.snap() for b in list(self.buf.values()) + [self.next, self.restart]]

    def guards_intact(self):
        return all(b.guards_intact() for b in list(self.buf.values()) + [self.next, self.restart])


class RowStates:
    """What the last environment call did with every row, as the test knows it: 0 untouched / consumed, 1 fresh request, 2 reset or pool
    swap, 3 step in flight, 4 terminal return."""

    def __init__(self, B):
        self.st = np.zeros(B, np.int32)

    def after_reset(self, mask=None):
        self.st = np.full(len(self.st), 2, np.int32) if mask is None else np.where(np.asarray(mask) != 0, 2, 0).astype(np.int32)

    def after_pool_reset(self, mask):
        self.st = np.where(np.asarray(mask) != 0, 2, self.st).astype(np.int32)

    def after_step(self, ids, req):
        ids = np.asarray(ids)
        st = np.where(req["status"] == 4, 3, np.where(req["status"] == 3, 2, np.where(req["terminal"] != 0, 4, 1)))
        self.st = np.where(ids == -2, 0, st).astype(np.int32)

    def consumed(self):
        self.st = np.where(np.isin(self.st, (1, 2, 4)), 0, self.st).astype(np.int32)


class HostLedger:
    """The rules of wrsn_episodes_collect as a host loop (include/wrsn_hip.h), on arrays shaped like the device's."""

    def __init__(self, B, M, E, quota=0, record=True):
        self.B, self.M, self.E, self.quota, self.with_record = B, M, E, quota, record
        self.a = {k: np.zeros(sh, dt) for k, (sh, dt) in log_shapes(B, M, E).items()}
        self.a["next"] = np.full(B, NEXT_FILL, np.int32); self.a["restart"] = np.full(B, RESTART_FILL, np.uint8)

    def collect(self, states, req, time_limit=0.0, record=None, consume=True, next=True, restart=True):
        """states: RowStates (updated when consume); req: the request rows (numpy, by field); record: the pool record per row."""
        a, M = self.a, self.M
        for e in range(self.B):
            st, k = int(states.st[e]), int(a["finished"][e])
            nxt, close = None, 0
            if self.quota > 0 and k >= self.quota:
                nxt = -2
            elif st == 3:
                nxt = -1
            elif st == 2:
                a["run_return"][e] = 0.0; a["run_decisions"][e] = 0
                nxt = int(req["agent_id"][e])
            elif st == 1:
                c = int(req["agent_id"][e])
                if 0 <= c < M:
                    a["run_return"][e, c] = a["run_return"][e, c] + np.float64(req["reward"][e]); a["run_decisions"][e, c] += 1
                if req["status"][e] == 1:
                    close = 3
                elif time_limit > 0 and req["now"][e] >= time_limit:
                    close = 2
                else:
                    nxt = c
            elif st == 4:
                close = 1
            again = 0
            if close:
                if k < self.E:
                    a["lifetime"][k, e] = req["now"][e]; a["ended"][k, e] = close
                    a["ep_return"][k, e] = a["run_return"][e]; a["decisions"][k, e] = a["run_decisions"][e]
                    if self.with_record:
                        a["record"][k, e] = -1 if record is None else record[e]
                else:
                    a["dropped"][e] += 1
                a["finished"][e] = k + 1
                a["run_return"][e] = 0.0; a["run_decisions"][e] = 0
                nxt = -2
                again = 0 if (self.quota > 0 and k + 1 >= self.quota) else 1
            if next and nxt is not None:
                a["next"][e] = nxt
            if restart:
                a["restart"][e] = again
        if consume:
            states.consumed()

    def get(self):
        return {k: v.copy() for k, v in self.a.items()}


def assert_same(got, want, tag, keys=None):
    for k in (keys or want):
        assert same(got[k], want[k]), (tag, k, got[k], want[k])


class Loop:
    """The evaluation loop of `evaluate_policy` on a side, driven by a fixed action script, with the device's ledger and the host's side
    by side: reset, collect, then per launch step, collect, restart the closed rows (reset or pool swap), collect.  Every collect
    compares every field of the log and both vectors bit for bit; `calls` keeps the device's snapshots."""

    def __init__(self, side, E, quota, time_limit, pool_index=None, seed=0):
        self.side, self.time_limit, self.pool_index = side, time_limit, pool_index
        self.led, self.host = Ledger(side, E, quota), HostLedger(side.B, side.M, E, quota)
        self.states = RowStates(side.B)
        self.script = np.random.default_rng(seed)
        self.calls, self.launches, self.seen_states = [], 0, set()

    def collect(self, tag):
        self.seen_states.update(int(s) for s in self.states.st)
        req = self.side._host()
        rec = self.side.pool_info()["record"] if self.pool_index is not None else None
        self.led.collect(self.time_limit)
        self.host.collect(self.states, req, self.time_limit, rec)
        got = self.led.get()
        assert_same(got, self.host.get(), (tag, self.launches))
        assert self.led.guards_intact(), tag
        self.calls.append(got)
        return got

    def start(self):
        self.side.reset(); self.states.after_reset()
        return self.collect("reset")

    def launch(self):
        side = self.side
        ids = self.calls[-1]["next"].copy()
        side.step(ids, self.script.random((side.B, 3))); self.states.after_step(ids, side._host())
        mask = self.collect("step")["restart"]
        if self.pool_index is not None:
            side.pool_reset(mask=mask, index=self.pool_index(self.launches)); self.states.after_pool_reset(mask)
        else:
            side.reset(mask=mask); self.states.after_reset(mask)
        self.launches += 1
        return self.collect("restart")

    def run(self, until, max_launches=400):
        """Launches until until(log) holds."""
        got = self.start()
        while not until(got):
            assert self.launches < max_launches, (self.launches, got["finished"])
            got = self.launch()
        return got


# ------------------------------------------------------------------------------------------------ the heuristic
class BareSide:
    """A handle for B rows of N nodes and M chargers with no scenario, in the memory of `Side` (EmuSide / VecSide): all
    wrsn_entity_heuristic_act needs, at any N."""

    def __init__(self, Side, B, N, M):
        self.B, self.N, self.M, self.name = B, N, M, Side.name
        if Side.name == "emu":
            from emu_env import emu_lib
            lib, self.device = emu_lib(), None
        else:
            from sides import need_gpu
            lib, self.device = _lib.load(), need_gpu().device("cuda:0")
        self.handle = _lib.RawHandle(lib, B, N, 1, M, 12, 1.0, 0)
        self.env = self                                       # what entity_act_ref.sync asks of a device side

    def synchronize(self):
        self.handle.sync()

    def close(self):
        self.handle.close()


def heuristic_ref(node, mc, env, ids, charge_scale, out, out64):
    """wrsn_entity_heuristic_act in numpy float32, statement for statement; writes the rows that are evaluated into out / out64."""
    f = np.float32
    B, N, M = node.shape[0], node.shape[1], mc.shape[1]
    cs = f(charge_scale)
    with np.errstate(all="ignore"):
        for e in range(B):
            a = int(ids[e])
            if not 0 <= a < M:
                continue
            selfs = [o for o in range(M) if mc[e, o, 3] == f(1)]
            me = selfs[0] if selfs else a
            u, v, w = node[e, :, 0], node[e, :, 1], node[e, :, 2]
            alive = node[e, :, 7] == f(1)
            claimed = np.zeros(N, bool)
            for o in range(M):
                if o == me or mc[e, o, 4] != f(1):
                    continue
                dx = ((u - mc[e, o, 6]) / env[e, 0]).astype(f); dy = ((v - mc[e, o, 7]) / env[e, 1]).astype(f)
                claimed |= ((dx * dx).astype(f) + (dy * dy).astype(f)).astype(f) <= f(1)
            score = np.where(w > f(-np.inf), w, f(-np.inf)).astype(f)
            pick = NONE
            for cand in (alive & ~claimed, alive):
                idx = np.nonzero(cand)[0]
                if len(idx):
                    pick = int(idx[np.argmax(score[idx])])       # argmax: the first (lowest-index) maximum
                    break
            if pick != NONE:
                t = f(cs * f(f(1) - node[e, pick, 3]))
                t = (t if t < f(1) else f(1)) if t > f(0) else f(0)
                row = np.array([node[e, pick, 0], node[e, pick, 1], t], f)
            else:
                row = np.array([mc[e, me, 0], mc[e, me, 1], 0], f)
            out[e] = row; out64[e] = row.astype(np.float64)


class HeuristicCall:
    """One wrsn_entity_heuristic_act on a side: entity rows, ids and guarded, pattern-filled outputs in the side's memory."""

    def __init__(self, side, node, mc, env, ids):
        B, N, M = node.shape[0], node.shape[1], mc.shape[1]
        self.side, self.B = side, B
        self.ent = R.EntBuf(B, N, M, device=side.device)
        R.fill_entities(self.ent, node, mc, env)
        self.ids = T.Guarded(side, (B,), np.int32, data=np.asarray(ids, np.int32))
        self.act, self.act64 = T.Guarded(side, (B, 3), np.float32), T.Guarded(side, (B, 3), np.float64)

    def run(self, charge_scale=1.0, ent="own", **over):
        p = dict(agent_ptr=self.ids.ptr, ent_ptrs=self.ent.ptrs() if isinstance(ent, str) else ent, charge_scale=charge_scale,
                 action=self.act.ptr, action_f64=self.act64.ptr)
        p.update(over)
        self.side.handle.entity_heuristic_act(**p)
        R.sync(self.side)
        return self.act.get(), self.act64.get()

    def expected(self, node, mc, env, ids, charge_scale=1.0):
        """The outputs the call must leave: the reference rows over pattern-filled buffers."""
        out = np.frombuffer(bytes([T.PATTERN]) * (self.B * 12), np.float32).reshape(self.B, 3).copy()
        out64 = np.frombuffer(bytes([T.PATTERN]) * (self.B * 24), np.float64).reshape(self.B, 3).copy()
        heuristic_ref(node, mc, env, ids, charge_scale, out, out64)
        return out, out64

    def guards_intact(self):
        return self.ids.guards_intact() and self.act.guards_intact() and self.act64.guards_intact() and self.ent.guards_intact(self.ent.snap())


# ------------------------------------------------------------------------------------------------ evaluate_policy and the trainer on the emulator
def emu_eval_vec(side):
    """tests/sides.py's EmuVec (through the adapter of the prepare tests, which the trainer needs) plus what `evaluate_policy` and
    BatchedEntityIPPO(log_episodes=True) use of a VecWRSN: masked resets, pool swaps and the new calls, as VecWRSN offers them."""
    import entity_prepare_ref as P
    from multi_agent_rl_wrsn_amd import VecWRSN

    class EmuEvalVec(P.EmuPrepareVec):
        scenarios = property(lambda self: self.side.scenarios)
        _pool = property(lambda self: self.side._pool)

        def reset(self, mask=None):
            self.side.reset(None if mask is None else mask.numpy()); return self._result()

        def pool_reset(self, mask=None, index=None):
            self.side.pool_reset(None if mask is None else mask.numpy(), None if index is None else index.numpy()); return self._result()

        def save_envs(self, envs=None):
            return self.torch.from_numpy(self.side.save_envs(envs))

        def set_pool(self, records, seed=0):
            self.side.set_pool(None if records is None else records.numpy(), seed)

        def new_episode_log(self, *a, **kw): return VecWRSN.new_episode_log(self, *a, **kw)
        def episodes_collect(self, *a, **kw): return VecWRSN.episodes_collect(self, *a, **kw)
        def entity_heuristic_act(self, *a, **kw): return VecWRSN.entity_heuristic_act(self, *a, **kw)

    return EmuEvalVec(side)
