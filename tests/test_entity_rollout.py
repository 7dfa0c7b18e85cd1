"""Entity transition rows (wrsn_rollout_record_entities / wrsn_rollout_collect_entities, csrc/wrsn_rollout.h) on the emulated library.

The bodies take the side (tests/sides.py): this module runs them on EmuSide, tests/test_entity_rollout_gpu.py on VecSide.  Every
comparison of copied data is exact.  `TrBuf` holds a set of transition buffers with guard bytes on both sides of every array, in the
side's memory; `Mirror` restates the bookkeeping of IPPO.py:137-155 on the host from what the request rows and the entity buffers show
call by call, so the expected content of the buffers is known without a second implementation of the copy."""
import numpy as np
import pytest
from sides import EmuSide

from test_ippo import _policy, reference_bookkeeping

PATTERN, GUARD = 0xA5, 64
FIELDS = ("pend_state", "pend_action", "pend_logp", "pend_valid", "state", "action", "next_state", "reward", "logp", "now", "env", "count")


def row_elems(N, M):
    return 8 * N + 12 * M + 8


class TrBuf:
    """Transition buffers for rows of S floats, `capacity` slots per charger; every array sits between GUARD pattern bytes -- behind it
    `spare` further slots per charger's worth of pattern bytes the library is not told about -- and is pattern-filled, except `count`
    and `pend_valid` (zero)."""

    def __init__(self, side, capacity, S, A=3, spare=0):
        B, M, C = side.B, side.M, capacity
        self.side, self.capacity, self.S, self.A = side, capacity, S, A
        self.spec = {"pend_state": ((B, M, S), np.float32), "pend_action": ((B, M, A), np.float32), "pend_logp": ((B, M), np.float32),
                     "pend_valid": ((B, M), np.uint8), "state": ((M, C, S), np.float32), "action": ((M, C, A), np.float32),
                     "next_state": ((M, C, S), np.float32), "reward": ((M, C), np.float32), "logp": ((M, C), np.float32),
                     "now": ((M, C), np.float64), "env": ((M, C), np.int32), "count": ((M,), np.int32)}
        self.raw, self.nbytes = {}, {}
        for k, (sh, dt) in self.spec.items():
            self.nbytes[k] = int(np.prod(sh)) * np.dtype(dt).itemsize
            per_slot = self.nbytes[k] // C if k in ("state", "action", "next_state", "reward", "logp", "now", "env") else 0
            n = GUARD + self.nbytes[k] + spare * per_slot + GUARD
            if side.device is None:
                buf = np.empty(n + 16, dtype=np.uint8); off = (-buf.ctypes.data) % 16
            else:
                import torch
                buf = torch.empty(n + 16, dtype=torch.uint8, device=side.device); off = (-buf.data_ptr()) % 16
            self.raw[k] = buf[off:off + n]
            self.raw[k][:] = PATTERN
        for k in ("count", "pend_valid"):
            self.raw[k][GUARD:GUARD + self.nbytes[k]] = 0

    def ptr(self, k):
        r = self.raw[k]
        return (r.ctypes.data if isinstance(r, np.ndarray) else r.data_ptr()) + GUARD

    def c(self, **override):
        """The C struct; override: field -> address (0: NULL)."""
        from multi_agent_rl_wrsn_amd import _lib
        p = {k: self.ptr(k) for k in FIELDS}; p.update(override)
        return _lib.WrsnTransitionBuffers(self.capacity, self.A, *[p[k] or None for k in FIELDS])

    def snap(self):
        """Host copies of the raw bytes, guards included."""
        return {k: (r.copy() if isinstance(r, np.ndarray) else r.cpu().numpy()) for k, r in self.raw.items()}

    def arrays(self, snap=None):
        snap = snap or self.snap()
        return {k: snap[k][GUARD:GUARD + self.nbytes[k]].view(dt).reshape(sh) for k, (sh, dt) in self.spec.items()}

    def guards_intact(self, snap):
        """The bytes in front of every array and everything behind it (spare slots, guard) hold the pattern."""
        return all((s[:GUARD] == PATTERN).all() and (s[GUARD + self.nbytes[k]:] == PATTERN).all() for k, s in snap.items())


# ---- what differs between the sides: where arrays live, how the request rows are named
def to_side(side, a):
    """A host array in the side's memory (kept alive by the caller)."""
    a = np.ascontiguousarray(a)
    if side.device is None:
        return a
    import torch
    return torch.from_numpy(a).to(side.device)


def addr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def out_ptrs(side, obs=True, **override):
    if side.device is None:
        p = side._ptrs(obs and side.render)
    else:
        p = side.env._out_ptrs()
        if not obs:
            p["obs"] = 0
    p.update(override)
    return p


def registered(side):
    """Addresses (node, mc, env) of the entity buffers registered on the side's handle."""
    if side.device is None:
        return side.ent.ptrs()
    e = side.env
    return e.nodes_feat.data_ptr(), e.chargers_feat.data_ptr(), e.env_feat.data_ptr()


def entity_rows(side):
    """Packed host rows [B, R] of the registered entity buffers."""
    if side.device is None:
        s = side.ent.snap()
        return np.stack([np.concatenate([x.reshape(-1) for x in side.ent.rows(s, e)]) for e in range(side.B)])
    side.env.synchronize()
    e = side.env
    return np.concatenate([e.nodes_feat.flatten(1).cpu().numpy(), e.chargers_feat.flatten(1).cpu().numpy(), e.env_feat.cpu().numpy()], 1)


def sync(side):
    if side.device is not None:
        side.env.synchronize()


def record(side, buf_c, ids, act, lp, ent=None):
    keep = [to_side(side, np.asarray(ids, np.int32)), to_side(side, np.asarray(act, np.float32)), to_side(side, np.asarray(lp, np.float32))]
    side.handle.rollout_record_entities(buf_c, addr(keep[0]), addr(keep[1]), addr(keep[2]), ent)
    sync(side)


def collect(side, buf_c, ent=None, consume=True, **override):
    side.handle.rollout_collect_entities(buf_c, ent, consume, **out_ptrs(side, **override))
    sync(side)


class Mirror:
    """IPPO.py:137-155 on the host for a batch without a step budget (auto-reset or not): per (environment, charger) the pending row, action
    and log-probability; per charger the appended transitions (env, state, action, logp, reward, next_state, now)."""

    def __init__(self, side):
        self.side = side
        self.pend = [[None] * side.M for _ in range(side.B)]
        self.out = [[] for _ in range(side.M)]

    def record(self, ids, act, lp):
        rows = entity_rows(self.side)
        for e, a in enumerate(ids):
            if a >= 0:
                self.pend[e][a] = (rows[e].copy(), np.asarray(act[e], np.float32).copy(), np.float32(lp[e]))

    def collect(self, stepped):
        """After a step in which the rows of `stepped` were run (to completion: no step budget)."""
        r = self.side._host(); rows = entity_rows(self.side)
        for e in stepped:
            if r["terminal"][e] or r["status"][e] == 3:        # episode over, or restarted by auto-reset: what was pending is dropped
                self.pend[e] = [None] * self.side.M
                continue
            a = int(r["agent_id"][e])
            if a < 0 or self.pend[e][a] is None:
                continue
            s, x, lp = self.pend[e][a]
            self.out[a].append((e, s, x, lp, np.float32(r["reward"][e]), rows[e].copy(), float(r["now"][e])))


def auto_resets(side):
    return side.auto_reset if side.device is None else side.env.auto_reset


def policy_ids(side, done):
    """The request's ids with finished (terminal) environments marked -1 (auto-reset) or -2; actions and log-probabilities of a fixed stand-in policy."""
    r = side._host()
    ids = r["agent_id"].astype(np.int32).copy()
    act = np.zeros((side.B, 3), np.float32); lp = np.zeros(side.B, np.float32)
    for e in range(side.B):
        if r["terminal"][e] or ids[e] < 0:
            ids[e] = -1 if auto_resets(side) else -2          # a finished episode restarts in the step, or is left alone
        else:
            act[e], lp[e] = _policy(e, done[e]); done[e] += 1
    return ids, act, lp


def drive(side, bufs, n_calls, stop=None):
    """n_calls of record / step / collect into every TrBuf of `bufs` (the last one consumes); returns the Mirror."""
    m = Mirror(side); done = [0] * side.B
    side.reset()
    for _ in range(n_calls):
        ids, act, lp = policy_ids(side, done)
        for b in bufs:
            record(side, b.c(), ids, act, lp)
        m.record(ids, act, lp)
        side.step(ids, act.astype(np.float64))
        for k, b in enumerate(bufs):
            collect(side, b.c(), consume=(k == len(bufs) - 1))
        m.collect([e for e in range(side.B) if ids[e] != -2])
        if stop is not None and stop(m):
            break
    return m


def assert_equals_mirror(buf, m, tag=""):
    """Every stored transition is bit for bit the mirror's with the same (env, now, logp); counts equal; unreached slots keep the pattern."""
    snap = buf.snap(); a_ = buf.arrays(snap)
    assert buf.guards_intact(snap), tag
    for a in range(buf.side.M):
        n = int(a_["count"][a]); want = m.out[a]
        assert n == len(want), (tag, a, n, len(want))
        k = min(n, buf.capacity)
        got = sorted(range(k), key=lambda q: (a_["env"][a, q], a_["now"][a, q], a_["logp"][a, q]))
        if n <= buf.capacity:
            ref = sorted(want, key=lambda t: (t[0], t[6], t[3]))
        else:                                                  # which k of the n are stored is the order of arrival: match by key
            keyed = {(t[0], t[6], float(t[3])): t for t in want}
            assert len(keyed) == len(want)
            ref = [keyed[(int(a_["env"][a, q]), float(a_["now"][a, q]), float(a_["logp"][a, q]))] for q in got]
        for q, t in zip(got, ref):
            assert a_["env"][a, q] == t[0] and a_["now"][a, q] == t[6] and a_["logp"][a, q] == t[3], (tag, a, q)
            assert np.array_equal(a_["state"][a, q].view(np.uint32), t[1].view(np.uint32)), (tag, a, q, "state")
            assert np.array_equal(a_["action"][a, q], t[2]) and a_["reward"][a, q] == t[4], (tag, a, q)
            assert np.array_equal(a_["next_state"][a, q].view(np.uint32), t[5].view(np.uint32)), (tag, a, q, "next_state")
        for name in ("state", "next_state", "action", "reward", "logp", "now", "env"):     # slots no transition reached
            rest = np.ascontiguousarray(a_[name][a, k:]).view(np.uint8)
            assert (rest == PATTERN).all(), (tag, a, name)
    return a_


# ------------------------------------------------------------------------------------------------------------ 1. bookkeeping
def bookkeeping_equals_the_reference_lists(Side):
    """The body of test_emulated_transition_buffers_equal_the_reference_bookkeeping (tests/test_ippo.py) on entity rows: a batch with
    auto-reset and a step budget == the reference's per-environment lists on single environments, whose states are wrsn_entities rows
    packed the same way.  N = 70: R = 592 floats, 148 chunks -- more than two 64-chunk strides of a wave and not a multiple of 64."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    B, M, CAP, K = 3, 2, 64, 28
    scs = [synth_scenario(300 + e, 70, 60) for e in range(B)]
    side = Side(scs, DEFAULT_MC_SPEC, M, map_size=12, render=False, entities=True, step_budget=60, auto_reset=True)
    R = row_elems(side.N, M)
    assert R == 592
    buf = TrBuf(side, CAP, R)
    side.reset()
    n_dec = np.zeros(B, dtype=int)
    for it in range(400):
        r = side._host()
        ids = r["agent_id"].astype(np.int32).copy()
        act = np.zeros((B, 3), np.float32); lp = np.zeros(B, np.float32)
        for e in range(B):
            if ids[e] >= 0 and n_dec[e] < K:
                act[e], lp[e] = _policy(e, n_dec[e]); n_dec[e] += 1
            elif ids[e] >= 0:
                ids[e] = -2                                    # this environment has had its K decisions
        record(side, buf.c(), ids, act, lp)
        side.step(ids, act.astype(np.float64))
        collect(side, buf.c())
        if (n_dec >= K).all() and not (side._host()["status"] == 4).any():
            break
    snap = buf.snap(); arrs = buf.arrays(snap)
    assert buf.guards_intact(snap)
    side.close()
    want = [[] for _ in range(M)]
    for e in range(B):
        one = Side([scs[e]], DEFAULT_MC_SPEC, M, map_size=12, render=False)
        eb = one.entity_buffers()

        def req(one=one, eb=eb, e=e):
            r = one._host()
            a = int(r["agent_id"][0]); state = None
            if a >= 0:
                one.entities([a], eb)
                state = np.concatenate([x.reshape(-1) for x in eb.rows(eb.snap(), 0)]).copy()
            return dict(agent_id=a, state=state, reward=float(r["reward"][0]), terminal=bool(r["terminal"][0]), now=float(r["now"][0]),
                        policy=lambda n, e=e: _policy(e, n))

        def reset(one=one, req=req):
            one.reset(); return req()

        def step(a, action, one=one, req=req):
            one.step([a], np.asarray(action, np.float64)[None]); return req()
        per_agent = reference_bookkeeping(step, reset, M, K)
        for a in range(M):
            want[a] += [(e,) + t for t in per_agent[a]]
        one.close()
    for a in range(M):
        n = int(arrs["count"][a])
        assert n == len(want[a]) and 0 < n <= CAP
        got = sorted(range(n), key=lambda q: (arrs["env"][a, q], arrs["now"][a, q], arrs["logp"][a, q]))
        ref = sorted(want[a], key=lambda t: (t[0], t[6], t[3]))
        for q, t in zip(got, ref):
            assert arrs["env"][a, q] == t[0] and arrs["now"][a, q] == t[6]
            assert np.array_equal(arrs["state"][a, q].view(np.uint32), t[1].view(np.uint32)) and np.array_equal(arrs["action"][a, q], t[2])
            assert arrs["logp"][a, q] == t[3] and arrs["reward"][a, q] == np.float32(t[4])
            assert np.array_equal(arrs["next_state"][a, q].view(np.uint32), t[5].view(np.uint32))


def test_emulated_entity_transition_buffers_equal_the_reference_bookkeeping():
    bookkeeping_equals_the_reference_lists(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 2. ragged and large rows
def ragged_rows_arrive_whole(Side):
    """One handle with a 33-node and a 70-node network: the zero rows beyond an environment's own n_node arrive in state and next_state."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(411, 33, 17), synth_scenario(412, 70, 60)]
    side = Side(scs, DEFAULT_MC_SPEC, 2, map_size=12, render=False, entities=True)
    buf = TrBuf(side, 32, row_elems(side.N, 2))
    m = drive(side, [buf], 10)
    a_ = assert_equals_mirror(buf, m, "ragged")
    seen = 0
    for a in range(2):
        for q in range(int(a_["count"][a])):
            if a_["env"][a, q] == 0:
                for name in ("state", "next_state"):
                    nodes = a_[name][a, q][:8 * 70].reshape(70, 8)
                    assert (nodes[33:].view(np.uint32) == 0).all() and nodes[:33, 7].any() and a_[name][a, q][-3] == 33.0
                seen += 1
    assert seen > 0
    side.close()


def large_rows_arrive_whole(Side):
    """Two (257, 129) environments, 3 chargers, six calls: rows of 8.4 KB, 525 chunks -- a second pass of the wave with a ragged end."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(421 + e, 257, 129) for e in range(2)]
    side = Side(scs, DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True)
    R = row_elems(257, 3)
    assert R // 4 == 525
    buf = TrBuf(side, 16, R)
    m = drive(side, [buf], 6)
    a_ = assert_equals_mirror(buf, m, "large")
    assert int(a_["count"].sum()) > 0
    side.close()


def test_emulated_ragged_entity_rows():
    ragged_rows_arrive_whole(EmuSide)


def test_emulated_large_entity_rows():
    large_rows_arrive_whole(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 3. extent
def extent_is_respected(Side):
    """capacity 4 with two spare slots per charger behind every array, more than 4 transitions per charger: count runs past 4, slots 0..3 are written, the spare slots,
    the guards and everything else keep their bytes; a record whose agent_id is all -2 writes nothing."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(300 + e, 70, 60) for e in range(3)]
    side = Side(scs, DEFAULT_MC_SPEC, 2, map_size=12, render=False, entities=True, auto_reset=True)
    buf = TrBuf(side, 4, row_elems(side.N, 2), spare=2)
    m = drive(side, [buf], 40, stop=lambda m: min(len(o) for o in m.out) > 4)
    a_ = assert_equals_mirror(buf, m, "extent")
    assert (a_["count"] > 4).all()
    for a in range(2):
        for name in ("state", "next_state"):
            assert not (a_[name][a, :4].view(np.uint32) == PATTERN * 0x01010101).any()       # no 4-byte slot of a stored row keeps the pattern
    before = buf.snap()
    record(side, buf.c(), np.full(3, -2, np.int32), np.ones((3, 3), np.float32), np.ones(3, np.float32))
    after = buf.snap()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    side.close()


def test_emulated_entity_rows_extent():
    extent_is_respected(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 4. consume
def consume_feeds_both_kinds_of_buffers(Side):
    """With the image on: entity collect with consume = 0, then the image collect -- both buffers hold the same multiset of
    (env, now, reward) per charger; a second entity collect with consume = 1 after a consuming one appends nothing."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    B, M, G = 3, 2, 12
    scs = [synth_scenario(300 + e, 70, 60) for e in range(B)]
    side = Side(scs, DEFAULT_MC_SPEC, M, map_size=G, render=True, entities=True, auto_reset=True)
    ent = TrBuf(side, 64, row_elems(side.N, M)); img = TrBuf(side, 64, 4 * G * G)
    obs_ptr = out_ptrs(side)["obs"]
    assert obs_ptr
    done = [0] * B
    side.reset()
    for _ in range(12):
        ids, act, lp = policy_ids(side, done)
        record(side, ent.c(), ids, act, lp)
        keep = [to_side(side, ids), to_side(side, act), to_side(side, lp)]
        side.handle.rollout_record(img.c(), addr(keep[0]), addr(keep[1]), addr(keep[2]), obs_ptr); sync(side)
        side.step(ids, act.astype(np.float64))
        collect(side, ent.c(), consume=False)
        side.handle.rollout_collect(img.c(), **out_ptrs(side)); sync(side)
    e_, i_ = ent.arrays(), img.arrays()
    assert np.array_equal(e_["count"], i_["count"]) and (e_["count"] > 0).all()
    for a in range(M):
        n = int(e_["count"][a])
        key = lambda x: sorted(zip(x["env"][a, :n].tolist(), x["now"][a, :n].tolist(), x["reward"][a, :n].tolist()))
        assert key(e_) == key(i_)
    # a consuming collect, then a second one after the same launch
    ids, act, lp = policy_ids(side, done)
    record(side, ent.c(), ids, act, lp)
    side.step(ids, act.astype(np.float64))
    collect(side, ent.c(), consume=True)
    first = ent.snap()
    assert int(ent.arrays(first)["count"].sum()) > int(e_["count"].sum())
    collect(side, ent.c(), consume=True)
    second = ent.snap()
    assert all(np.array_equal(first[k], second[k]) for k in first)
    side.close()


def test_emulated_entity_collect_consume():
    consume_feeds_both_kinds_of_buffers(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 5. arguments
def bad_arguments_leave_everything_untouched(Side):
    """Every WRSN_ERR_ARG case of the two calls leaves the buffers as they were and the requests unconsumed: the valid collect that
    follows still appends what the mirror expects.  out->obs == NULL is accepted (it is NULL throughout); an explicit `ent` equal to the
    registered buffers gives the same transitions as NULL (the same bytes, slot order within a charger's list apart)."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, _lib, synth_scenario
    scs = [synth_scenario(300 + e, 70, 60) for e in range(3)]
    side = Side(scs, DEFAULT_MC_SPEC, 2, map_size=12, render=False, entities=True, auto_reset=True)
    R = row_elems(side.N, 2)
    buf = TrBuf(side, 32, R); twin = TrBuf(side, 32, R)
    reg = registered(side)
    assert out_ptrs(side)["obs"] == 0

    def refused(call):
        before = buf.snap()
        with pytest.raises(_lib.WrsnError) as ei:
            call()
        sync(side)
        assert ei.value.code == -1
        after = buf.snap()
        assert all(np.array_equal(before[k], after[k]) for k in before)

    def bad_ents():
        for k in range(3):
            yield tuple(0 if j == k else p for j, p in enumerate(reg))
            yield tuple(p + 4 if j == k else p for j, p in enumerate(reg))

    def bad_bufs():
        for k in ("pend_state", "state", "next_state"):
            yield buf.c(**{k: 0})
            yield buf.c(**{k: buf.ptr(k) + 4})

    m = Mirror(side); done = [0] * side.B
    side.reset()
    for call in range(8):
        ids, act, lp = policy_ids(side, done)
        keep = [to_side(side, ids), to_side(side, act), to_side(side, lp)]
        if call < 2:
            for e_ in bad_ents():
                refused(lambda: side.handle.rollout_record_entities(buf.c(), addr(keep[0]), addr(keep[1]), addr(keep[2]), e_))
            for c_ in bad_bufs():
                refused(lambda: side.handle.rollout_record_entities(c_, addr(keep[0]), addr(keep[1]), addr(keep[2])))
            for k in range(3):
                p = [addr(x) for x in keep]; p[k] = 0
                refused(lambda: side.handle.rollout_record_entities(buf.c(), *p))
            side.handle.set_entity_out()
            refused(lambda: side.handle.rollout_record_entities(buf.c(), addr(keep[0]), addr(keep[1]), addr(keep[2])))
            side.handle.set_entity_out(*reg)
        record(side, buf.c(), ids, act, lp)
        record(side, twin.c(), ids, act, lp, ent=reg)
        m.record(ids, act, lp)
        side.step(ids, act.astype(np.float64))
        if call < 3:
            for e_ in bad_ents():
                refused(lambda: collect(side, buf.c(), ent=e_))
            for c_ in bad_bufs():
                refused(lambda: collect(side, c_))
            for k in ("agent_id", "reward", "terminal", "now", "status"):
                refused(lambda: collect(side, buf.c(), **{k: 0}))
            side.handle.set_entity_out()
            refused(lambda: collect(side, buf.c()))
            side.handle.set_entity_out(*reg)
        collect(side, buf.c(), consume=False)
        collect(side, twin.c(), ent=reg, consume=True)
        m.collect([e for e in range(side.B) if ids[e] != -2])
    a_ = assert_equals_mirror(buf, m, "arguments")
    assert int(a_["count"].sum()) > 0 and len(m.out[0]) + len(m.out[1]) == int(a_["count"].sum())
    # the explicit `ent`: the same transitions, bit for bit.  Two environments that return one charger in one call race for its slots,
    # and the two launches need not resolve the race alike, so the stored rows are compared by key (both against the mirror); what no
    # race touches -- the counts and everything pending -- byte for byte
    assert_equals_mirror(twin, m, "arguments, explicit ent")
    s1, s2 = buf.snap(), twin.snap()
    assert all(np.array_equal(s1[k], s2[k]) for k in ("count", "pend_state", "pend_action", "pend_logp", "pend_valid"))
    side.close()


def test_emulated_entity_rollout_bad_arguments():
    bad_arguments_leave_everything_untouched(EmuSide)
