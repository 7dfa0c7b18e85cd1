"""The lookahead expert (wrsn_clone_envs_from, wrsn_lookahead_candidates / _collect / _pick, `LookaheadPolicy`) on the emulated library.

The bodies take the side (tests/sides.py) or a factory of environments: this module runs them on EmuSide, tests/test_lookahead_gpu.py on
VecSide / VecWRSN.  References and why each comparison is of bytes: tests/lookahead_ref.py.  Sizes of the candidates tests are those of
tests/test_entity_heuristic.py (N = 5 a partial wave, 64 one wave, 65 a wave and a node, 257 more than four; M = 1, 3, 8; B = 6: two
blocks, the second partial) times K = 1, 3, 8.

End to end: the networks of tests/test_evaluate.py (B = 8, 33 nodes of 1 000 J, M = 3), K = 3, a simulation batch of 24 slots.  SEED and
HORIZON were chosen on the emulator with `reference_policy` alone, the horizon search starting at a tenth of these networks' 150 to 200 s
under the heuristic: at 16 s, the first value tried, the reference picks k != 0 and k == 0 from the third decision on, and clones die
inside their horizon from decision 17 on, when the first networks are about to die (with max_time = 1e9: inside the 320 s of
tests/test_evaluate.py no clone dies).  A decision costs the emulator over a second (reference and policy), so its test reaches that
point with EMU_PREFIX = 14 launches under the plain heuristic, one step each, and compares the EMU_LAUNCHES = 3 decisions that follow,
in which the reference meets all three conditions (2 / 5 / 3 rows at the second of them); the device test starts at the reset and runs
every episode to its end.  Both assert the three conditions."""
import numpy as np
import pytest
from sides import EmuSide, load_fixture

import entity_act_ref as R
import entity_train_ref as T
import episode_ref as E
import lookahead_ref as L
import test_entity_heuristic as H
import test_evaluate as V

WRSN_ERR_ARG = -1
KS = (1, 3, 8)
SEED, HORIZON, EMU_PREFIX, EMU_LAUNCHES = 500, 16.0, 14, 3


# ------------------------------------------------------------------------------------------------------------ 1. clone across handles
def _rows_of(side, envs):
    rows = side.rows()
    return [rows[e] for e in envs]


def clone_across_handles(Side):
    """Source B = 2, destination B = 6, M = 3: after 1 -> 3 and after 2 -> 6 every destination's next 5 requests under one action script
    equal its source's own continuation bit for bit -- request rows and entity rows -- and the source's record bytes are the same before
    and after a clone."""
    _, sc, mc = load_fixture("hanoi1000n50_m3_s1")
    _, sc2, _ = load_fixture("sonla1000n50_m2_s4")
    kw = dict(map_size=12, render=False, entities=True)
    src, dst = Side([sc, sc2], mc, 3, **kw), Side([sc2, sc] * 3, mc, 3, **kw)
    src.reset(); dst.reset()
    rng = np.random.default_rng(11)
    for _ in range(3):
        src.step(src._host()["agent_id"], rng.random((2, 3)) * [1, 1, 0.3])
    for src_idx, dst_idx in (([0, 0, 0], [1, 3, 5]), ([0, 1, 0, 1, 0, 1], [0, 1, 2, 3, 4, 5])):
        rec0, rows0, ent0 = np.array(_host_bytes(src.save_envs())), src.rows(), L.ent_rows(src)
        dst_rec0 = np.array(_host_bytes(dst.save_envs()))
        L.clone_from(dst, src, src_idx, dst_idx)
        assert np.array_equal(np.array(_host_bytes(src.save_envs())), rec0) and src.rows() == rows0
        assert all(np.array_equal(a, b) for a, b in zip(L.ent_rows(src), ent0))
        others = [e for e in range(6) if e not in dst_idx]
        if others:                                            # environments the call did not name keep every byte
            assert np.array_equal(np.array(_host_bytes(dst.save_envs(others))), dst_rec0[others])
        assert _rows_of(dst, dst_idx) == [rows0[s] for s in src_idx]
        se, de = L.ent_rows(src), L.ent_rows(dst)
        for s, d in zip(src_idx, dst_idx):
            if rows0[s][0] >= 0:                              # the cloned rows are rendered: entity rows included
                assert all(np.array_equal(a[s], b[d]) for a, b in zip(se, de)), (s, d)
        for k in range(5):
            act = rng.random((2, 3)) * [1, 1, 0.3]
            ids_s = src._host()["agent_id"]
            ids_d = np.full(6, -2, np.int32); acts_d = np.zeros((6, 3))
            for s, d in zip(src_idx, dst_idx):
                ids_d[d] = ids_s[s]; acts_d[d] = act[s]
            src.step(ids_s, act); dst.step(ids_d, acts_d)
            rs = src.rows()
            assert _rows_of(dst, dst_idx) == [rs[s] for s in src_idx], (k, rs, dst.rows())
            se, de = L.ent_rows(src), L.ent_rows(dst)
            for s, d in zip(src_idx, dst_idx):
                assert all(np.array_equal(a[s], b[d]) for a, b in zip(se, de)), (k, s, d)
    src.close(); dst.close()


def _host_bytes(rec):
    return rec if isinstance(rec, np.ndarray) else rec.cpu().numpy()


def test_emulated_clone_across_handles():
    clone_across_handles(EmuSide)


def clone_refusals(Side, other_stream, other_device=None):
    """Every refusal of wrsn_clone_envs_from is WRSN_ERR_ARG with a message and changes nothing in either handle."""
    from multi_agent_rl_wrsn_amd._lib import RawHandle, WrsnError
    _, sc, mc = load_fixture("hanoi1000n50_m3_s1")
    _, scp, mcp = load_fixture("prob_gp/hanoi1000n50_m3_p05")
    kw = dict(map_size=12, render=False, entities=True)
    src, dst, gen = Side([sc, sc], mc, 3, **kw), Side([sc] * 3, mc, 3, **kw), Side([scp], mcp, 3, **kw)
    for s in (src, dst, gen):
        s.reset()
    src.step(src._host()["agent_id"], np.full((2, 3), 0.3))
    lib, N, Tn = src.handle.lib, src.N, src.T
    bare = lambda B=2, n=N, t=Tn, m=3, **k: RawHandle(lib, B, n, t, m, 12, 100.0, 0, **k)
    empty, wide, many, deg, cov, big = bare(), bare(n=200), bare(m=2), bare(max_degree=9), bare(max_cover=9), bare(t=200)
    small_dst = bare(n=N - 1)                                 # the same NP, one node fewer than the source handle
    state = lambda: (np.array(_host_bytes(src.save_envs())), src.rows(), np.array(_host_bytes(dst.save_envs())), dst.rows())
    base = state()

    def refused(word, d=dst, s=src.handle, si=(0, 1), di=(0, 1), **over):
        with pytest.raises(WrsnError) as ei:
            if isinstance(d, RawHandle):
                d.clone_envs_from(s, si, di, over.get("src_req", L.req_only(src)), **L.out_ptrs(dst))
            else:
                L.clone_from(d, src, si, di, src_handle=s, **over)
        assert ei.value.code == WRSN_ERR_ARG and word in str(ei.value), (word, str(ei.value))
        now = state()
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(now, base)), word

    refused("same handle", s=dst.handle)
    refused("NP", s=wide)
    refused("TP", s=big)
    refused("ECAP", s=deg)
    refused("CCAP", s=cov)
    refused("M", s=many)
    refused("n_node", d=small_dst)
    refused("generators", s=gen.handle, si=(0,), di=(0,))
    refused("holds no scenario", s=empty)
    refused("null", s=None)
    refused("null", src_req=None)
    refused("n < 1", si=(), di=())
    refused("request rows", src_req=dict(L.req_only(src), now=0))
    refused("out of range", si=(0, 2))
    refused("appears twice", di=(1, 1))
    src.handle.set_stream(other_stream(src))
    refused("different streams")
    src.handle.set_stream(other_stream(src, back=True))
    if other_device is not None:
        refused("different devices", s=other_device(lib, N, Tn))
    L.clone_from(dst, src, [0, 1], [2, 0])                    # and the valid call still works
    assert _rows_of(dst, [2, 0]) == src.rows()
    for h in (empty, wide, many, deg, cov, big, small_dst):
        h.close()
    for s in (src, dst, gen):
        s.close()


def test_emulated_clone_refusals():
    clone_refusals(EmuSide, lambda side, back=False: 0 if back else 64)   # the emulator only stores the stream: any other value differs


# ------------------------------------------------------------------------------------------------------------ 2. candidates
def now_for(B):
    return np.linspace(3.0, 250.75, B)


def candidates_sizes(Side, N, M, K):
    """Every byte of the [K, B] outputs and of the state slots equals the reference; candidate 0 equals the heuristic's calls; skipped
    rows keep the pattern; padding appears exactly where a row has fewer than K alive nodes."""
    side = E.BareSide(Side, H.B0, N, M)
    node, mc, env, ids = H.rows_for(N, M)
    node[2, :, 7] = 0; node[2, :2, 7] = 1                     # row 2: two alive nodes
    call = L.CandCall(side, node, mc, env, ids, now_for(H.B0), K)
    got, _ = call.check(horizon=12.5, min_charge=0.0, tag=(N, M, K, "mc 0"))
    for k in range(K):
        assert (got["node"][k, [1, 4]].view(np.uint8) == T.PATTERN).all()      # the skipped rows
        assert (got["node"][k, 2] >= 0) == (k < 2) and got["done"][k, 2] == (0 if k < 2 else 1) and got["sim_agent_id"][k, 2] == (ids[2] if k < 2 else -2)
    call.check(horizon=7.0, charge_scale=0.7, min_charge=0.02, tag=(N, M, K, "mc 0.02"))
    side.close()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N,M", H.SIZES)
def test_emulated_candidates_sizes(N, M, K):
    candidates_sizes(EmuSide, N, M, K)


def candidates_planted(Side, N=65, M=3, K=3):
    """Planted rows: ties (the lowest index first), the unclaimed / claimed boundary inside the first K, everything claimed, no alive
    node, NaN and inf scores."""
    f = np.float32
    B = 6
    side = E.BareSide(Side, B, N, M)
    node, mc, env, _ = H.rows_for(N, M, B, seed=1)
    ids = np.zeros(B, np.int32)
    mc[:, :, 3] = 0; mc[:, 0, 3] = 1; mc[:, :, 4] = 0
    node[..., 7] = 1; node[..., 2] = np.linspace(0.1, 0.9, N, dtype=f)[None, :]; node[..., 3] = f(0.5)
    node[..., 0] = np.linspace(0.05, 0.95, N, dtype=f)[None, :]; node[..., 1] = f(0.5)
    last = N - 1
    node[0, :, 2] = f(0.3); node[0, [4, 2, last], 2] = f(0.7)                 # 0: three equal best scores
    if M > 1:                                                                 # 1: a disc that leaves only nodes 1 and 3 unclaimed
        mc[1, 1, 4] = 1; mc[1, 1, 6] = node[1, 1, 0]; mc[1, 1, 7] = f(0.5); env[1, :2] = f(10.0)
        node[1, [1, 3], 1] = f(200.0)                                         #    (far away in v: outside the disc)
        mc[2, 1, 4] = 1; mc[2, 1, 6:8] = f(0.5); env[2, :2] = f(10.0)         # 2: everything claimed
    node[3, :, 7] = 0                                                         # 3: no alive node
    node[4, last, 2] = f(np.nan); node[4, 1, 2] = f(np.inf); node[4, 5, 2] = f(-np.inf); node[4, 6:, 7] = 0   # 4: NaN, inf, -inf among 6 alive
    call = L.CandCall(side, node, mc, env, ids, now_for(B), K)
    got, _ = call.check(horizon=20.0, min_charge=0.02, tag="planted")
    assert got["node"][:, 0].tolist() == [2, 4, last][:K]
    if M > 1:
        _, _, claimed = L.ranking(node[1], mc[1], env[1], 0)
        assert claimed.sum() == N - 2 and got["node"][:, 1].tolist() == [3, 1, last][:K]          # two unclaimed, then the best claimed
        assert L.ranking(node[2], mc[2], env[2], 0)[2].all() and got["node"][:, 2].tolist() == [last, last - 1, last - 2][:K]
    assert got["node"][:, 3].tolist() == [-1] * K and got["sim_agent_id"][:, 3].tolist() == ([0] + [-2] * K)[:K]
    assert got["done"][:, 3].tolist() == ([0] + [1] * K)[:K] and got["sim_action"][0, 3].tolist() == [float(mc[3, 0, 0]), float(mc[3, 0, 1]), 0.02]
    assert got["node"][:, 4].tolist() == [1, 4, 3][:K]                         # inf first, then by score; NaN and -inf last
    side.close()
    if K == 3:                                                                # and the tail of row 4's order, with K = 8 > 6 alive nodes
        side = E.BareSide(Side, B, N, M)
        got, _ = L.CandCall(side, node, mc, env, ids, now_for(B), 8).check(horizon=20.0, tag="planted K 8")
        assert got["node"][:, 4].tolist() == [1, 4, 3, 2, 0, 5, -1, -1] and got["done"][:, 4].tolist() == [0] * 6 + [1, 1]
        side.close()


def test_emulated_candidates_planted():
    candidates_planted(EmuSide)


def test_emulated_candidates_planted_single_charger():
    candidates_planted(EmuSide, N=64, M=1)


def candidates_properties(Side):
    """A row's bytes do not depend on the other rows or on the row order; two calls give equal bytes."""
    N, M, K = 65, 3, 3
    side = E.BareSide(Side, H.B0, N, M)
    node, mc, env, ids = H.rows_for(N, M)
    now = now_for(H.B0)
    base, _ = L.CandCall(side, node, mc, env, ids, now, K).check(min_charge=0.02, tag="base")
    again, _ = L.CandCall(side, node, mc, env, ids, now, K).check(min_charge=0.02, tag="again")
    assert all(E.same(base[k], again[k]) for k in base)
    perm = np.array([3, 5, 0, 1, 4, 2])
    got, _ = L.CandCall(side, node[perm], mc[perm], env[perm], ids[perm], now[perm], K).check(min_charge=0.02, tag="permuted")
    assert all(E.same(got[k], base[k][:, perm]) for k in L.SHAPES(K, H.B0))
    for keep in (0, 3):
        n2, m2, e2 = node.copy(), mc.copy(), env.copy()
        others = [e for e in range(H.B0) if e != keep]
        n2[others] = np.nan; m2[others] = np.nan; e2[others] = np.nan
        got = L.CandCall(side, n2, m2, e2, ids, now, K).run(min_charge=0.02)
        assert all(E.same(got[k][:, keep], base[k][:, keep]) for k in L.SHAPES(K, H.B0)), keep
    side.close()


def test_emulated_candidates_properties():
    candidates_properties(EmuSide)


def candidates_bad_arguments(Side):
    """Every WRSN_ERR_ARG case leaves every buffer untouched, and the valid call that follows gives the reference's bytes."""
    from multi_agent_rl_wrsn_amd._lib import WrsnError
    N, M, K = 33, 3, 3
    side = E.BareSide(Side, H.B0, N, M)
    node, mc, env, ids = H.rows_for(N, M)
    call = L.CandCall(side, node, mc, env, ids, now_for(H.B0), K)
    nd, mp, ev = call.ent.ptrs()
    b, raw = call.look.buf, call.look.raw
    cases = [dict(state=raw(K=0)), dict(state=raw(K=9)), dict(state=raw(B=H.B0 + 1)), dict(state=None), dict(state=raw(t0=0)), dict(state=raw(done=0)),
             dict(state=raw(ret=b["ret"].ptr + 4)), dict(agent_ptr=0), dict(now_ptr=0), dict(node=0), dict(sim_agent_id=0), dict(sim_action=0), dict(stored=0),
             dict(ent=None), dict(ent=(0, mp, ev)), dict(ent=(nd + 4, mp, ev)), dict(ent=(nd, mp + 8, ev)), dict(sim_action=b["sim_action"].ptr + 4),
             dict(node=b["node"].ptr + 2), dict(horizon=float("nan")), dict(horizon=float("inf")), dict(horizon=0.0), dict(horizon=-1.0),
             dict(min_charge=-0.1), dict(min_charge=1.0), dict(min_charge=float("nan")), dict(x_clip=0.0), dict(x_clip=float("inf"))]
    for over in cases:
        with pytest.raises(WrsnError) as ei:
            call.run(**over)
        assert ei.value.code == WRSN_ERR_ARG, over
        R.sync(side)
        assert call.look.untouched(), over
    call.check(tag="after the refusals")
    side.close()


def test_emulated_candidates_bad_arguments():
    candidates_bad_arguments(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 3. collect and pick
def collect_matches_the_host(Side, step_budget):
    """A simulation side of 8 slots under a random action script, the state initialised by hand with horizons that end early, late and
    never: every field and next_agent_id of every collect equal the host mirror's, with and without close_all.  The request rows the
    call reads are the test's copies of the side's, so that one of them can be scripted to fall off the end (status 1, no charger):
    these networks either die or run on for ever, no action script makes a step of theirs fall off.  Without a step budget the run must
    show terminal returns inside a horizon, the fell-off row and closings by the horizon; with one, rows in flight."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    K, B = 2, 4
    R_ = K * B
    side = Side(V.scenarios(R_), DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True, step_budget=step_budget)
    look = L.LookBuf(side, K, B)
    side.reset()
    now0 = side._host()["now"]
    horizon = np.array([1e9, 1e9, 40.0, 1e9, 150.0, 1e9, 300.0, 5.0])
    done0 = np.zeros(R_, np.uint8); done0[3] = 1               # slot 3 was never valid
    z = np.zeros(R_)
    look.set(t0=now0, t_end=now0 + horizon, last_now=now0, ret=z, survived=z - 1.0, done=done0, died=np.zeros(R_, np.uint8))
    look.next.set(np.full(R_, E.NEXT_FILL, np.int32))
    g0 = look.get()
    host = L.HostLook(g0, g0["next"])
    states = E.RowStates(R_)
    states.after_reset()
    rng = np.random.default_rng(3)
    dts = dict(agent_id=np.int32, reward=np.float64, terminal=np.uint8, now=np.float64, status=np.int32)
    rows = {k: T.Guarded(side, (R_,), dt) for k, dt in dts.items()}
    seen, launches, fell = set(), 0, []

    def one(close_all=False, fall=None):
        seen.update(int(s) for s in states.st)
        req = side._host()
        if fall is not None and states.st[fall] == 1:          # the scripted row: this step fell off the end
            req["status"][fall] = 1; req["agent_id"][fall] = -1; req["reward"][fall] = 0.0
            fell.append(fall)
        for k, b in rows.items():
            b.set(req[k])
        L.collect(side, look, close_all, req={k: b.ptr for k, b in rows.items() if k != "terminal"})
        host.collect(states, req, close_all)
        got, want = look.get(), host.get(K, B)
        for k in want:
            assert E.same(got[k], want[k]), (launches, k, got[k], want[k])
        assert look.guards_intact() and all(b.guards_intact() for b in rows.values())
        for k in ("node", "sim_agent_id", "sim_action", "stored", "choice", "action_f64", "action", "chosen"):
            assert (got[k].view(np.uint8) == T.PATTERN).all(), k
        return got

    got = one()                                               # after the reset: nothing is written, next keeps its bytes
    assert (got["next"][done0 == 0] == E.NEXT_FILL).all() and got["next"][3] == -2
    ids = np.where(done0 != 0, -2, side._host()["agent_id"]).astype(np.int32)
    while not got["done"].all() and launches < 40:
        side.step(ids, rng.random((R_, 3)) * [1, 1, 0.5]); states.after_step(ids, side._host())
        launches += 1
        got = one(fall=5 if launches == 3 else None)
        again = one()                                         # the row state was consumed: a second call finds nothing
        assert all(E.same(got[k], again[k]) for k in got)
        ids = got["next"].copy()
        if step_budget and launches == 4:
            break
    flat = {k: got[k].reshape(-1) for k in ("done", "died", "survived", "last_now", "t0")}
    if step_budget:
        assert 3 in seen and not got["done"].all()
        got = one(close_all=True)                             # closes what is open with the last_now it has
        assert got["done"].all() and (got["next"] == -2).all()
    else:
        assert got["done"].all() and {1, 4} <= seen and fell == [5]
        died = flat["died"] != 0
        assert died[[0, 1]].all() and not died[[3, 5]].any()                    # terminal returns inside the horizon
        assert (flat["survived"][[0, 1]] == (flat["last_now"] - flat["t0"])[[0, 1]]).all() and (flat["survived"][[0, 1]] < 1e9).all()
        late = died & (flat["last_now"] - flat["t0"] > horizon)                 # a terminal return behind the horizon counts as the horizon
        assert (flat["survived"][late] == horizon[late]).all()
        assert 0 < flat["survived"][5] == flat["last_now"][5] - flat["t0"][5] < 1e9            # the fell-off row closed where it fell
        by_horizon = ~died & (np.arange(R_) != 3) & (np.arange(R_) != 5)
        assert by_horizon.sum() >= 2 and (flat["survived"][by_horizon] == horizon[by_horizon]).all() and flat["survived"][3] == -1.0
    side.close()


@pytest.mark.parametrize("step_budget", [0, 60])
def test_emulated_collect_matches_the_host(step_budget):
    collect_matches_the_host(EmuSide, step_budget)


def pick_cases(Side):
    """Hand-built states: each key decides, a NaN never wins, invalid and unfinished slots are ignored, nothing valid gives k = 0, skipped
    rows keep every byte."""
    from multi_agent_rl_wrsn_amd._lib import WrsnError
    K, B, M = 4, 8, 3
    side = E.BareSide(Side, B, 5, M)
    look = L.LookBuf(side, K, B)
    nan = np.nan
    #            survived per k             ret per k                 sim_agent_id            done
    rows = [([5, 9, 9, 1],            [0, 1, 2, 3],            [0, 0, 0, 0],           [1, 1, 1, 1]),     # 0: survived, then ret: k = 2
            ([7, 7, 7, 7],            [1, 4, 4, 2],            [1, 1, 1, 1],           [1, 1, 1, 1]),     # 1: ties in both: the lowest k = 1
            ([3, 8, 2, 1],            [9, 0, 9, 9],            [2, 2, 2, 2],           [1, 1, 1, 1]),     # 2: survived alone: k = 1
            ([6, 6, 6, 6],            [1, nan, 0.5, nan],      [0, 0, 0, 0],           [1, 1, 1, 1]),     # 3: NaN ret never wins: k = 0
            ([nan, 2, nan, 1],        [9, 1, 9, 1],            [0, 0, 0, 0],           [1, 1, 1, 1]),     # 4: NaN survived never wins: k = 1
            ([1, 99, 99, 3],          [0, 5, 5, 0],            [1, -2, 1, 1],          [1, 1, 0, 1]),     # 5: invalid (1) and unfinished (2) ignored: k = 3
            ([9, 9, 9, 9],            [1, 1, 1, 1],            [2, -2, -2, -2],        [0, 1, 1, 1]),     # 6: nothing qualifies: k = 0
            ([1, 2, 3, 4],            [1, 2, 3, 4],            [0, 0, 0, 0],           [1, 1, 1, 1])]     # 7: skipped (agent -1)
    want = [2, 1, 1, 0, 1, 3, 0]
    sv, rt, sa, dn = (np.array([r[i] for r in rows]).T.copy() for i in range(4))
    rng = np.random.default_rng(0)
    act, st = rng.random((K, B, 3)), rng.random((K, B, 2)).astype(np.float32)
    look.set(survived=sv.astype(np.float64), ret=rt.astype(np.float64), sim_agent_id=sa.astype(np.int32), done=dn.astype(np.uint8), sim_action=act, stored=st,
             t0=np.zeros((K, B)), t_end=np.zeros((K, B)), last_now=np.zeros((K, B)), died=np.zeros((K, B), np.uint8), node=np.zeros((K, B), np.int32))
    ids = T.Guarded(side, (B,), np.int32, data=np.array([0, 1, 2, 0, 0, 1, 2, -1], np.int32))
    before = look.get()
    L.pick(side, look, ids.ptr)
    got = look.get()
    assert look.guards_intact() and ids.guards_intact()
    assert got["choice"][:7].tolist() == want == [L.pick_ref(sa[:, e], dn[:, e], sv[:, e], rt[:, e]) for e in range(7)]
    for e, k in enumerate(want):
        assert E.same(got["action_f64"][e], act[k, e]) and E.same(got["action"][e], act[k, e].astype(np.float32)) and E.same(got["chosen"][e], st[k, e])
    for k in ("choice", "action_f64", "action", "chosen"):
        assert (got[k][7:].view(np.uint8) == T.PATTERN).all(), k
    for k in list(L.SHAPES(K, B)) + ["next"]:
        assert E.same(got[k], before[k]), k
    only = L.LookBuf(side, K, B)                              # the optional outputs may be NULL
    only.set(**{k: before[k] for k in L.SHAPES(K, B)})
    L.pick(side, only, ids.ptr, action_f64=0, action=0, stored=0, cand_stored=0)
    assert only.get()["choice"][:7].tolist() == want and only.action_f64.untouched() and only.chosen.untouched()
    look.choice.fill()
    for over in (dict(agent_ptr=0), dict(sim_agent_id=0), dict(sim_action=0), dict(choice=0), dict(cand_stored=0), dict(state=None),
                 dict(state=look.raw(K=9)), dict(state=look.raw(B=B - 1)), dict(state=look.raw(survived=0))):
        with pytest.raises(WrsnError) as ei:
            L.pick(side, look, ids.ptr, **over)
        assert ei.value.code == WRSN_ERR_ARG and look.choice.untouched(), over
    wrong = E.BareSide(Side, B + 1, 5, M)                     # collect on a handle whose batch is not K * B
    req = dict(agent_id=ids.ptr, reward=look.buf["ret"].ptr, now=look.buf["t0"].ptr, status=look.choice.ptr)
    before = look.get()
    for over in (dict(), dict(nxt=0), dict(state=None), dict(state=look.raw(K=0))):
        with pytest.raises(WrsnError) as ei:
            L.collect(wrong, look, req=req, **over)
        assert ei.value.code == WRSN_ERR_ARG, over
    right = E.BareSide(Side, K * B, 5, M)                     # the right batch: the request rows are still checked
    for over in (dict(now=0), dict(status=0), dict(nxt=ids.ptr)):
        with pytest.raises(WrsnError) as ei:
            L.collect(right, look, req=req, **over)
        assert ei.value.code == WRSN_ERR_ARG, over
    after = look.get()
    assert all(E.same(after[k], before[k]) for k in before)
    wrong.close(); right.close(); side.close()


def test_emulated_pick_cases():
    pick_cases(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 4. end to end
def emu_envs(K, max_time=V.MAX_TIME):
    """(real, sim) environments of tests/test_evaluate.py's networks on the emulator: sim holds K copies of the batch."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    scs = V.scenarios(8, seed=SEED, max_time=max_time)
    mk = lambda s: L.emu_look_vec(EmuSide(s, DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True))
    return mk(scs), mk(scs * K)


def close_envs(envs):
    for env in envs:
        env.side.close() if hasattr(env, "side") else env.close()


def k1_is_the_heuristic(make_envs, whole_episode):
    """K = 1: the actions are HeuristicPolicy(min_charge=0.02)'s bytes at every launch, and the evaluate_policy result (the partial log at
    the launch cap, where the episodes are not run to their end) equals the heuristic's field for field."""
    from multi_agent_rl_wrsn_amd import HeuristicPolicy, LookaheadPolicy, evaluate_policy
    from multi_agent_rl_wrsn_amd.evaluate import LaunchCapReached
    env, sim = make_envs(1)
    twin, sim2 = make_envs(1)
    look, heur, calls = LookaheadPolicy(sim, K=1, horizon=HORIZON, min_charge=0.02), HeuristicPolicy(min_charge=0.02), [0]

    def both(e, ids):
        a = look(e, ids).clone()
        b = heur(e, ids)
        rows = ((ids >= 0) & (ids < e.num_agent)).cpu().numpy()
        assert E.same(a.cpu().numpy()[rows], b.cpu().numpy()[rows]) and (look.choice.cpu().numpy()[rows] == 0).all(), calls
        calls[0] += 1
        return a

    def run(e, policy):
        try:
            return evaluate_policy(e, policy, episodes=1, max_launches=400 if whole_episode else 5)
        except LaunchCapReached as ex:
            assert not whole_episode
            return ex.result

    got, want = run(env, both), run(twin, heur)
    assert calls[0] == int(got["launches"]) > 0 and look.calls == calls[0] and look.sim_launches >= look.calls
    for k in want:
        if k != "summary":
            assert E.same(got[k], want[k]), k
    close_envs((env, sim, twin, sim2))


def test_emulated_k1_is_the_heuristic():
    k1_is_the_heuristic(emu_envs, whole_episode=False)


def _advance(env, ids, act):
    """One launch of the real environment; rows whose episode ended (or that were left alone) are left alone from now on."""
    r = env.step(ids, act)
    L.sync(env)
    term, status, agent = (r[k].cpu().numpy() for k in ("terminal", "status", "agent_id"))
    keep = (ids.cpu().numpy() != -2) & (term == 0) & (status != 1) & (agent >= 0)
    return env.torch.from_numpy(np.where(keep, agent, -2).astype(np.int32)).to(env.device)


def k3_matches_the_reference(make_envs, prefix, launches, whole=False):
    """K = 3 on networks without a time limit (every episode ends by death).  After `prefix` launches under HeuristicPolicy(min_charge=0.02)
    -- 0 on the device; on the emulator the prefix brings the networks to where they die, at the price of one step a launch -- at every
    decision of the next `launches` launches choice, the action bytes, ret, survived and died equal the host reference loop's; the real
    environment's record bytes are the same before and after a policy call; a second run, without the reference, gives the first one's
    bytes.  The reference alone picks k != 0 and k == 0, and a slot closes by a terminal return inside its horizon.  whole: the launches
    must have taken every environment to the end of its episode."""
    from multi_agent_rl_wrsn_amd import HeuristicPolicy, LookaheadPolicy
    K = 3
    runs = []
    for with_ref in (True, False):
        env, sim = make_envs(K, 1e9)
        ref_sim = make_envs(K, 1e9)[1] if with_ref else None
        policy, heur = LookaheadPolicy(sim, K=K, horizon=HORIZON, min_charge=0.02, poll=4), HeuristicPolicy(min_charge=0.02)
        ids = env.reset()["agent_id"].clone()
        for _ in range(prefix):
            ids = _advance(env, ids, heur(env, ids))
        log = []
        for n in range(launches):
            rows = ((ids >= 0) & (ids < env.num_agent)).cpu().numpy()
            if not rows.any():
                break
            want = L.reference_policy(env, ref_sim, ids, K, HORIZON, min_charge=0.02) if with_ref else None
            rec0 = env.save_envs().cpu().numpy().copy()
            act = policy(env, ids).clone()
            L.sync(env)
            assert np.array_equal(env.save_envs().cpu().numpy(), rec0), n
            v = (policy.look.sim_agent_id.cpu().numpy() >= 0) & rows[None, :]
            got = dict(choice=policy.choice.cpu().numpy()[rows], action=act.cpu().numpy()[rows], stored=policy.stored.cpu().numpy()[rows],
                       ret=policy.look.ret.cpu().numpy()[v], survived=policy.look.survived.cpu().numpy()[v], died=policy.look.died.cpu().numpy()[v] != 0)
            if with_ref:
                assert (v == want["valid"]).all(), n
                assert E.same(got["choice"], want["choice"][rows]), (n, got["choice"], want["choice"])
                assert E.same(got["action"], want["action"][rows]), n
                assert E.same(got["ret"], want["ret"][v]) and E.same(got["survived"], want["survived"][v]) and (got["died"] == want["died"][v]).all(), n
                inside = want["died"] & v & (want["survived"] < HORIZON)
                got.update(k_other=int((want["choice"][rows] != 0).sum()), k_zero=int((want["choice"][rows] == 0).sum()), inside=int(inside.sum()))
            log.append(got)
            ids = _advance(env, ids, act)
        assert not whole or not bool(((ids >= 0) & (ids < env.num_agent)).any()), "whole: every environment's episode must have ended"
        if with_ref:                                          # conditions on the reference, not measurements
            assert sum(x["k_other"] for x in log) >= 1 and sum(x["k_zero"] for x in log) >= 1 and sum(x["inside"] for x in log) >= 1, \
                [(x["k_other"], x["k_zero"], x["inside"]) for x in log]
        runs.append(log)
        close_envs([e for e in (env, sim, ref_sim) if e is not None])
    assert len(runs[0]) == len(runs[1]) > 0
    for a, b in zip(*runs):
        for k in ("choice", "action", "stored", "ret", "survived", "died"):
            assert E.same(a[k], b[k]), k


def test_emulated_k3_matches_the_reference():
    k3_matches_the_reference(emu_envs, EMU_PREFIX, EMU_LAUNCHES)
