"""Scenario pools (wrsn_pool_set / wrsn_pool_reset) on the CPU: the unmodified HIP sources in the lockstep wavefront emulator of
tests/emu.  A finished episode restarts in a pool record the device selects: pinned to the reference runs of tests/golden, to
wrsn_load_envs of the same records, and to Python's `random` for prob_gp < 1."""
import numpy as np
import pytest

from parity import check_decision, close
from test_env_records import _peeks, _row, _same
from sides import EmuSide, aligned, load_fixture, python_mt_state

SENT_I, SENT_F = -77, -12345.5                                # sentinels of rows that must stay untouched


def PoolEmu(scenarios, mc, M, N, T, **kw):
    """An EmuSide for a stated geometry (n_node / n_target of the handle, not the largest of its scenarios): what one pool needs of the
    handles its records come from and go to."""
    return EmuSide(scenarios, mc, M, n_node=N, n_target=T, **kw)


def _record(ev, e=0):
    """The record of environment e with its pending request."""
    rec = aligned((1, ev.h.env_record_bytes()))
    p = ev._ptrs(False); p.pop("obs")
    ev.h.save_envs(np.asarray([e], dtype=np.int32), rec.ctypes.data, **p)
    return rec


def _pool(records):
    out = aligned((len(records), records[0].shape[1]))
    for i, r in enumerate(records):
        out[i] = r[0]
    return out


def _pool_reset(ev, mask=None, index=None, ids=None, with_obs=True):
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    ev.h.pool_reset(0 if m is None else m.ctypes.data, 0 if i is None else i.ctypes.data, 0 if ids is None else ids.ctypes.data,
                    **ev._ptrs(with_obs))


def _pool_info(ev):
    """[B, 2]: the pool record every environment runs, and its swaps."""
    info = ev.pool_info()
    return np.stack([info["record"], info["swaps"]], 1)


def _fill_sentinels(ev):
    ev.agent_id[:] = SENT_I; ev.status[:] = SENT_I; ev.reward[:] = SENT_F; ev.now[:] = SENT_F; ev.terminal[:] = 99; ev.obs[:] = SENT_F


POOL_FIXTURES = ("hanoi1000n50_m2_cap9000_detour", "sonla1000n50_m2_s4", "redundant_m2_deaths")


def test_terminal_rows_restart_in_the_drawn_fixture(hip_lib):
    """Three networks of different node counts, targets and charger specs in one pool of a 82-node / 56-target handle.  Each of three
    environments runs one of them to its terminal return under the reference's actions; the next call replaces exactly the terminal
    rows, by the record pool_draw names, and the episode that follows is the drawn fixture's, decision by decision."""
    from multi_agent_rl_wrsn_amd import pool_draw
    N, T, M, P = 82, 56, 2, 3
    fx = [load_fixture(n) for n in POOL_FIXTURES]
    assert [len(z["in_action"]) for z, _, _ in fx] == [8, 7, 16]
    assert len({tuple(mc.values()) for _, _, mc in fx}) > 1 and len({sc.n_node for _, sc, _ in fx}) == 3
    recs = []
    for z, sc, mc in fx:
        src = PoolEmu([sc], mc, M, N, T)
        src.reset()
        recs.append(_record(src))
        src.h.close()
    pool = _pool(recs)
    ev = PoolEmu([fx[0][1]] * 3, fx[0][2], M, N, T)
    ev.reset()
    ev.h.load_envs([0, 1, 2], pool.ctypes.data, **ev._ptrs(True))    # environment e starts in fixture e
    seed = 2
    # the episodes of this seed visit every fixture after a swap (a deterministic property of the stated draw)
    assert {pool_draw(seed, e, 0, P) for e in range(3)} | {pool_draw(seed, e, 1, P) for e in range(3)} == {0, 1, 2}
    ev.h.pool_set(pool.ctypes.data, P, seed)
    assert np.array_equal(_pool_info(ev), [[-1, 0]] * 3)
    cur = [0, 1, 2]; k = [0, 0, 0]; swaps = [0, 0, 0]; pending = [False] * 3; episodes = [0, 0, 0]
    noise = []; checked = 0
    for call in range(80):
        if min(episodes) >= 2:
            break
        ids = np.full(3, -2, dtype=np.int32); act = np.zeros((3, 3))
        for e in range(3):
            if pending[e]:                                    # its last return was terminal: wrsn_pool_reset takes the row
                ids[e] = -1
                continue
            if episodes[e] >= 2:                              # done: left alone
                continue
            z = fx[cur[e]][0]
            ids[e] = int(z["in_agent"][k[e]]); act[e] = z["in_action"][k[e]]
        before = [_row(ev, e) for e in range(3)]
        want_ids = ids.copy()
        _pool_reset(ev, ids=ids)
        for e in range(3):                                    # exactly the terminal rows were marked for the step to leave alone
            assert ids[e] == (-2 if pending[e] else want_ids[e]), (call, e)
        ev.step(ids, act, auto_reset=True)
        info = _pool_info(ev)
        for e in range(3):
            if pending[e]:
                rec = pool_draw(seed, e, swaps[e], P)
                swaps[e] += 1; cur[e] = rec; k[e] = 0; pending[e] = False
                z, sc, _ = fx[rec]
                assert int(ev.status[e]) == 3 and int(ev.agent_id[e]) == int(z["reset_agent"]) and float(ev.reward[e]) == 0.0
                nd = ev.nodes()
                assert close(nd["energy"][e][:sc.n_node], z["reset_node_energy"]) and close(nd["cs"][e][:sc.n_node], z["reset_node_cs"], atol=1e-9)
                assert np.array_equal(nd["status"][e][:sc.n_node], z["reset_node_status"])
                assert np.array_equal(nd["level"][e][:sc.n_node], z["reset_node_level"])
                assert np.max(np.abs(ev.obs[e] - z["reset_obs"])) <= 1e-5 * max(1.0, np.abs(z["reset_obs"]).max())
            elif want_ids[e] == -2:
                assert _row(ev, e) == before[e]
            else:
                z, sc, _ = fx[cur[e]]
                check_decision(z, k[e], ev.decision(e, sc), where="%s (env %d, episode %d)" % (POOL_FIXTURES[cur[e]], e, episodes[e]), noise=noise)
                checked += 1
                if z["terminal"][k[e]]:
                    pending[e] = True; episodes[e] += 1
                k[e] += 1
            assert tuple(info[e]) == (cur[e] if swaps[e] else -1, swaps[e]), (call, e, info[e])
    assert min(episodes) >= 2 and min(swaps) >= 1 and checked >= 8 + 7 + 16 + 3 * 7
    assert len(noise) <= 4, noise


def test_masked_pool_reset_equals_a_load(hip_lib):
    """wrsn_pool_reset with a mask and an index array against wrsn_load_envs of the same records into the same rows of a twin:
    request rows, observations and every peek are bit-identical, and so are the steps that follow; the rows not selected keep their
    sentinel-filled outputs byte for byte."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    M = 2
    own = [synth_scenario(31 + e, 60, 40) for e in range(5)]
    others = [synth_scenario(41, 50, 30), synth_scenario(42, 64, 40), synth_scenario(43, 33, 17)]
    kw = dict(warm_up_time=5.0, map_size=20)
    src = PoolEmu(others, DEFAULT_MC_SPEC, M, 64, 40, **kw)
    src.reset()
    for _ in range(4):                                                  # record 0 is a running environment, not a fresh reset
        src.step([int(src.agent_id[0]), -2, -2], np.array([[0.3, 0.6, 0.1]] * 3))
    pool = _pool([_record(src, e) for e in range(3)])
    a = PoolEmu(own, DEFAULT_MC_SPEC, M, 64, 40, **kw); b = PoolEmu(own, DEFAULT_MC_SPEC, M, 64, 40, **kw)
    rng = np.random.RandomState(5)
    a.reset(); b.reset()
    act = rng.rand(5, 3) * np.array([1.0, 1.0, 0.2])
    a.step(a.agent_id.copy(), act); b.step(b.agent_id.copy(), act)
    a.h.pool_set(pool.ctypes.data, 3, 9)
    _fill_sentinels(a); _fill_sentinels(b)
    mask = [1, 0, 1, 0, 1]; index = [2, 7, 0, -1, 2]                    # (indices of rows not selected are not read)
    ids = np.arange(5, dtype=np.int32)
    _pool_reset(a, mask, index, ids)
    assert list(ids) == [-2, 1, -2, 3, -2]
    loaded = _pool([pool[2:3], pool[0:1], pool[2:3]])
    b.h.load_envs([0, 2, 4], loaded.ctypes.data, **b._ptrs(True))
    for e in (0, 2, 4):
        assert _row(a, e) == _row(b, e) and int(a.status[e]) == 0, e
        assert np.array_equal(a.obs[e], b.obs[e]), e
        _same(_peeks(a, e), _peeks(b, e))
    assert _row(a, 2)[1] > 5.0                                         # the running record's request, not a reset
    for e in (1, 3):
        assert (int(a.agent_id[e]), int(a.status[e]), float(a.reward[e]), float(a.now[e]), int(a.terminal[e])) == (SENT_I, SENT_I, SENT_F, SENT_F, 99)
        assert np.all(a.obs[e] == np.float32(SENT_F))
        _same(_peeks(a, e), _peeks(b, e))
    assert np.array_equal(_pool_info(a), [[2, 1], [-1, 0], [0, 1], [-1, 0], [2, 1]])
    assert np.array_equal(_pool_info(b), [[-1, 0]] * 5)
    # rows 1 and 3 were mid-episode: restore their requests (both handles hold the same), then K further steps
    for ev in (a, b):
        ev.agent_id[[1, 3]] = -1; ev.status[[1, 3]] = 0
    for k in range(4):
        act = rng.rand(5, 3) * np.array([1.0, 1.0, 0.2])
        ia = a.agent_id.copy(); ib = b.agent_id.copy()
        assert np.array_equal(ia, ib)
        a.step(ia, act); b.step(ib, act)
        for e in range(5):
            assert _row(a, e) == _row(b, e), (k, e)
            if a.agent_id[e] >= 0:
                assert np.array_equal(a.obs[e], b.obs[e]), (k, e)
            _same(_peeks(a, e), _peeks(b, e))
    # a clone carries the source's pool record along, a load clears it
    a.h.clone_envs([0], [1], **a._ptrs(True))
    assert tuple(_pool_info(a)[1]) == (2, 0)
    a.h.load_envs([0], pool.ctypes.data, **a._ptrs(True))
    assert tuple(_pool_info(a)[0]) == (-1, 1)


def test_stochastic_pool_record_brings_its_generator(hip_lib):
    from multi_agent_rl_wrsn_amd import _lib
    name = "prob_gp/redundant_m2_p05"
    z, sc, mc = load_fixture(name)
    _, sc2, _ = load_fixture("prob_gp/redundant_rev_m2_p05")
    M = int(z["num_agent"])
    src = PoolEmu([sc], mc, M, 30, 56)
    src.reset()
    pool = _pool([_record(src)])
    want_rng = src.h.peek(_lib.PEEK_RNG_STATE)[0].copy()
    ev = PoolEmu([sc2, sc2], mc, M, 30, 56)
    ev.reset()
    for _ in range(4):                                                  # the old occupants have drawn
        ev.step(ev.agent_id.copy(), np.array([[0.2, 0.4, 0.3]] * 2))
    ev.h.pool_set(pool.ctypes.data, 1, 0)
    _pool_reset(ev, [0, 1], [0, 0])
    assert np.array_equal(ev.h.peek(_lib.PEEK_RNG_STATE)[1], want_rng)
    assert not np.array_equal(ev.h.peek(_lib.PEEK_RNG_STATE)[0], want_rng)
    assert int(ev.agent_id[1]) == int(z["reset_agent"]) and int(ev.status[1]) == 0
    noise = []
    for k in range(len(z["in_action"])):
        ev.step([-2, int(z["in_agent"][k])], np.stack([z["in_action"][k]] * 2))
        check_decision(z, k, ev.decision(1, sc), where=name, noise=noise)
        if z["terminal"][k]:
            break
        words, n = ev.h.rng_state()
        assert n[1] == int(z["rng_draws"][k]), k
        assert np.array_equal(words[1], python_mt_state(int(z["seed64"]), int(n[1]))), k
    assert z["terminal"][k]
    assert len(noise) <= max(1, len(z["in_action"]) // 3), noise


def test_pool_refusals_leave_the_handle_working(hip_lib):
    from emu_env import emu_lib
    from multi_agent_rl_wrsn_amd import _lib
    _, sc, mc = load_fixture("redundant_m2_deaths")             # 30 nodes: NP 64
    _, big, _ = load_fixture("hanoi1000n50_m3_s1")              # 82 nodes: NP 128
    _, six, _ = load_fixture("six_m1_bs_charge_ongrid")
    _, gsc, _ = load_fixture("prob_gp/redundant_m2_p05")
    ev = PoolEmu([sc, six, sc], mc, 2, 30, 56)
    ev.reset()
    pool = _pool([_record(ev, 0), _record(ev, 1)])
    before = [_peeks(ev, e) for e in range(3)]; rows = [_row(ev, e) for e in range(3)]

    def refused(fn, code, *words):
        with pytest.raises(_lib.WrsnError) as ei:
            fn()
        assert ei.value.code == code, str(ei.value)
        for w in words:
            assert w in str(ei.value), (w, str(ei.value))
        for e in range(3):
            _same(_peeks(ev, e), before[e])
            assert _row(ev, e) == rows[e]

    refused(lambda: _pool_reset(ev, [1, 1, 1], [0, 0, 0]), -5, "pool")                      # no pool yet
    bigh = PoolEmu([big], mc, 2, 82, 56)
    brec = _record(bigh)
    refused(lambda: ev.h.pool_set(brec.ctypes.data, 1, 0), -1, "record 0", "NP")
    bad = _pool([pool[0:1], pool[1:2]]); bad[1, 4] = 7
    refused(lambda: ev.h.pool_set(bad.ctypes.data, 2, 0), -1, "record 1", "version")
    g = PoolEmu([gsc], mc, 2, 30, 56); g.reset()
    grec = _record(g)
    refused(lambda: ev.h.pool_set(grec.ctypes.data, 1, 0), -1, "has_gen")
    with pytest.raises(_lib.WrsnError) as ei:                                            # and the reverse
        g.h.pool_set(pool.ctypes.data, 2, 0)
    assert ei.value.code == -1 and "has_gen" in str(ei.value)
    shifted = np.zeros(pool.size + 32, dtype=np.uint8)
    off = (-shifted.ctypes.data) % 16 + 4
    shifted[off:off + pool.size] = pool.reshape(-1)
    refused(lambda: ev.h.pool_set(shifted.ctypes.data + off, 2, 0), -1, "aligned")
    refused(lambda: _pool_reset(ev, [1, 1, 1], [0, 0, 0]), -5, "pool")                      # none of the refused pools was kept
    # an environment that holds no scenario yet
    empty = _lib.RawHandle(emu_lib(), 2, 30, 56, 2, 100, 100.0)
    agent = np.zeros(2, dtype=np.int32); rw = np.zeros(2); term = np.zeros(2, dtype=np.uint8); now = np.zeros(2); stat = np.zeros(2, dtype=np.int32)
    outp = dict(agent_id=agent.ctypes.data, reward=rw.ctypes.data, terminal=term.ctypes.data, now=now.ctypes.data, status=stat.ctypes.data)
    empty.pool_set(pool.ctypes.data, 2, 0)
    empty.load_envs([1], pool.ctypes.data, **outp)
    with pytest.raises(_lib.WrsnError) as ei:
        empty.pool_reset(0, 0, 0, **outp)
    assert ei.value.code == -5 and "environment 0" in str(ei.value)
    empty.close()
    # a good pool; the aliasing rule
    ev.h.pool_set(pool.ctypes.data, 2, 0)
    refused(lambda: ev.h.pool_reset(0, 0, ev.agent_id.ctypes.data, **ev._ptrs(True)), -1, "agent_id")
    # an index outside the pool: that row is left as it was with the status of the header, the others are swapped
    _fill_sentinels(ev)
    ids = np.array([0, 0, 0], dtype=np.int32)
    _pool_reset(ev, [1, 1, 1], [1, 2, 0], ids)
    assert _lib.STATUS_POOL_INDEX == -5
    assert (int(ev.agent_id[1]), int(ev.status[1]), float(ev.now[1]), int(ev.terminal[1])) == (SENT_I, _lib.STATUS_POOL_INDEX, SENT_F, 99)
    assert np.all(ev.obs[1] == np.float32(SENT_F)) and list(ids) == [-2, 0, -2]
    _same(_peeks(ev, 1), before[1])
    assert _row(ev, 0)[:4] == rows[1][:4] and _row(ev, 2)[:4] == rows[0][:4]
    _same(_peeks(ev, 0), before[1]); _same(_peeks(ev, 2), before[0])
    assert np.array_equal(_pool_info(ev), [[1, 1], [-1, 0], [0, 1]])
    # the handle still steps
    ev.agent_id[1] = rows[1][0]
    ev.step(ev.agent_id.copy(), np.array([[0.5, 0.5, 0.1]] * 3))
    assert all(int(s) in (0, 1) for s in ev.status)
    # clearing the pool
    ev.h.pool_set(0, 0, 0)
    with pytest.raises(_lib.WrsnError) as ei:
        _pool_reset(ev, [1, 1, 1], [0, 0, 0])
    assert ei.value.code == -5


def test_pool_draw_reaches_every_record():
    from multi_agent_rl_wrsn_amd import pool_draw
    P = 7
    for seed in (0, 1, 0xDEADBEEF, 2 ** 64 - 1):
        seen = {pool_draw(seed, e, k, P) for e in range(512) for k in range(4)}
        assert seen == set(range(P)), (seed, seen)
    assert all(0 <= pool_draw(3, e, k, 1) < 1 for e in range(8) for k in range(3))
    # the function as stated, spelled out once for one argument set
    m = 2 ** 64 - 1
    z = ((5 ^ ((3 << 32) | 2)) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    assert pool_draw(5, 3, 2, 11) == ((z >> 32) * 11) >> 32
