"""Environment records (wrsn_save_envs / wrsn_load_envs / wrsn_clone_envs) on the CPU: the unmodified HIP sources in the lockstep
wavefront emulator of tests/emu.  A restored environment continues exactly as the source would have: against the reference runs of
tests/golden, against Python's `random` for prob_gp < 1, and against an untouched twin."""
import numpy as np
import pytest

from parity import check_decision
from sides import EmuSide, load_fixture, python_mt_state


def _row(ev, e):
    return (int(ev.agent_id[e]), float(ev.now[e]), float(ev.reward[e]), int(ev.terminal[e]), int(ev.status[e]))


def _peeks(ev, e, sc=None):
    """Everything the handle reports about environment e (node / target arrays cut to those of scenario sc when given)."""
    from multi_agent_rl_wrsn_amd import _lib
    nd = ev.nodes()
    n, t = (sc.n_node, sc.n_target) if sc is not None else (ev.N, ev.T)
    out = {k: v[e][:n].copy() for k, v in nd.items()}
    out["mc"] = ev.h.peek(_lib.PEEK_MC)[e].copy()
    out["env"] = ev.h.peek(_lib.PEEK_ENV)[e].copy()
    out["targets"] = ev.targets_active()[e][:t].copy()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _save(ev, envs):
    rec = np.zeros((len(envs), ev.h.env_record_bytes()), dtype=np.uint8)
    p = ev._ptrs(False); p.pop("obs")
    ev.h.save_envs(np.asarray(envs, dtype=np.int32), rec.ctypes.data, **p)
    return rec


def _load(ev, envs, rec, with_obs=True):
    ev.h.load_envs(np.asarray(envs, dtype=np.int32), rec.ctypes.data, **ev._ptrs(with_obs))


# (fixture, another scenario of the same NP / TP class that the destination handle is built with)
RESUME = [("hanoi1000n50_m1_s3", "sonla1000n50_m2_s4"),            # M = 1
          ("redundant_m2_deaths", "six_m1_bs_charge_ongrid"),       # M = 2, node deaths
          ("hanoi1000n50_m3_s1", "sonla1000n50_m2_s4"),             # M = 3
          ("six_m3_bs_charge_ongrid", "redundant_m2_map64"),        # bs_charge_ongrid, a 6-node record in a 30-node handle
          ("prob_gp/redundant_m2_p05", "prob_gp/redundant_rev_m2_p05")]


@pytest.mark.parametrize("name,other", RESUME)
def test_resume_from_a_record_matches_the_reference(hip_lib, name, other):
    """Replay the fixture to its middle decision, save, load into environment 0 of a handle built with another scenario, and continue:
    every later decision still matches the reference run (and, for prob_gp < 1, the generator matches Python's word for word)."""
    from multi_agent_rl_wrsn_amd import _lib
    z, sc, mc = load_fixture(name)
    _, sc2, _ = load_fixture(other)
    M = int(z["num_agent"]); kw = dict(map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    K = len(z["in_action"]); mid = K // 2
    src = EmuSide([sc], mc, M, **kw)
    src.reset()
    for k in range(mid):
        src.step([int(z["in_agent"][k])], z["in_action"][k][None])
    rec = _save(src, [0])
    row0, obs0 = _row(src, 0), src.obs[0].copy()
    dst = EmuSide([sc2, sc], mc, M, **kw)                        # N, T: the larger of the two scenarios -- same NP and TP as the source's
    assert dst.h.env_record_bytes() == src.h.env_record_bytes()
    dst.reset()
    _load(dst, [0], rec)
    assert _row(dst, 0) == row0
    if row0[0] >= 0:
        assert np.array_equal(dst.obs[0], obs0)
    _same(_peeks(dst, 0, sc), _peeks(src, 0, sc))
    stoch = name.startswith("prob_gp/")
    noise = []
    for k in range(mid, K):
        dst.step([int(z["in_agent"][k]), -2], np.stack([z["in_action"][k], z["in_action"][k]]))
        if z["is_none"][k]:
            assert int(dst.status[0]) == 1 and int(dst.agent_id[0]) == -1
            break
        check_decision(z, k, dst.decision(0, sc), where=name, noise=noise)
        if stoch and not z["terminal"][k]:
            words, n = dst.h.rng_state()
            assert n[0] == int(z["rng_draws"][k]), (name, k)
            assert np.array_equal(words[0], python_mt_state(int(z["seed64"]), int(n[0]))), (name, k)
        if z["terminal"][k]:
            break
    assert len(noise) <= max(1, K // 3), noise


def test_clone_within_a_handle_follows_the_source_and_leaves_it_alone(hip_lib):
    z, sc, mc = load_fixture("hanoi1000n50_m3_s1")
    _, sc2, _ = load_fixture("sonla1000n50_m2_s4")
    M = 3
    ev = EmuSide([sc, sc2, sc2], mc, M)
    twin = EmuSide([sc], mc, M)
    ev.reset(); twin.reset()
    for k in range(4):
        a = int(z["in_agent"][k])
        ev.step([a, -1, -2], np.stack([z["in_action"][k]] * 3)); twin.step([a], z["in_action"][k][None])
        assert _row(ev, 0) == _row(twin, 0)
    ev.h.clone_envs([0, 0], [1, 2], **ev._ptrs(True))
    assert _row(ev, 1) == _row(ev, 0) == _row(ev, 2)
    assert np.array_equal(ev.obs[1], ev.obs[0]) and np.array_equal(ev.obs[2], ev.obs[0])
    _same(_peeks(ev, 1, sc), _peeks(ev, 0, sc))
    rng = np.random.RandomState(3)
    for k in range(6):
        act = rng.rand(3) * np.array([1.0, 1.0, 0.4])
        ids = ev.agent_id.copy()
        other = np.array([1.0, 0.0, 0.4]) - act * np.array([1.0, 1.0, 0.0])   # a different action for environment 2
        ev.step(ids, np.stack([act, act, other])); twin.step(twin.agent_id.copy(), act[None])
        assert _row(ev, 0) == _row(ev, 1) == _row(twin, 0), k
        assert np.array_equal(ev.obs[0], ev.obs[1]) and np.array_equal(ev.obs[0], twin.obs[0])
        _same(_peeks(ev, 1, sc), _peeks(ev, 0, sc))
        _same(_peeks(ev, 0, sc), _peeks(twin, 0, sc))
        if ev.terminal[0] or ev.agent_id[0] < 0:
            break
    assert _row(ev, 2) != _row(ev, 0) or not np.array_equal(ev.nodes()["energy"][2], ev.nodes()["energy"][0])


def test_reset_and_auto_reset_after_a_load_restore_the_sources_warm_up(hip_lib):
    z, sc, mc = load_fixture("redundant_m2_deaths")
    _, sc2, _ = load_fixture("six_m1_bs_charge_ongrid")
    M = 2
    fresh = EmuSide([sc], mc, M)
    fresh.reset()
    want = _peeks(fresh, 0, sc); want_row = _row(fresh, 0); want_obs = fresh.obs[0].copy()
    src = EmuSide([sc], mc, M)
    src.reset()
    term_k = int(np.argmax(z["terminal"]))
    for k in range(term_k + 1):
        src.step([int(z["in_agent"][k])], z["in_action"][k][None])
    assert src.terminal[0] == 1
    rec = _save(src, [0])
    for auto in (False, True):
        dst = EmuSide([sc, sc2], mc, M)                         # environment 1 was built with the six-node network
        dst.reset()
        _load(dst, [1], rec)
        assert dst.terminal[1] == 1
        if auto:
            dst.step([-1, -1], np.zeros((2, 3)), auto_reset=True)
            assert int(dst.status[1]) == 3
        else:
            dst.reset()
        assert _row(dst, 1)[:4] == want_row[:4]
        assert np.array_equal(dst.obs[1], want_obs)
        _same(_peeks(dst, 1, sc), want)


def _raw(lib, scenarios, mc, M, N=None, T=None, warm_up_time=100.0):
    from multi_agent_rl_wrsn_amd import _lib
    h = _lib.RawHandle(lib, len(scenarios), N or max(s.n_node for s in scenarios), T or max(s.n_target for s in scenarios), M, 100, warm_up_time)
    h.set_scenarios(scenarios, mc)
    return h


def test_refusals_change_nothing(hip_lib):
    from emu_env import emu_lib
    from multi_agent_rl_wrsn_amd import _lib
    lib = emu_lib()
    _, sc, mc = load_fixture("redundant_m2_deaths")             # 30 nodes: NP 64
    _, big, _ = load_fixture("hanoi1000n50_m3_s1")              # 82 nodes: NP 128
    _, six, _ = load_fixture("six_m1_bs_charge_ongrid")
    _, gsc, _ = load_fixture("prob_gp/redundant_m2_p05")
    _, gsc2, _ = load_fixture("prob_gp/redundant_rev_m2_p05")
    ev = EmuSide([sc, six, sc], mc, 2)
    ev.reset()
    rec = _save(ev, [0, 1])
    before = [_peeks(ev, e) for e in range(3)]; rows = [_row(ev, e) for e in range(3)]

    def refused(fn, *words):
        with pytest.raises(_lib.WrsnError) as ei:
            fn()
        assert ei.value.code == -1
        for w in words:
            assert w in str(ei.value), (w, str(ei.value))
        for e in range(3):
            _same(_peeks(ev, e), before[e])
            assert _row(ev, e) == rows[e]

    bigh = EmuSide([big], mc, 2)
    brec = _save(bigh, [0])
    refused(lambda: _load(ev, [0], brec), "NP")
    h3 = EmuSide([sc], mc, 3); r3 = _save(h3, [0])
    refused(lambda: _load(ev, [2], r3), "M")
    bad = rec.copy(); bad[0, 0] ^= 0x55
    refused(lambda: _load(ev, [0, 1], bad), "magic")
    bad = rec.copy(); bad[1, 4] = 7                          # record 1: every header is checked before anything changes
    refused(lambda: _load(ev, [0, 1], bad), "record 1", "version")
    refused(lambda: _load(ev, [0, 3], rec), "out of range")
    refused(lambda: _load(ev, [2, 2], rec), "twice")
    refused(lambda: ev.h.clone_envs([0, 1], [1, 2], **ev._ptrs(True)), "also a source")
    refused(lambda: ev.h.clone_envs([0], [-1], **ev._ptrs(True)), "out of range")
    g = EmuSide([gsc, gsc2], mc, 2); g.reset()
    grec = _save(g, [0])
    refused(lambda: _load(ev, [0], grec), "has_gen")      # generator record -> a handle without generators that holds a scenario
    before_g = _peeks(g, 1); st_g = g.h.peek(_lib.PEEK_RNG_STATE).copy()
    with pytest.raises(_lib.WrsnError) as ei:               # and the reverse
        _load(g, [1], rec[:1].copy())
    assert "has_gen" in str(ei.value)
    _same(_peeks(g, 1), before_g)
    assert np.array_equal(g.h.peek(_lib.PEEK_RNG_STATE), st_g)
    # a handle that holds no scenario yet takes a generator record and turns stochastic
    empty = _lib.RawHandle(lib, 2, 30, 56, 2, 100, 100.0)
    with pytest.raises(_lib.WrsnError):
        empty.peek(_lib.PEEK_RNG_STATE)
    agent = np.zeros(2, dtype=np.int32); rw = np.zeros(2); term = np.zeros(2, dtype=np.uint8); now = np.zeros(2); stat = np.zeros(2, dtype=np.int32)
    empty.load_envs([1], grec.ctypes.data, agent_id=agent.ctypes.data, reward=rw.ctypes.data, terminal=term.ctypes.data, now=now.ctypes.data,
                    status=stat.ctypes.data)
    assert np.array_equal(empty.peek(_lib.PEEK_RNG_STATE)[1], g.h.peek(_lib.PEEK_RNG_STATE)[0])
    assert (int(agent[1]), float(now[1])) == (int(g.agent_id[0]), float(g.now[0]))
    with pytest.raises(_lib.WrsnError) as ei:               # environment 0 of that handle holds nothing to save
        empty.save_envs([0], grec.ctypes.data, agent_id=agent.ctypes.data, reward=rw.ctypes.data, terminal=term.ctypes.data,
                        now=now.ctypes.data, status=stat.ctypes.data)
    assert "holds no scenario" in str(ei.value)
    empty.close()


def test_ragged_record_round_trips(hip_lib):
    """A 50-node environment saved from a 200-node handle, loaded into another 200-node handle, saved again and loaded back:
    every step that follows is bit-identical to the original's."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    small, large = synth_scenario(11, 50, 40), synth_scenario(12, 200, 200)
    kw = dict(warm_up_time=5.0)
    a = EmuSide([small, large], DEFAULT_MC_SPEC, 2, **kw); b = EmuSide([large], DEFAULT_MC_SPEC, 2, **kw)
    a.reset(); b.reset()
    rng = np.random.RandomState(1)
    act = rng.rand(2, 3) * np.array([1.0, 1.0, 0.3])
    a.step([int(a.agent_id[0]), -2], act)
    rec = _save(a, [0])
    b.h.load_envs([0], rec.ctypes.data, **b._ptrs(True))
    rec2 = _save(b, [0])
    c = EmuSide([large, large], DEFAULT_MC_SPEC, 2, **kw); c.reset()
    _load(c, [1], rec2)
    for k in range(3):
        act = rng.rand(3) * np.array([1.0, 1.0, 0.3])
        a.step([int(a.agent_id[0]), -2], np.stack([act, act])); b.step([int(b.agent_id[0])], act[None])
        c.step([-2, int(c.agent_id[1])], np.stack([act, act]))
        assert _row(a, 0) == _row(b, 0) == _row(c, 1), k
        assert np.array_equal(a.obs[0], b.obs[0]) and np.array_equal(a.obs[0], c.obs[1])
        _same(_peeks(a, 0, small), _peeks(b, 0, small)); _same(_peeks(a, 0, small), _peeks(c, 1, small))
        if a.terminal[0] or a.agent_id[0] < 0:
            break


def test_record_format_version_1_is_pinned(hip_lib):
    """The size and segment count of a record are part of format version 1: literals measured when the format was introduced (one
    environment, one charger, default max_degree / max_cover), not computed by the library under test.  A per-environment array added to
    or dropped from a handle changes them, and then needs a new WRSN_REC_VERSION."""
    import struct
    for name, nbytes, has_gen, nseg in (("hanoi1000n50_m1_warmup10", 116480, 0, 43),                  # 82 nodes, 50 targets: NP 128, TP 64
                                        ("prob_gp/hanoi1000n50_m1_warmup10_p05", 123648, 1, 48)):     # + the generator block
        z, sc, mc = load_fixture(name)
        assert (sc.n_node, sc.n_target, int(z["num_agent"])) == (82, 50, 1), name
        ev = EmuSide([sc], mc, 1, map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
        assert ev.h.env_record_bytes() == nbytes, name
        rec = _save(ev, [0])
        assert rec.shape == (1, nbytes), name
        magic, version = struct.unpack_from("<II", rec[0].tobytes(), 0)
        assert (magic, version) == (0x52534E57, 1), name
        assert struct.unpack_from("<iiq", rec[0].tobytes(), 48) == (has_gen, nseg, nbytes), name


def clone_skips_the_request_fields_the_caller_leaves_out(Side):
    """wrsn_clone_envs with NULL fields in `out` (wrsn_rec_rows_kernel: "NULL fields of `out` are skipped"): the environment is copied
    whatever rows are given; a row that is given follows the source, one that is not keeps every byte -- here and on the device (the
    body runs there from tests/test_env_records_gpu.py).  The reference is the numpy copy of the rows."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(48000 + e, 30, 20) for e in range(4)]
    side = Side(scs, DEFAULT_MC_SPEC, 2, map_size=8, render=False)
    side.reset()
    rng = np.random.RandomState(48)
    for _ in range(2):
        side.step(side._host()["agent_id"], rng.rand(4, 3) * [1.0, 1.0, 0.02])
    before = side._host(); nodes = side.nodes()["energy"].copy()
    assert len({float(before["now"][e]) for e in range(4)}) == 4 and not np.array_equal(nodes[0], nodes[2])   # the rows and states differ
    ptrs = side.out_ptrs()
    given = ("agent_id", "terminal", "status")
    side.handle.clone_envs([0, 1], [2, 3], **{k: (v if k in given else 0) for k, v in ptrs.items()})
    side.handle.sync()
    after = side._host(); got = side.nodes()["energy"]
    for k in before:
        want = before[k].copy()
        if k in given:
            want[2:] = before[k][:2]
        assert np.array_equal(after[k], want), (k, after[k], want)
    assert np.array_equal(got[2:], nodes[:2]) and np.array_equal(got[:2], nodes[:2])
    # the other way round: only the clock and the reward follow
    side.handle.clone_envs([3], [0], **{k: (v if k in ("now", "reward") else 0) for k, v in ptrs.items()})
    side.handle.sync()
    last = side._host()
    for k in after:
        want = after[k].copy()
        if k in ("now", "reward"):
            want[0] = after[k][3]
        assert np.array_equal(last[k], want), (k, last[k], want)
    assert np.array_equal(side.nodes()["energy"][0], nodes[1])
    side.close()


def test_emulated_clone_skips_the_request_fields_the_caller_leaves_out(hip_lib):
    clone_skips_the_request_fields_the_caller_leaves_out(EmuSide)
