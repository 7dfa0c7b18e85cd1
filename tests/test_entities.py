"""Entity observations (wrsn_set_entity_out / wrsn_entities) on the CPU: the unmodified HIP sources in the lockstep wavefront emulator
of tests/emu.  The rows are held to the float64 formula sheet of the header evaluated from wrsn_peek (one float32 ulp), the formulas
to the reference's own get_state images of tests/golden (splatted back into four maps), every path that renders to the standalone
call (bit for bit), and the extent of what a call writes to a byte pattern with guards."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from entity_ref import EntBuf, check_extent, check_rows, peeks, reference, splat

FIXTURES = ("six_m3_zero_length",                 # 6 nodes: far fewer nodes than threads
            "hanoi1000n50_m3_s1",
            "hanoi1000n50_m1_s3",                 # M = 1: no other charger
            "hanoi1000n50_m3_cap1500_mcdeath",    # a dead charger
            "redundant_m2_deaths",                # nodes die while the episode goes on
            "synth300_m3_s27")                    # more nodes than a 256-thread block


def _emu(scenarios, mc, M, **kw):
    from emu_env import EmuVec
    return EmuVec(scenarios, mc, M, **kw)


def _register(ev):
    buf = EntBuf(ev.B, ev.N, ev.M)
    ev.h.set_entity_out(*buf.ptrs())
    return buf


def _standalone(ev, agents):
    """Rows of wrsn_entities for `agents` in buffers of their own."""
    buf = EntBuf(ev.B, ev.N, ev.M)
    a = np.ascontiguousarray(agents, dtype=np.int32)
    ev.h.entities(a.ctypes.data, *buf.ptrs())
    return buf, buf.snap()


def _check_call(ev, buf, rendered, tag):
    """After a call that rendered exactly the rows `rendered`: extent, untouched rows, and bit-equality with the standalone call."""
    snap = buf.snap()
    check_extent(buf, snap, rendered, tag)
    agents = np.array([int(ev.agent_id[e]) if e in rendered else -1 for e in range(ev.B)], dtype=np.int32)
    sbuf, ssnap = _standalone(ev, agents)
    check_extent(sbuf, ssnap, rendered, tag + " (standalone)")
    for e in rendered:
        assert np.array_equal(buf.row_bytes(snap, e), sbuf.row_bytes(ssnap, e)), (tag, "row %d differs from wrsn_entities" % e)
    return snap


_REPLAY = {}


def _replay(name):
    """The fixture's scripted actions through an entity-only handle (out->obs NULL).  Per request with agent_id >= 0 (the reset's
    included): the decision index (-1: reset), the rows the call wrote and the float64 reference rows.  Computed once per fixture."""
    if name in _REPLAY:
        return _REPLAY[name]
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    z = load_golden(name)
    sc, mc = scenario_from_golden(z)
    M = int(z["num_agent"])
    ev = _emu([sc], mc, M, map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    buf = _register(ev)
    out = []

    def record(k):
        a = int(ev.agent_id[0])
        snap = _check_call(ev, buf, {0}, "%s decision %d" % (name, k))
        out.append({"k": k, "agent": a, "got": tuple(x.copy() for x in buf.rows(snap, 0)),
                    "ref": reference(peeks(ev.h), 0, a, sc, mc, ev.N, M), "terminal": bool(ev.terminal[0])})

    ev.reset(with_obs=False)
    record(-1)
    for k in range(len(z["in_action"])):
        buf.fill()
        ev.step([int(z["in_agent"][k])], z["in_action"][k][None], with_obs=False)
        if z["is_none"][k] or int(ev.agent_id[0]) < 0:
            check_extent(buf, buf.snap(), set(), "%s decision %d renders nothing" % (name, k))
            break
        record(k)
    _REPLAY[name] = (z, sc, out)
    return _REPLAY[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_values_on_fixtures(name):
    z, sc, recs = _replay(name)
    assert len(recs) >= 2
    for r in recs:
        check_rows(r["got"], r["ref"], sc.n_node, "%s decision %d" % (name, r["k"]))
    nodes = np.stack([r["ref"][0] for r in recs])
    if name == "redundant_m2_deaths":
        assert (nodes[:, :, 7] == 0).any() and (nodes[-1, :, 6] != nodes[0, :, 6]).any(), "dead-node rows and level changes should appear"
    if name == "hanoi1000n50_m3_cap1500_mcdeath":
        assert any((r["ref"][1][:, 4] == 0).any() for r in recs), "a dead charger should appear"


@pytest.mark.parametrize("name", FIXTURES)
def test_features_are_what_get_state_draws(name):
    """The float64 feature values of the formula sheet, splatted with the reference's func and the bandwidths of the environment row,
    are the reference's observation: reset_obs, obs_full[k] and the strided obs_sample[k] at 1e-5 of the map's peak."""
    z, sc, recs = _replay(name)
    G, s = int(z["map_size"]), int(z["obs_stride"])
    full = 0
    for r in recs:
        k = r["k"]
        if k >= 0 and (r["terminal"] or np.isinf(z["reward"][k]) or int(z["agent_id"][k]) < 0):
            continue                                          # what the existing observation tests skip
        maps = splat(*r["ref"], G)
        if k < 0 or k < z["obs_full"].shape[0]:
            ref = z["reset_obs"] if k < 0 else z["obs_full"][k]
            assert np.max(np.abs(maps - ref)) <= 1e-5 * max(1.0, float(np.abs(ref).max())), (name, k, "full map")
            full += 1
        if k >= 0:
            ref = z["obs_sample"][k]
            assert np.max(np.abs(maps[:, ::s, ::s] - ref)) <= 1e-5 * max(1.0, float(np.nanmax(np.abs(ref)))), (name, k, "sample")
    assert full >= 1


# ---------------------------------------------------------------------------------------------------------------------------
def _batch(map_size=8):
    """Five small networks, two chargers; the nodes of environment 2 hold little energy: its episodes end within a few steps (terminal rows)."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, DEFAULT_NODE_SPEC, synth_scenario
    weak = dict(DEFAULT_NODE_SPEC, capacity=1200.0)          # little above the threshold: the first node dies within a few steps
    scs = [synth_scenario(31 + e, 40, 30, node_spec=(weak if e == 2 else None)) for e in range(5)]
    return scs, DEFAULT_MC_SPEC, _emu(scs, DEFAULT_MC_SPEC, 2, map_size=map_size)


def _drive(ev, buf, calls, with_obs, seen, tag):
    """`calls` step calls with auto-reset; row 1 is left alone (-2) in every other call.  Every call is checked."""
    rng = np.random.RandomState(11)
    for c in range(calls):
        ids = ev.agent_id.copy()
        ids[ev.status == 4] = -1
        skip = c % 2 == 1
        if skip:
            ids[1] = -2
        before = ev.agent_id.copy()
        buf.fill()
        ev.step(ids, rng.rand(ev.B, 3), with_obs=with_obs, auto_reset=True)
        rendered = set()
        for e in range(ev.B):
            if skip and e == 1:
                assert int(ev.agent_id[e]) == int(before[e])
                seen.add("-2")
            elif int(ev.status[e]) == 4:
                seen.add("status 4")
            elif ev.terminal[e]:
                seen.add("terminal")
            elif int(ev.agent_id[e]) >= 0:
                rendered.add(e); seen.add("rendered")
        _check_call(ev, buf, rendered, "%s call %d" % (tag, c))


def test_blocking_steps_and_a_masked_reset_write_the_rendered_rows_only(hip_lib):
    scs, mc, ev = _batch()
    buf = _register(ev)
    mask = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    ev.h.reset(mask.ctypes.data, **ev._ptrs(True))
    _check_call(ev, buf, {0, 2, 3}, "masked reset")
    buf.fill()
    ev.reset()
    snap = _check_call(ev, buf, set(range(5)), "reset")
    pk = peeks(ev.h)
    for e in range(5):
        check_rows(buf.rows(snap, e), reference(pk, e, int(ev.agent_id[e]), scs[e], mc, ev.N, 2), scs[e].n_node, "reset row %d" % e)
    seen = set()
    _drive(ev, buf, 12, True, seen, "blocking")
    assert {"-2", "terminal", "rendered"} <= seen, seen


def test_step_budget_leaves_rows_in_flight_untouched(hip_lib):
    scs, mc, ev = _batch()
    buf = _register(ev)
    ev.h.set_step_budget(40)
    ev.reset(with_obs=False)
    seen = set()
    _drive(ev, buf, 24, False, seen, "budget 40")
    assert {"-2", "status 4", "rendered"} <= seen, seen


def test_time_sliced_launches_write_the_rendered_rows_only(hip_lib):
    scs, mc, ev = _batch()
    buf = _register(ev)
    ev.h.set_step_budget(100000)
    ev.h.set_step_deadline(1)                                 # 100 readings of the emulator's stand-in clock
    ev.reset(with_obs=False)
    seen = set()
    _drive(ev, buf, 24, False, seen, "time slices")
    assert {"-2", "status 4", "rendered"} <= seen, seen


def test_load_clone_and_pool_reset_write_the_replaced_rows_only(hip_lib):
    from test_scenario_pool import _aligned
    scs, mc, ev = _batch()
    buf = _register(ev)
    ev.reset(with_obs=False)
    rng = np.random.RandomState(4)
    for _ in range(3):
        ev.step(np.where(ev.agent_id >= 0, ev.agent_id, -2).astype(np.int32), rng.rand(5, 3), with_obs=False)   # a finished row is left alone
    assert (ev.agent_id[[0, 3]] >= 0).all()
    rec = _aligned((2, ev.h.env_record_bytes()))
    p = ev._ptrs(False); p.pop("obs")
    ev.h.save_envs(np.array([0, 3], dtype=np.int32), rec.ctypes.data, **p)
    # load: records of environments 0 and 3 into 1 and 4
    buf.fill()
    ev.h.load_envs(np.array([1, 4], dtype=np.int32), rec.ctypes.data, **ev._ptrs(False))
    snap = _check_call(ev, buf, {1, 4}, "load")
    pk = peeks(ev.h)
    for dst, src in ((1, 0), (4, 3)):
        check_rows(buf.rows(snap, dst), reference(pk, dst, int(ev.agent_id[dst]), scs[src], mc, ev.N, 2), scs[src].n_node, "loaded row %d" % dst)
    # clone: 0 -> 2 (with the image this time)
    buf.fill()
    ev.h.clone_envs([0], [2], **ev._ptrs(True))
    _check_call(ev, buf, {2}, "clone")
    # pool reset: rows 1 and 3 by mask, records chosen by the caller
    ev.h.pool_set(rec.ctypes.data, 2, 5)
    mask = np.array([0, 1, 0, 1, 0], dtype=np.uint8); index = np.array([9, 1, 9, 0, 9], dtype=np.int32)
    buf.fill()
    ev.h.pool_reset(mask.ctypes.data, index.ctypes.data, 0, **ev._ptrs(False))
    _check_call(ev, buf, {1, 3}, "pool reset")


def test_ragged_batch_values_and_zero_rows():
    """six_* (6 nodes) and hanoi1000n50 (82 nodes) in one handle: rows beyond each n_node are written as zeros."""
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    six, _ = scenario_from_golden(load_golden("six_m3_zero_length"))
    hanoi, mc = scenario_from_golden(load_golden("hanoi1000n50_m3_s1"))
    scs = [six, hanoi]
    ev = _emu(scs, mc, 3, map_size=8)
    assert ev.N == 82 and six.n_node == 6
    buf = _register(ev)
    ev.reset(with_obs=False)
    rng = np.random.RandomState(2)
    checked = 0
    for c in range(4):
        snap = buf.snap(); pk = peeks(ev.h)
        for e in range(2):
            if ev.agent_id[e] < 0:
                continue
            rows = buf.rows(snap, e)
            check_rows(rows, reference(pk, e, int(ev.agent_id[e]), scs[e], mc, ev.N, 3), scs[e].n_node, "ragged call %d row %d" % (c, e))
            assert not rows[0][scs[e].n_node:].any()
            checked += 1
        ids = np.where(ev.agent_id >= 0, ev.agent_id, -2).astype(np.int32)
        ev.step(ids, rng.rand(2, 3), with_obs=False)
    assert checked >= 6


def test_entity_only_calls_unregistering_and_identical_requests(hip_lib):
    """out->obs NULL with entities registered writes the rows; after wrsn_set_entity_out(h, NULL) the same calls write nothing into
    the buffers that were registered; the requests do not depend on entities being registered."""
    scs, mc, ev = _batch()
    _, _, plain = _batch()
    buf = _register(ev)
    rng = np.random.RandomState(8)
    hist = []
    for c in range(10):
        act = rng.rand(5, 3)
        for v in (ev, plain):
            if c == 0:
                v.reset(with_obs=False)
            else:
                v.step(v.agent_id.copy(), act, with_obs=False, auto_reset=True)
        for k in ("agent_id", "reward", "now", "terminal", "status"):
            assert getattr(ev, k).tobytes() == getattr(plain, k).tobytes(), (c, k)
        hist.append(ev.agent_id.copy())
    snap = buf.snap()
    assert any(buf.full(snap, e) for e in range(5))
    ev.h.set_entity_out()                                     # off
    buf.fill()
    ev.reset(with_obs=False)
    ev.step(ev.agent_id.copy(), rng.rand(5, 3), with_obs=False, auto_reset=True)
    ev.h.clone_envs([0], [1], **ev._ptrs(False))
    check_extent(buf, buf.snap(), set(), "unregistered")
    assert (ev.agent_id >= 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
def test_entity_struct_matches_the_header():
    from multi_agent_rl_wrsn_amd import _lib
    text = open(os.path.join(ROOT, "include", "wrsn_hip.h")).read()
    m = re.search(r"typedef struct wrsn_entity_out \{(.*?)\} wrsn_entity_out;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    members = re.findall(r"float\s*\*\s*(\w+)\s*;", body)
    assert members == [n for n, _ in _lib.WrsnEntityOut._fields_] == ["node", "mc", "env"]
    assert C.sizeof(_lib.WrsnEntityOut) == 3 * C.sizeof(C.c_void_p)
    for name, want in (("WRSN_ENT_NODE_F", _lib.ENT_NODE_F), ("WRSN_ENT_MC_F", _lib.ENT_MC_F), ("WRSN_ENT_ENV_F", _lib.ENT_ENV_F)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, text).group(1)) == want
    assert len(_lib.ENT_NODE_FIELDS) == 8 and len(_lib.ENT_MC_FIELDS) == 12 and len(_lib.ENT_ENV_FIELDS) == 8
    assert {"wrsn_set_entity_out", "wrsn_entities"} <= set(_lib.EXPORTS)
    import multi_agent_rl_wrsn_amd as pkg
    assert pkg.ENT_NODE["weight"] == 2 and pkg.ENT_MC["move_time"] == 9 and pkg.ENT_ENV["n_node"] == 5


def test_bad_entity_structs_are_refused_and_change_nothing(hip_lib):
    from multi_agent_rl_wrsn_amd import _lib
    scs, mc, ev = _batch()
    buf = _register(ev)
    node, mcp, envp = buf.ptrs()
    ids = np.zeros(5, dtype=np.int32)
    for bad in ((node + 4, mcp, envp), (node, mcp + 8, envp), (node, mcp, envp + 2), (0, mcp, envp), (node, 0, envp), (node, mcp, 0)):
        with pytest.raises(_lib.WrsnError) as ei:
            ev.h.set_entity_out(*bad)
        assert ei.value.code == -1
        with pytest.raises(_lib.WrsnError) as ei:
            ev.h.entities(ids.ctypes.data, *bad)
        assert ei.value.code == -1
    check_extent(buf, buf.snap(), set(), "refused calls")
    ev.reset(with_obs=False)                                  # the handle still holds the buffers registered first
    check_extent(buf, buf.snap(), set(range(5)), "after refusals")
