"""Entity observations (wrsn_set_entity_out / wrsn_entities), one body each, run here on the emulator (the unmodified HIP sources in
the lockstep wavefront emulator of tests/emu) and by tests/test_entities_gpu.py on the device.  The rows are held to the float64 formula sheet of the header
evaluated from wrsn_peek (one float32 ulp), the formulas to the reference's own get_state images of tests/golden (splatted back into
four maps), every path that renders to the standalone call (bit for bit: the rendered rows, and the whole buffers with their guards),
and the extent of what a call writes to a byte pattern with guards.  CPU only: the header, the refusals and the splat.  Helpers and tolerances: tests/entity_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from entity_ref import check_extent, check_rows, peeks, reference, splat
from sides import EmuSide, load_fixture

FIXTURES = ("six_m3_zero_length",                 # 6 nodes: far fewer nodes than threads
            "hanoi1000n50_m3_s1",
            "hanoi1000n50_m1_s3",                 # M = 1: no other charger
            "hanoi1000n50_m3_cap1500_mcdeath",    # a dead charger
            "redundant_m2_deaths",                # nodes die while the episode goes on
            "synth300_m3_s27")                    # more nodes than a 256-thread block
# What differs between the sides is size: the emulator draws 8 x 8 images and drives a fixed number of calls; the device draws 16 x 16
# (100 x 100 where no image is asked for) and drives until every kind of row occurred, at least 9 calls.
BATCH_G = {"emu": 8, "gpu": 16}
NO_IMAGE_G = {"emu": 8, "gpu": 100}
DRIVE = {"blocking": {"emu": (12, 12), "gpu": (40, 9)}, "budget 40": {"emu": (24, 24), "gpu": (60, 9)},
         "time slices": {"emu": (24, 24), "gpu": (300, 9)}}     # side -> (most calls, least calls)
# the emulator clones with the image (its per-call switch; VecWRSN renders what its constructor says)
CLONE_KW = {"emu": dict(with_obs=True), "gpu": {}}


def _registered(side):
    buf = side.entity_buffers()
    side.set_entity_out(buf)
    return buf


def _agents(side):
    return np.array([r[0] for r in side.rows()], dtype=np.int32)


def _check_call(side, buf, rendered, tag):
    """After a call that rendered exactly the rows `rendered`: extent, untouched rows, and bit-equality with the standalone call -- of
    the rendered rows and of the whole buffers, guards included."""
    snap = buf.snap()
    check_extent(buf, snap, rendered, tag)
    agents = np.where([e in rendered for e in range(side.B)], _agents(side), -1)
    sbuf = side.entity_buffers()
    side.entities(agents, sbuf)
    ssnap = sbuf.snap()
    check_extent(sbuf, ssnap, rendered, tag + " (standalone)")
    for e in rendered:
        assert np.array_equal(buf.row_bytes(snap, e), sbuf.row_bytes(ssnap, e)), (tag, "row %d differs from wrsn_entities" % e)
    for k in snap:
        assert np.array_equal(snap[k], ssnap[k]), (tag, k, "buffers differ from wrsn_entities")
    return snap


_REPLAY = {}


def _replay(Side, name):
    """The fixture's scripted actions through an entity-only handle (no image).  Per request with agent_id >= 0 (the reset's included):
    the decision index (-1: reset), the rows the call wrote and the float64 reference rows.  Computed once per side and fixture."""
    if (Side.name, name) in _REPLAY:
        return _REPLAY[Side.name, name]
    z, sc, mc = load_fixture(name)
    M = int(z["num_agent"])
    side = Side([sc], mc, M, map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]), render=False)
    buf = _registered(side)
    out = []

    def record(k):
        a, _, _, terminal, _ = side.rows()[0]
        snap = _check_call(side, buf, {0}, "%s decision %d" % (name, k))
        out.append({"k": k, "agent": a, "got": tuple(x.copy() for x in buf.rows(snap, 0)),
                    "ref": reference(peeks(side.handle), 0, a, sc, mc, side.N, M), "terminal": bool(terminal)})

    side.reset()
    record(-1)
    for k in range(len(z["in_action"])):
        buf.fill()
        side.step([int(z["in_agent"][k])], z["in_action"][k][None])
        if z["is_none"][k] or side.rows()[0][0] < 0:
            check_extent(buf, buf.snap(), set(), "%s decision %d renders nothing" % (name, k))
            break
        record(k)
    side.close()
    _REPLAY[Side.name, name] = (z, sc, out)
    return _REPLAY[Side.name, name]


def values_on_fixtures(Side, name):
    z, sc, recs = _replay(Side, name)
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
    z, sc, recs = _replay(EmuSide, name)
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
def _batch():
    """Five small networks for two chargers; the nodes of environment 2 hold little energy: its episodes end within a few steps
    (terminal rows)."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, DEFAULT_NODE_SPEC, synth_scenario
    weak = dict(DEFAULT_NODE_SPEC, capacity=1200.0)          # little above the threshold: the first node dies within a few steps
    scs = [synth_scenario(31 + e, 40, 30, node_spec=(weak if e == 2 else None)) for e in range(5)]
    return scs, DEFAULT_MC_SPEC


def _time_sliced_batch(side_name):
    """(networks, chargers, launch keywords): the emulator slices the small batch after 100 readings of its stand-in clock, the device
    eight 200-node networks after 50 us."""
    from multi_agent_rl_wrsn_amd import synth_scenario
    if side_name == "emu":
        return _batch()[0], 2, dict(step_budget=100000, step_deadline_us=1)
    return [synth_scenario(500 + e, 200, 200) for e in range(8)], 3, dict(step_deadline_us=50)


def _batch_side(Side, render=False, **kw):
    scs, mc = _batch()
    return scs, mc, Side(scs, mc, 2, map_size=(BATCH_G if render else NO_IMAGE_G)[Side.name], render=render, **kw)


def _rendered(rows, touched):
    return {e for e in touched if rows[e][4] != 4 and not rows[e][3] and rows[e][0] >= 0}


def _drive(side, buf, need, tag):
    """Step calls with auto-reset until every kind of row in `need` occurred (DRIVE: most and least calls); row 1 is left alone (-2) in
    every other call.  Every call is checked."""
    calls, least = DRIVE[tag][side.name]
    rng = np.random.RandomState(11)
    seen = set()
    for c in range(calls):
        before = side.rows()
        ids = np.array([-1 if r[4] == 4 else r[0] for r in before], dtype=np.int32)
        skip = c % 2 == 1
        if skip:
            ids[1] = -2
        buf.fill()
        side.step(ids, rng.rand(side.B, 3))
        rows = side.rows()
        touched = [e for e in range(side.B) if not (skip and e == 1)]
        if skip:
            assert rows[1][0] == before[1][0]
            seen.add("-2")
        for e in touched:
            if rows[e][4] == 4:
                seen.add("status 4")
            elif rows[e][3]:
                seen.add("terminal")
        rendered = _rendered(rows, touched)
        if rendered:
            seen.add("rendered")
        _check_call(side, buf, rendered, "%s call %d" % (tag, c))
        if need <= seen and c + 1 >= least:
            break
    assert need <= seen, (tag, seen)


def blocking_steps_and_a_masked_reset(Side):
    scs, mc, side = _batch_side(Side, render=True, auto_reset=True)
    buf = _registered(side)
    side.reset([1, 0, 1, 1, 0])
    _check_call(side, buf, {0, 2, 3}, "masked reset")
    buf.fill()
    side.reset()
    snap = _check_call(side, buf, set(range(5)), "reset")
    pk = peeks(side.handle); agents = _agents(side)
    for e in range(5):
        check_rows(buf.rows(snap, e), reference(pk, e, int(agents[e]), scs[e], mc, side.N, 2), scs[e].n_node, "reset row %d" % e)
    _drive(side, buf, {"-2", "terminal", "rendered"}, "blocking")
    side.close()


def step_budget(Side):
    scs, mc, side = _batch_side(Side, auto_reset=True, step_budget=40)
    buf = _registered(side)
    side.reset()
    _drive(side, buf, {"-2", "status 4", "rendered"}, "budget 40")
    side.close()


def time_sliced_launches(Side):
    scs, M, kw = _time_sliced_batch(Side.name)
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC
    side = Side(scs, DEFAULT_MC_SPEC, M, map_size=NO_IMAGE_G[Side.name], render=False, auto_reset=True, **kw)
    buf = _registered(side)
    side.reset()
    _drive(side, buf, {"-2", "status 4", "rendered"}, "time slices")
    side.close()


def load_clone_and_pool_reset(Side):
    scs, mc, side = _batch_side(Side)
    buf = _registered(side)
    side.reset()
    rng = np.random.RandomState(4)
    for _ in range(3):
        a = _agents(side)
        side.step(np.where(a >= 0, a, -2), rng.rand(5, 3))   # a finished row is left alone
    assert (_agents(side)[[0, 3]] >= 0).all()
    rec = side.save_envs([0, 3])
    # load: records of environments 0 and 3 into 1 and 4
    buf.fill()
    side.load_envs(rec, [1, 4])
    snap = _check_call(side, buf, {1, 4}, "load")
    pk = peeks(side.handle); agents = _agents(side)
    for dst, src in ((1, 0), (4, 3)):
        check_rows(buf.rows(snap, dst), reference(pk, dst, int(agents[dst]), scs[src], mc, side.N, 2), scs[src].n_node, "loaded row %d" % dst)
    # clone: 0 -> 2
    buf.fill()
    side.clone_envs([0], [2], **CLONE_KW[Side.name])
    _check_call(side, buf, {2}, "clone")
    # pool reset: rows 1 and 3 by mask, records chosen by the caller
    side.set_pool(rec, 5)
    buf.fill()
    side.pool_reset([0, 1, 0, 1, 0], [9, 1, 9, 0, 9])
    _check_call(side, buf, {1, 3}, "pool reset")
    side.close()


def ragged_batch_values_and_zero_rows(Side):
    """six_* (6 nodes) and hanoi1000n50 (82 nodes) in one handle: rows beyond each n_node are written as zeros."""
    _, six, _ = load_fixture("six_m3_zero_length")
    _, hanoi, mc = load_fixture("hanoi1000n50_m3_s1")
    scs = [six, hanoi]
    side = Side(scs, mc, 3, map_size=NO_IMAGE_G[Side.name], render=False)
    assert side.N == 82 and six.n_node == 6
    buf = _registered(side)
    side.reset()
    rng = np.random.RandomState(2)
    checked = 0
    for c in range(4):
        snap = buf.snap(); pk = peeks(side.handle); agents = _agents(side)
        for e in range(2):
            if agents[e] < 0:
                continue
            rows = buf.rows(snap, e)
            check_rows(rows, reference(pk, e, int(agents[e]), scs[e], mc, side.N, 3), scs[e].n_node, "ragged call %d row %d" % (c, e))
            assert not rows[0][scs[e].n_node:].any()
            checked += 1
        side.step(np.where(agents >= 0, agents, -2), rng.rand(2, 3))
    assert checked >= 6
    side.close()


def unregistering_and_identical_requests(Side):
    """No image with entities registered writes the rows; after wrsn_set_entity_out(h, NULL) the same calls write nothing into the
    buffers that were registered; the requests do not depend on entities being registered."""
    scs, mc, side = _batch_side(Side, auto_reset=True)
    _, _, plain = _batch_side(Side, auto_reset=True)
    buf = _registered(side)
    rng = np.random.RandomState(8)
    for c in range(10):
        act = rng.rand(5, 3)
        for v in (side, plain):
            if c == 0:
                v.reset()
            else:
                v.step(_agents(v), act)
        assert side.rows() == plain.rows(), c
    snap = buf.snap()
    assert any(buf.full(snap, e) for e in range(5))
    side.set_entity_out(None)                                 # off
    buf.fill()
    side.reset()
    side.step(_agents(side), rng.rand(5, 3))
    side.clone_envs([0], [1])
    check_extent(buf, buf.snap(), set(), "unregistered")
    assert (_agents(side) >= 0).any()
    side.close(); plain.close()


# ---- the bodies above on the emulator (tests/test_entities_gpu.py: on the device)
@pytest.mark.parametrize("name", FIXTURES)
def test_values_on_fixtures(name):
    values_on_fixtures(EmuSide, name)


def test_blocking_steps_and_a_masked_reset_write_the_rendered_rows_only(hip_lib):
    blocking_steps_and_a_masked_reset(EmuSide)


def test_step_budget_leaves_rows_in_flight_untouched(hip_lib):
    step_budget(EmuSide)


def test_time_sliced_launches_write_the_rendered_rows_only(hip_lib):
    time_sliced_launches(EmuSide)


def test_load_clone_and_pool_reset_write_the_replaced_rows_only(hip_lib):
    load_clone_and_pool_reset(EmuSide)


def test_ragged_batch_values_and_zero_rows():
    ragged_batch_values_and_zero_rows(EmuSide)


def test_entity_only_calls_unregistering_and_identical_requests(hip_lib):
    unregistering_and_identical_requests(EmuSide)


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
    scs, mc, ev = _batch_side(EmuSide)
    buf = _registered(ev)
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
    ev.reset()                                                # the handle still holds the buffers registered first
    check_extent(buf, buf.snap(), set(range(5)), "after refusals")
