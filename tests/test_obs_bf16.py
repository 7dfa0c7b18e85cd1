"""bf16 observations (wrsn_set_obs_format) on the CPU: the unmodified HIP sources in the lockstep wavefront emulator of tests/emu.

A bf16 observation is DEFINED by the float32 one: every cell is the float32 cell rounded to nearest even, bit for bit.  The tests
hold the render kernel, the roll-out copy kernels, the environment records and the trainer's state inputs to that, and the result to
the reference within the bound that follows from it:

    |bf16 - ref| <= 2^-8 |ref| + (1 + 2^-8) 1e-5 max(1, peak(ref))

(round-to-nearest-even to 8 significand bits has relative error <= 2^-8; the float32 observation is held to 1e-5 max(1, peak) by the
existing tests, and rounding a value that is off by d moves the result by at most (1 + 2^-8) d)."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from sides import EmuSide

CANARY = 0xA5C3
N_CANARY = 4096
FIXTURES = ["hanoi1000n50_m3_s1", "redundant_m2_map64", "six_m3_bs_charge_ongrid"]


def rne(x32):
    """bf16 bit patterns of a float32 array, round to nearest even, in integer arithmetic (finite values)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f64(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def test_rne_helper_equals_torch():
    import torch
    g = torch.Generator().manual_seed(1)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (1 << 18,), generator=g, dtype=torch.int64).to(torch.int32)
    x = bits.view(torch.float32)
    x = x[torch.isfinite(x)]
    ties = (torch.arange(0, 1 << 16, dtype=torch.int64) << 16 | 0x8000).to(torch.int32).view(torch.float32)
    x = torch.cat([x, ties[torch.isfinite(ties)], torch.tensor([0.0, -0.0, 1e-40, -1e-40, 5.7, 3.0e38])])
    x = x[x.abs() < 3.3e38]                                   # beyond: rounds to infinity either way, not an observation value
    assert np.array_equal(rne(x.numpy()), x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


class Bf16Emu:
    """An EmuSide whose observation buffer is exactly B*4*G*G uint16 followed by a canary region."""

    def __init__(self, scenarios, mc, M, **kw):
        from multi_agent_rl_wrsn_amd import _lib
        self.ev = ev = EmuSide(scenarios, mc, M, **kw)
        ev.h.set_obs_format(_lib.OBS_BF16)
        n = ev.B * 4 * ev.G * ev.G
        self.raw = np.full(n + N_CANARY, CANARY, dtype=np.uint16)
        self.raw[:n] = 0
        ev.obs = self.raw[:n].reshape(ev.B, 4, ev.G, ev.G)     # EmuSide._ptrs hands out self.obs.ctypes.data

    def canary_ok(self):
        return bool((self.raw[self.ev.obs.size:] == CANARY).all())


def _pair(scenarios, mc, M, **kw):
    return EmuSide(scenarios, mc, M, **kw), Bf16Emu(scenarios, mc, M, **kw)


def _ref_ok(bits, ref):
    got = bf16_to_f64(bits).reshape(np.shape(ref)); ref = np.asarray(ref, dtype=np.float64)
    peak = max(1.0, float(np.nanmax(np.abs(ref))))
    return bool(np.all(np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + (1 + 2.0 ** -8) * 1e-5 * peak))


@functools.lru_cache(maxsize=None)
def _replay(name):
    """The fixture's scripted actions on two emulated handles, one per format, reuse on: [(k, float32 row, bf16 row)], k = -1 the reset."""
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    z = load_golden(name)
    sc, mc = scenario_from_golden(z)
    a, b = _pair([sc], mc, int(z["num_agent"]), map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    a.reset(); b.ev.reset()
    out = [(-1, a.obs[0].copy(), b.ev.obs[0].copy())]
    for k in range(len(z["in_action"])):
        for ev in (a, b.ev):
            ev.step([int(z["in_agent"][k])], z["in_action"][k][None])
        assert int(a.agent_id[0]) == int(b.ev.agent_id[0]) and a.now[0] == b.ev.now[0] and a.reward[0] == b.ev.reward[0]
        assert b.canary_ok()
        if z["is_none"][k] or z["terminal"][k]:
            break
        if a.agent_id[0] >= 0:
            out.append((k, a.obs[0].copy(), b.ev.obs[0].copy()))
    return z, out


@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_observation_is_the_rounded_float32_one_on_fixtures(name):
    """1. bit-exactness against the float32 path, every cell, after reset and after every decision."""
    z, rows = _replay(name)
    assert len(rows) >= 3
    for k, f32, b16 in rows:
        assert f32.shape == b16.shape == (4, int(z["map_size"]), int(z["map_size"]))
        assert np.array_equal(b16, rne(f32)), (name, k, int((b16 != rne(f32)).sum()))


@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_observation_matches_the_reference_on_fixtures(name):
    """2. against the reference's reset_obs, obs_full[k] and the strided obs_sample[k] (as tests/parity.py reads them)."""
    z, rows = _replay(name)
    s = int(z["obs_stride"])
    n_full = 0
    for k, _, b16 in rows:
        if k < 0:
            assert _ref_ok(b16, z["reset_obs"]), (name, "reset")
            continue
        if np.isinf(z["reward"][k]):
            continue
        assert _ref_ok(b16[:, ::s, ::s], z["obs_sample"][k]), (name, k, "sample")
        if k < z["obs_full"].shape[0]:
            assert _ref_ok(b16, z["obs_full"][k]), (name, k, "full"); n_full += 1
    assert n_full >= 1


def test_reference_values_satisfy_the_bound_themselves():
    """The bound of test 2 is derived, not tuned: rounding the fixtures' own values satisfies it."""
    for name in FIXTURES:
        z = load_golden(name)
        for ref in [z["reset_obs"]] + list(z["obs_full"]):
            assert _ref_ok(rne(ref.astype(np.float32)), ref)


def test_bf16_ragged_batch_of_different_networks(hip_lib):
    """1 + 2 on a batch of three networks of different sizes (ragged N / T) with node deaths, against the float32 handle and the oracle."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    from wrsn_oracle import OracleWRSN
    scs = [synth_scenario(7, 90, 60), synth_scenario(8, 130, 100), synth_scenario(9, 64, 64)]
    M = 3
    a, b = _pair(scs, DEFAULT_MC_SPEC, M)
    ors = [OracleWRSN(s.node_xy, s.target_xy, s.bs_xy, s.node_spec, DEFAULT_MC_SPEC, s.max_time, M) for s in scs]
    a.reset(); b.ev.reset()
    last = [o.reset() for o in ors]
    assert np.array_equal(b.ev.obs, rne(a.obs))
    for e in range(3):
        assert _ref_ok(b.ev.obs[e], last[e]["state"])
    rng = np.random.RandomState(5)
    done = [False] * 3
    checked = 0
    for step in range(14):
        act = rng.rand(3, 3)
        ids = [(-2 if done[e] else (-1 if last[e]["agent_id"] is None else last[e]["agent_id"])) for e in range(3)]
        keep = b.ev.obs.copy()
        a.step(ids, act); b.ev.step(ids, act)
        assert b.canary_ok()
        assert np.array_equal(a.agent_id, b.ev.agent_id) and np.array_equal(a.now, b.ev.now)
        for e, o in enumerate(ors):
            if done[e]:
                assert np.array_equal(b.ev.obs[e], keep[e])      # -2 row: untouched
                continue
            last[e] = o.step(last[e]["agent_id"], act[e])
            if last[e]["terminal"]:
                done[e] = True
                assert np.array_equal(b.ev.obs[e], keep[e])      # terminal return: no request, row untouched
                continue
            assert np.array_equal(b.ev.obs[e], rne(a.obs[e])), (step, e)
            assert _ref_ok(b.ev.obs[e], last[e]["state"]), (step, e)
            checked += 1
        if all(done):
            break
    assert checked >= 10


@pytest.mark.parametrize("G", [12, 64, 96, 100, 128])
def test_bf16_observation_at_other_map_sizes(G):
    """1 + 2 at the map sizes the float32 tests render: rows that are only 8-byte aligned (12, 100), G % 8 == 0 (64, 96, 128); fewer rows
    than one matrix-core band, no VALU rows, a full fourth band on the store wave."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    from wrsn_oracle import OracleWRSN
    sc = synth_scenario(33, 90, 70)
    M = 3
    a, b = _pair([sc], DEFAULT_MC_SPEC, M, map_size=G)
    o = OracleWRSN(sc.node_xy, sc.target_xy, sc.bs_xy, sc.node_spec, DEFAULT_MC_SPEC, sc.max_time, M, map_size=G)
    a.reset(); b.ev.reset(); r = o.reset()
    assert np.array_equal(b.ev.obs, rne(a.obs)) and _ref_ok(b.ev.obs[0], r["state"]) and b.canary_ok()
    rng = np.random.RandomState(4)
    n = 0
    for k in range(5):
        act = rng.rand(3)
        ids = [int(a.agent_id[0])]
        a.step(ids, act[None]); b.ev.step(ids, act[None]); r = o.step(r["agent_id"], act)
        assert b.canary_ok()
        if r["terminal"] or r["agent_id"] is None:
            break
        assert int(b.ev.agent_id[0]) == r["agent_id"]
        assert np.array_equal(b.ev.obs, rne(a.obs)), k
        assert _ref_ok(b.ev.obs[0], r["state"]), k
        n += 1
    assert n >= 3


def test_bf16_extent_and_untouched_rows(hip_lib):
    """3. the buffer is exactly B*4*G*G uint16 with a canary region behind it: after resets, steps with -2 and terminal rows and a masked
    reset, the canary and the rows the float32 path leaves untouched are byte-identical."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    sc = synth_scenario(21, 70, 50)
    b = Bf16Emu([sc, sc, sc], DEFAULT_MC_SPEC, 2, map_size=20)
    ev = b.ev
    ev.reset()
    assert b.canary_ok() and ev.obs.any(axis=(1, 2, 3)).all()
    rng = np.random.RandomState(3)
    ids = np.array([0, -2, 0], dtype=np.int32)
    seen_terminal = False
    for _ in range(60):
        keep = ev.obs.copy()
        ev.step(ids, rng.rand(3, 3))                           # no auto-reset: environment 0 runs into its terminal return
        assert b.canary_ok()
        assert np.array_equal(ev.obs[1], keep[1])              # -2 row
        for e in (0, 2):
            if ids[e] == -2 or ev.agent_id[e] < 0:
                assert np.array_equal(ev.obs[e], keep[e])      # terminal return / row left out: untouched
        if ev.terminal[0]:
            seen_terminal = True
            break
        ids[0] = ev.agent_id[0]; ids[2] = ev.agent_id[2] if not ev.terminal[2] else -2
    assert seen_terminal
    keep = ev.obs.copy()
    mask = np.array([1, 0, 0], dtype=np.uint8)
    ev.h.reset(mask.ctypes.data, **ev._ptrs(True))
    assert b.canary_ok()
    assert np.array_equal(ev.obs[1], keep[1]) and np.array_equal(ev.obs[2], keep[2])
    assert ev.agent_id[0] == 0 and not np.array_equal(ev.obs[0], keep[0])
    # the last row ends exactly where the buffer ends
    ev.step(np.array([-2, -2, int(ev.agent_id[2]) if ev.agent_id[2] >= 0 else -2], dtype=np.int32), rng.rand(3, 3))
    assert b.canary_ok()


def test_bf16_reuse_is_bit_identical():
    """4a. bf16 with map-1 reuse equals bf16 without, bit for bit, over an episode with same-instant returns."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(50 + e, 70, 60) for e in range(3)]
    M, G = 3, 20
    a = Bf16Emu(scs, DEFAULT_MC_SPEC, M, map_size=G); b = Bf16Emu(scs, DEFAULT_MC_SPEC, M, map_size=G)
    b.ev.h.set_obs_reuse(False)
    a.ev.reset(); b.ev.reset()
    assert np.array_equal(a.ev.obs, b.ev.obs)
    rng = np.random.RandomState(8)
    other = np.zeros_like(a.ev.obs)
    zero_time = 0
    for k in range(14):
        act = rng.rand(3, 3)
        ids = a.ev.agent_id.copy(); now0 = a.ev.now.copy()
        b.ev.obs[:] = 0x4242                                   # the caller of b scribbles over its buffer: b renders in full every time
        a.ev.step(ids, act, auto_reset=True); b.ev.step(ids, act, auto_reset=True)
        zero_time += int(((a.ev.now == now0) & (a.ev.status == 0) & (a.ev.agent_id >= 0)).sum())
        rows = a.ev.agent_id >= 0
        assert np.array_equal(a.ev.obs[rows], b.ev.obs[rows]), k
        if k % 3 == 1:
            agents = np.maximum(a.ev.agent_id, 0).astype(np.int32)
            a.ev.h.render(agents.ctypes.data, other.ctypes.data)
            assert np.array_equal(other[rows][:, 0], a.ev.obs[rows][:, 0])
    assert zero_time >= 3 and a.canary_ok() and b.canary_ok()


def test_reuse_does_not_survive_a_change_of_format_at_the_same_address():
    """4b. render float32 into a buffer, switch the handle to bf16, render into the SAME address: map 1 equals a render into a fresh
    buffer; the same in the other direction.  (Row 0 has the same address in both formats.)"""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, _lib, synth_scenario
    G = 20
    ev = EmuSide([synth_scenario(50, 70, 60)], DEFAULT_MC_SPEC, 3, map_size=G)    # reuse on
    ev.reset()
    agents = ev.agent_id.copy()
    buf = np.zeros(4 * G * G, dtype=np.float32)                # one address for both formats
    as16 = buf.view(np.uint16)[:4 * G * G].reshape(4, G, G)
    ev.h.render(agents.ctypes.data, buf.ctypes.data)           # float32 at `buf`: the reuse key now names this address
    f32 = buf.reshape(4, G, G).copy()
    assert np.array_equal(f32, ev.obs[0])
    ev.h.set_obs_format(_lib.OBS_BF16)
    ev.h.render(agents.ctypes.data, buf.ctypes.data)           # bf16 at the same address: map 1 has to be rendered
    got = as16.copy()
    fresh = np.zeros((4, G, G), dtype=np.uint16)
    ev.h.render(agents.ctypes.data, fresh.ctypes.data)
    assert np.array_equal(got[0], fresh[0]) and np.array_equal(got, fresh) and np.array_equal(got, rne(f32))
    # the other direction: bf16 at `buf` (remembered), then float32 at `buf`
    ev.h.render(agents.ctypes.data, buf.ctypes.data)
    assert np.array_equal(as16, fresh)
    ev.h.set_obs_format(_lib.OBS_F32)
    ev.h.render(agents.ctypes.data, buf.ctypes.data)
    assert np.array_equal(buf.reshape(4, G, G), f32)
    # and reuse still works within one format: scribble over map 1, render again at the same address -> map 1 is left alone
    buf[:G * G] = -3.0
    ev.h.render(agents.ctypes.data, buf.ctypes.data)
    assert (buf[:G * G] == -3.0).all() and np.array_equal(buf.reshape(4, G, G)[1:], f32[1:])


def _policy(e, n):
    r = np.random.RandomState(7919 * e + n)
    return r.rand(3).astype(np.float32), np.float32(-r.rand())


def _tr_arrays(B, M, S, CAP, obs_dtype):
    def guarded(shape, dtype):
        n = int(np.prod(shape))
        raw = np.full(n + N_CANARY, CANARY, dtype=np.uint16) if dtype == np.uint16 else np.zeros(n + N_CANARY, dtype=dtype)
        raw[:n] = 0
        return raw, raw[:n].reshape(shape)
    raws, arrs = {}, {}
    for k, shape, dt in (("pend_state", (B, M, S), obs_dtype), ("pend_action", (B, M, 3), np.float32), ("pend_logp", (B, M), np.float32),
                         ("pend_valid", (B, M), np.uint8), ("state", (M, CAP, S), obs_dtype), ("action", (M, CAP, 3), np.float32),
                         ("next_state", (M, CAP, S), obs_dtype), ("reward", (M, CAP), np.float32), ("logp", (M, CAP), np.float32),
                         ("now", (M, CAP), np.float64), ("env", (M, CAP), np.int32), ("count", (M,), np.int32)):
        raws[k], arrs[k] = guarded(shape, dt)
    return raws, arrs


def test_bf16_rollout_buffers_hold_the_observation_rows():
    """5. wrsn_rollout_record / wrsn_rollout_collect with bf16 buffers (a canary behind each): every stored state / next_state row is the
    bf16 observation row it was taken from; counts, rewards, now, env equal those of the same run in float32."""
    _rollout_buffers_hold_the_observation_rows(12)


def test_bf16_rollout_buffers_hold_rows_that_are_not_16_byte_aligned():
    """5 at an odd map size: a bf16 row is 8 G^2 bytes, so every second row of the buffers starts 8 bytes past a 16-byte boundary and
    the copy of wrsn_tr_copy goes element by element instead of in 16-byte accesses (no other roll-out test has such rows)."""
    G = 7
    assert (4 * G * G * 2) % 16 == 8
    _rollout_buffers_hold_the_observation_rows(G)


def _rollout_buffers_hold_the_observation_rows(G):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, _lib, synth_scenario
    B, M, CAP, K = 3, 2, 64, 20
    S = 4 * G * G
    scs = [synth_scenario(300 + e, 70, 60) for e in range(B)]
    runs = {}
    for fmt in ("f32", "bf16"):
        if fmt == "bf16":
            w = Bf16Emu(scs, DEFAULT_MC_SPEC, M, map_size=G); ev = w.ev
        else:
            w = None; ev = EmuSide(scs, DEFAULT_MC_SPEC, M, map_size=G)
        ev.h.set_step_budget(60)
        raws, arrs = _tr_arrays(B, M, S, CAP, np.uint16 if fmt == "bf16" else np.float32)
        buf = _lib.WrsnTransitionBuffers(CAP, 3, *[arrs[k].ctypes.data for k in ("pend_state", "pend_action", "pend_logp", "pend_valid", "state",
                                                                                "action", "next_state", "reward", "logp", "now", "env", "count")])
        ev.reset()
        n_dec = np.zeros(B, dtype=int)
        seen = []                                             # every observation row the library has handed out, as bytes
        for it in range(400):
            ids = ev.agent_id.copy()
            act = np.zeros((B, 3), np.float32); lp = np.zeros(B, np.float32)
            for e in range(B):
                if ids[e] >= 0 and n_dec[e] < K:
                    act[e], lp[e] = _policy(e, n_dec[e]); n_dec[e] += 1
                    seen.append(ev.obs[e].tobytes())
                elif ids[e] >= 0:
                    ids[e] = -2
            ev.h.rollout_record(buf, ids.ctypes.data, act.ctypes.data, lp.ctypes.data, ev.obs.ctypes.data)
            ev.step(ids, act.astype(np.float64), auto_reset=True)
            ev.h.rollout_collect(buf, **ev._ptrs(True))
            for e in range(B):
                if ev.agent_id[e] >= 0 and ev.status[e] != 4:
                    seen.append(ev.obs[e].tobytes())
            if (n_dec >= K).all() and not (ev.status == 4).any():
                break
        if w is not None:
            assert w.canary_ok()
            for k in ("pend_state", "state", "next_state"):
                assert (raws[k][arrs[k].size:] == CANARY).all(), k
        runs[fmt] = (arrs, set(seen))
    a32, _ = runs["f32"]; a16, seen16 = runs["bf16"]
    assert a16["state"].dtype == np.uint16 and a16["state"].nbytes * 2 == a32["state"].nbytes
    assert np.array_equal(a32["count"], a16["count"]) and (a16["count"] > 0).all()
    for k in ("reward", "now", "env", "logp", "action", "pend_valid", "pend_action", "pend_logp"):
        assert np.array_equal(a32[k], a16[k]), k
    for a in range(M):
        n = min(int(a16["count"][a]), CAP)
        for q in range(n):
            assert a16["state"][a, q].tobytes() in seen16 and a16["next_state"][a, q].tobytes() in seen16, (a, q)
        assert np.array_equal(a16["state"][a, :n], rne(a32["state"][a, :n])) and np.array_equal(a16["next_state"][a, :n], rne(a32["next_state"][a, :n]))
        assert not a16["state"][a, n:].any() and not a16["next_state"][a, n:].any()
    assert np.array_equal(a16["pend_state"], rne(a32["pend_state"]))


def test_bf16_records_render_the_destination_row(hip_lib):
    """6. clone_envs / save_envs + load_envs with out.obs on a bf16 handle: the destination's rendered row equals the source's."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    scs = [synth_scenario(60, 80, 70), synth_scenario(61, 80, 70), synth_scenario(62, 80, 70)]
    b = Bf16Emu(scs, DEFAULT_MC_SPEC, 2, map_size=20)
    ev = b.ev
    ev.reset()
    rng = np.random.RandomState(2)
    for _ in range(3):
        ids = ev.agent_id.copy(); ids[1:] = -2
        ev.step(ids, rng.rand(3, 3))
    assert ev.agent_id[0] >= 0 and not np.array_equal(ev.obs[0], ev.obs[1])
    ev.h.clone_envs([0], [1], **ev._ptrs(True))
    assert ev.agent_id[1] == ev.agent_id[0] and ev.now[1] == ev.now[0]
    assert np.array_equal(ev.obs[1], ev.obs[0]) and b.canary_ok()
    rec = np.zeros((1, ev.h.env_record_bytes()), dtype=np.uint8)
    p = ev._ptrs(False); p.pop("obs")
    ev.h.save_envs(np.array([0], dtype=np.int32), rec.ctypes.data, **p)
    assert not np.array_equal(ev.obs[2], ev.obs[0])
    ev.h.load_envs(np.array([2], dtype=np.int32), rec.ctypes.data, **ev._ptrs(True))
    assert ev.agent_id[2] == ev.agent_id[0] and np.array_equal(ev.obs[2], ev.obs[0]) and b.canary_ok()
    # the copies go on like the source: one more step of all three with the same action
    act = np.tile(rng.rand(1, 3), (3, 1))
    ev.step(ev.agent_id.copy(), act)
    assert ev.agent_id[1] == ev.agent_id[0] == ev.agent_id[2]
    if ev.agent_id[0] >= 0:
        assert np.array_equal(ev.obs[1], ev.obs[0]) and np.array_equal(ev.obs[2], ev.obs[0])


def test_obs_format_abi_default_and_bad_values():
    """7. the default is float32 (a fresh handle renders what a handle explicitly set to float32 renders, and what the fixture holds);
    formats 2 and -1 are WRSN_ERR_ARG and the handle goes on rendering in its previous format."""
    from multi_agent_rl_wrsn_amd import _lib
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    assert (_lib.OBS_F32, _lib.OBS_BF16) == (0, 1) and "wrsn_set_obs_format" in _lib.EXPORTS
    z = load_golden("six_m3_bs_charge_ongrid")
    sc, mc = scenario_from_golden(z)
    kw = dict(map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    fresh = EmuSide([sc], mc, int(z["num_agent"]), **kw)
    fresh.reset()
    assert fresh.obs.dtype == np.float32
    assert np.max(np.abs(fresh.obs[0] - z["reset_obs"])) <= 1e-5 * max(1.0, np.abs(z["reset_obs"]).max())
    ev = EmuSide([sc], mc, int(z["num_agent"]), **kw)
    ev.h.set_obs_reuse(False)
    ev.h.set_obs_format(_lib.OBS_F32)
    for bad in (2, -1):
        with pytest.raises(_lib.WrsnError) as ei:
            ev.h.set_obs_format(bad)
        assert ei.value.code == -1
    ev.reset()
    assert np.array_equal(ev.obs, fresh.obs)                  # still float32, byte for byte
    ev.h.set_obs_format(_lib.OBS_BF16)
    for bad in (2, -1, 256):
        with pytest.raises(_lib.WrsnError) as ei:
            ev.h.set_obs_format(bad)
        assert ei.value.code == -1
    raw = np.full(fresh.obs.size + N_CANARY, CANARY, dtype=np.uint16)
    ev.h.render(ev.agent_id.ctypes.data, raw.ctypes.data)     # still bf16
    assert np.array_equal(raw[:fresh.obs.size], rne(fresh.obs).reshape(-1)) and (raw[fresh.obs.size:] == CANARY).all()


def test_vec_env_rejects_unknown_obs_dtype_before_anything_is_created():
    import torch
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    from multi_agent_rl_wrsn_amd.vec_env import obs_torch_dtype
    assert obs_torch_dtype("float32") is torch.float32 and obs_torch_dtype(torch.float32) is torch.float32
    assert obs_torch_dtype("bfloat16") is torch.bfloat16 and obs_torch_dtype(torch.bfloat16) is torch.bfloat16
    for bad in ("float16", torch.float16, "bf16", None, 2):
        with pytest.raises(ValueError):
            VecWRSN([synth_scenario(1, 20, 10)], None, 1, obs_dtype=bad)


def test_trainer_takes_bf16_states_on_the_host():
    """8. PPOLearner on the CPU: evaluate, get_value / _values and one update on bf16 state tensors give bit-identical results to the
    same calls on states.float() -- a chunk / minibatch is widened exactly, nothing else changes."""
    import torch
    from multi_agent_rl_wrsn_amd import PPOLearner
    torch.set_num_threads(2)
    G, n = 12, 8
    args = dict(batch_size=n, minibatch_size=4, n_updates_per_iteration=2, lr=1e-3)
    g = torch.Generator().manual_seed(5)
    states16 = (torch.rand((n, 4, G, G), generator=g) * 3).to(torch.bfloat16)
    batch = dict(actions=torch.randn((n, G, G), generator=g), log_probs=torch.randn(n, generator=g) - 150.0, advantages=torch.randn(n, generator=g),
                 returns=torch.randn(n, generator=g), values=torch.randn(n, generator=g))
    res = []
    for states in (states16, states16.float()):
        torch.manual_seed(11)
        lr = PPOLearner(args, 1, G, "cpu", infer_chunk=3)        # chunks of 3, 3, 2 rows
        with torch.no_grad():
            lp, ent = lr.evaluate(0, states, batch["actions"])
            val = lr.get_value(0, states)
        vals = lr._values(0, states)
        rlp = lr.rollout_logp(0, states, batch["actions"])
        torch.manual_seed(3)
        act, alp = lr.get_action(0, states)
        ret, adv, v = lr.cal_rt_adv(0, states, batch["returns"], states, torch.zeros(n))
        stats = lr.update(0, dict(batch, states=states), shuffle=np.random.RandomState(3).shuffle)
        params = torch.cat([p.detach().reshape(-1) for p in list(lr.actors[0].parameters()) + list(lr.critics[0].parameters())])
        res.append((lp, ent, val, vals, rlp, act, alp, ret, adv, v, torch.tensor(stats), params))
    for x, y in zip(*res):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert states16.dtype == torch.bfloat16                   # the caller's tensor is not converted in place
