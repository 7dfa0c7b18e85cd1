"""The launch order of a step call (wrsn_estimate_kernel / wrsn_sort_kernel behind WRSN_PEEK_ORDER) against numpy: one body, run here
on the emulator and by tests/test_launch_order_gpu.py on the device.

The order decides which environments a budgeted or time-sliced launch takes, and nothing else compares it with anything.  The sort
workgroup has 256 threads on the emulator and 1024 on the device, so the keys per thread K that a batch size selects differ: the
emulator's shapes cover K = 1, 1, 2, 4, the device's K = 1, 1, 2, 4, 8 (every instantiation the dispatch of launch_order has).

  (a) the order is numpy's stable sort of key >> 18 (the sort's 2 048 buckets of 8 simulated seconds; padding keys behind the batch), ties
      by environment index -- on the device that rests on the lanes of one LDS atomic being served in lane order --, a permutation of
      0 .. B-1, and the same over three calls on the same loaded state;
  (b) with one charger (the asking charger is the only alive one) the work figure of every key is the estimate's formula in float64
      from what the peeks show before the call: frame, charging_time_max and clock (WRSN_PEEK_ENV), charger position and safe horizon
      (WRSN_PEEK_MC), the velocity of the charger type and the clipped action.  Exact: float64 on both sides, quantised to quarter seconds
      (a product is never fused with a sum where the estimate is computed: dist2 forbids it, and the frame translation is compared
      through the quantisation only).

Seven rows in ten are sent 10.6 m from where their charger stands with no charging time: 10.12 s of work, so they fall into two
buckets at most (with and without the surcharge of a node that may run dry) and ties span waves and keys of one thread; the share is
checked on the keys.  The other rows get random actions past both clip edges, and every eleventh row is nobody's (-2: no work)."""
import numpy as np
import pytest

from sides import EmuSide

N_NODE, N_UNIQ, SEED = 20, 24, 47000
EMU_B = (1, 63, 257, 520)                                    # K = 1, 1, 2, 4 of 256 sort threads
GPU_B = (1, 1000, 1025, 2049, 8192)                          # K = 1, 1, 2, 4, 8 of 1 024 sort threads
NEAR_M = 10.6                                                # tie rows: metres between the charger and where it is sent (2.12 s: 10.12 s of
                                                             # work, 40.48 quarter seconds -- not ON a quantisation step, where the last bit of
                                                             # the frame translation, fused on the device, would decide)
MAX_CHARGE = 0.01                                            # other rows: largest charging-time action (216 s of 21 600)


def expected_work(env, mc, ids, act, velocity):
    """The 16-bit work figure of wrsn_estimate_kernel per row, for one charger: quarter seconds until the charger that is handed `act`
    is done, + 250 s when a node may run dry before that, + 8 s for a step that does anything; 0 for a row that is nobody's.  -1 where
    the peeks do not decide it (no request pending: the charger's old action runs on)."""
    now, ctm = env["now"], env["charging_time_max"]
    a = np.clip(act, 0.0, 1.0)
    px = a[:, 0] * (env["xmax"] - env["xmin"]) + env["xmin"]
    py = a[:, 1] * (env["ymax"] - env["ymin"]) + env["ymin"]
    dx, dy = px - mc["loc_x"][:, 0], py - mc["loc_y"][:, 0]
    t = now + np.sqrt(dx * dx + dy * dy) / velocity + ctm * a[:, 2]
    w = np.clip(t - now, 0.0, 1.0e4)
    safe = mc["safe"][:, 0]
    w = np.where(safe < 0, 0.0, np.where(safe < w, w + 250.0, w)) + 8.0
    q = np.minimum((w * 4.0).astype(np.int64), 0xFFFF)
    q = np.where(ids == -2, 0, q)
    return np.where((ids == 0) & (mc["status"][:, 0] != 0) | (ids == -2), q, -1)


def launch_order_is_pinned(Side, B):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    uniq = [synth_scenario(SEED + u, N_NODE, N_NODE) for u in range(N_UNIQ)]
    scs = [uniq[e % N_UNIQ] for e in range(B)]
    side = Side(scs, DEFAULT_MC_SPEC, 1, map_size=8, render=False)
    rng = np.random.RandomState(SEED + B)
    side.reset()
    ids = side._host()["agent_id"].astype(np.int64)
    assert (ids == 0).all()
    # one call that spreads the states: clocks, charger positions and safe horizons differ from row to row afterwards
    act = rng.rand(B, 3); act[:, 2] *= MAX_CHARGE
    side.step(ids, act)
    ids = side._host()["agent_id"].astype(np.int64)
    env, mc = side.env_info(), side.mcs()
    tie = (np.arange(B) % 10) < 7
    ang = rng.rand(B) * 2.0 * np.pi
    act = rng.rand(B, 3) * [1.4, 1.4, MAX_CHARGE] - [0.2, 0.2, 0.0]
    act[tie, 0] = ((mc["loc_x"][:, 0] + NEAR_M * np.cos(ang) - env["xmin"]) / (env["xmax"] - env["xmin"]))[tie]
    act[tie, 1] = ((mc["loc_y"][:, 0] + NEAR_M * np.sin(ang) - env["ymin"]) / (env["ymax"] - env["ymin"]))[tie]
    act[tie, 2] = 0.0
    ids[np.arange(B) % 11 == 7] = -2
    assert B < 11 or ((act[:, :2] < 0).any() and (act[:, :2] > 1).any()), "both clip edges of the estimate"
    want_q = expected_work(env, mc, ids, act, DEFAULT_MC_SPEC["velocity"])
    rec = side.save_envs()
    seen = []
    for call in range(3):
        if call:
            side.load_envs(rec)
        side.step(ids, act)
        keys, order = side.handle.launch_order()
        seen.append((keys.copy(), order.copy()))
        # (a)
        assert np.array_equal(keys & 0x1FFF, np.arange(B)), call
        assert np.array_equal(np.sort(order), np.arange(B)), (call, "not a permutation")
        want = np.argsort(keys >> 18, kind="stable")
        if not np.array_equal(order, want):
            bad = np.nonzero(order != want)[0]
            raise AssertionError(("order", call, B, len(bad), [(int(p), int(order[p]), int(want[p]), int(keys[order[p]] >> 18), int(keys[want[p]] >> 18)) for p in bad[:8]]))
        # (b)
        got_q = 0xFFFF - (keys >> 13).astype(np.int64)
        known = want_q >= 0
        assert known.sum() >= (B * 9) // 10, (known.sum(), B)
        if not np.array_equal(got_q[known], want_q[known]):
            bad = np.nonzero(known & (got_q != want_q))[0]
            raise AssertionError(("work figure", call, B, len(bad), [(int(e), int(got_q[e]), int(want_q[e]), float(mc["safe"][e, 0])) for e in bad[:8]]))
    for k, o in seen[1:]:
        assert np.array_equal(k, seen[0][0]) and np.array_equal(o, seen[0][1]), "the order of a loaded state differs from call to call"
    bucket, count = np.unique(seen[0][0] >> 18, return_counts=True)
    shared = int(count[count > 1].sum())
    print("launch order on %s, B = %d: %d buckets, largest %d rows, %d rows share theirs; work figures %d .. %d, %d rows with the surcharge"
          % (Side.name, B, len(bucket), count.max(), shared, want_q[want_q >= 0].min(), want_q.max(), int((mc["safe"][:, 0] < 10).sum())))
    if B > 1:
        assert 2 * shared >= B and 2 * np.sort(count)[-2:].sum() >= B, (shared, np.sort(count)[-2:], B)   # ties are exercised: two buckets hold the near rows
        assert len(bucket) >= 3 or B < 11
    side.close()


@pytest.mark.parametrize("B", EMU_B)
def test_emulated_launch_order_is_pinned(B, hip_lib):
    launch_order_is_pinned(EmuSide, B)
