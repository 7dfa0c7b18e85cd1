"""The heuristic baseline on the entity rows (wrsn_entity_heuristic_act; csrc/wrsn_rollout.h) on the emulated library.

The bodies take the side (tests/sides.py): this module runs them on EmuSide, tests/test_entity_heuristic_gpu.py on VecSide.  The reference
is numpy float32 with the operations in the order of include/wrsn_hip.h (tests/episode_ref.py, `heuristic_ref`); every comparison is of
bytes, so there is no tolerance.  Sizes: N = 5 is a partial wave, 64 one full wave, 65 a wave and one more node, 257 more than four
waves' worth; M = 1 has nobody to claim a node, M = 8 is the widest charger block.  B = 6 rows are two blocks of four waves, the second
one partial."""
import numpy as np
import pytest
from sides import EmuSide

import entity_act_ref as R
import episode_ref as E

WRSN_ERR_ARG = -1
SIZES = [(N, M) for N in (5, 64, 65, 257) for M in (1, 3, 8)]
B0 = 6


def rows_for(N, M, B=B0, seed=0):
    """Synthetic entity rows with discs that claim a fair share of the nodes: (node, mc, env, ids); row 1 is skipped (id -1), row 4 has
    an id beyond M (skipped too)."""
    ids = np.arange(B, dtype=np.int32) % M
    ids[1] = -1
    if B > 4:
        ids[4] = M
    node, mc, env = R.synth_rows(40 + N + M, B, N, M, np.clip(ids, 0, M - 1))
    env[:, :2] = 0.25                                         # a charging disc of a quarter of the field: some nodes claimed, some not
    return node, mc, env, ids


def run_case(side, node, mc, env, ids, charge_scale=1.0, tag=""):
    call = E.HeuristicCall(side, node, mc, env, ids)
    got = call.run(charge_scale)
    want = call.expected(node, mc, env, ids, charge_scale)
    assert call.guards_intact(), tag
    assert E.same(got[0], want[0]), (tag, "action", got[0], want[0])
    assert E.same(got[1], want[1]), (tag, "action_f64")
    return got


# ------------------------------------------------------------------------------------------------------------ 1. sizes
def sizes_match(Side, N, M):
    """Every evaluated row equals the reference, skipped rows keep their pattern bytes, guards hold; the rows do differ from each other."""
    side = E.BareSide(Side, B0, N, M)
    node, mc, env, ids = rows_for(N, M)
    got, _ = run_case(side, node, mc, env, ids, tag=(N, M))
    assert (got[1].view(np.uint8) == E.T.PATTERN).all() and (got[4].view(np.uint8) == E.T.PATTERN).all()   # the skipped rows
    assert np.isfinite(got[[0, 2, 3, 5]]).all()
    if N > 5:
        assert len({tuple(r) for r in got[[0, 2, 3, 5]].tolist()}) > 1
    side.close()


@pytest.mark.parametrize("N,M", SIZES)
def test_emulated_heuristic_sizes(N, M):
    sizes_match(EmuSide, N, M)


# ------------------------------------------------------------------------------------------------------------ 2. planted cases
def planted(N, M):
    """Rows with one planted situation each; returns (node, mc, env, ids, what the test asserts about row e -> function of the action)."""
    B = 8
    ids = np.zeros(B, np.int32)
    node, mc, env, _ = rows_for(N, M, B, seed=1)
    ids[:] = 0
    mc[:, :, 3] = 0; mc[:, 0, 3] = 1
    f = np.float32
    checks = {}
    node[..., 7] = 1; node[..., 2] = np.linspace(0.1, 0.9, N, dtype=f)[None, :]; node[..., 3] = f(0.5)
    mc[:, :, 4] = 0                                           # nobody claims anything unless a case says so
    last = N - 1
    # 0: ties in w_n: the lowest index wins
    node[0, :, 2] = f(0.3); node[0, [2, last], 2] = f(0.7)
    checks[0] = lambda a: (a[0], a[1]) == (node[0, 2, 0], node[0, 2, 1])
    # 1: every alive node claimed (M > 1: a disc over the whole field): the fallback picks the largest of all alive nodes
    if M > 1:
        mc[1, 1, 4] = 1; mc[1, 1, 6:8] = f(0.5); env[1, :2] = f(10.0)
    checks[1] = lambda a: (a[0], a[1]) == (node[1, last, 0], node[1, last, 1])
    # 2: no alive node: the charger stays where it is and does not charge
    node[2, :, 7] = 0
    checks[2] = lambda a: tuple(a) == (mc[2, 0, 0], mc[2, 0, 1], f(0))
    # 3: a NaN w_n in an alive node never wins, inf does
    node[3, last, 2] = f(np.nan); node[3, 1, 2] = f(np.inf)
    checks[3] = lambda a: (a[0], a[1]) == (node[3, 1, 0], node[3, 1, 1])
    # 4: NaN and inf in dead rows have no effect
    node[4, 0, 7] = 0; node[4, 0, :7] = f(np.nan); node[4, 3 % N, 7] = 0; node[4, 3 % N, 2] = f(np.inf)
    checks[4] = lambda a: (a[0], a[1]) == (node[4, last, 0], node[4, last, 1]) and np.isfinite(a).all()
    # 5: no is_self row: self is the asking charger (here 0 again, but through agent_id); with M > 1 charger 1 asks and charger 0 claims
    mc[5, :, 3] = 0
    if M > 1:
        ids[5] = 1; mc[5, 0, 4] = 1; mc[5, 0, 6:8] = node[5, last, :2]; env[5, :2] = f(1e-3)   # a tiny disc on the best node
        checks[5] = lambda a: (a[0], a[1]) == (node[5, last - 1, 0], node[5, last - 1, 1])
    else:
        checks[5] = lambda a: (a[0], a[1]) == (node[5, last, 0], node[5, last, 1])
    # 6 / 7: charge_scale hits both clamps (checked by the caller with its own scales)
    node[6, :, 3] = f(0.25); node[7, :, 3] = f(1.5)
    return node, mc, env, ids, checks


def planted_cases(Side, N=65, M=3):
    side = E.BareSide(Side, 8, N, M)
    node, mc, env, ids, checks = planted(N, M)
    got, got64 = run_case(side, node, mc, env, ids, tag="planted")
    for e, ok in checks.items():
        assert ok(got[e]), (e, got[e])
    assert got[6, 2] == np.float32(0.75) and got[7, 2] == 0            # 1 - 0.25; 1 - 1.5 < 0: the lower clamp
    hi, _ = run_case(side, node, mc, env, ids, charge_scale=8.0, tag="scale 8")
    assert hi[6, 2] == 1 and hi[7, 2] == 0                             # the upper clamp
    lo, _ = run_case(side, node, mc, env, ids, charge_scale=-2.0, tag="scale -2")
    assert lo[6, 2] == 0 and lo[7, 2] == 1                             # -2 * -0.5 = 1
    nan_level = node.copy(); nan_level[0, :, 3] = np.nan
    got, _ = run_case(side, nan_level, mc, env, ids, tag="NaN level")
    assert got[0, 2] == 0
    side.close()


def test_emulated_heuristic_planted():
    planted_cases(EmuSide)


def test_emulated_heuristic_planted_single_charger():
    planted_cases(EmuSide, N=64, M=1)


# ------------------------------------------------------------------------------------------------------------ 3. properties
def rows_are_independent(Side):
    """A row's bytes do not change when the rows are permuted, when every other row is NaN-laden, or when the call is repeated; NaN and
    inf in padded (dead) node rows have no effect."""
    N, M = 65, 3
    side = E.BareSide(Side, B0, N, M)
    node, mc, env, ids = rows_for(N, M)
    base, _ = run_case(side, node, mc, env, ids, tag="base")
    again, _ = run_case(side, node, mc, env, ids, tag="again")
    assert E.same(base, again)
    perm = np.array([3, 5, 0, 1, 4, 2])
    got, _ = run_case(side, node[perm], mc[perm], env[perm], ids[perm], tag="permuted")
    assert E.same(got, base[perm])
    for keep in (0, 3):
        n2, m2, e2 = node.copy(), mc.copy(), env.copy()
        others = [e for e in range(B0) if e != keep]
        n2[others] = np.nan; m2[others] = np.nan; e2[others] = np.nan
        got, _ = run_case(side, n2, m2, e2, ids, tag=("laden", keep))
        assert E.same(got[keep], base[keep])
    dead = node[..., 7] != 1
    n3 = node.copy(); n3[dead, 2:7] = np.nan; n3[dead, 0] = np.inf
    got, _ = run_case(side, n3, mc, env, ids, tag="NaN in dead rows")
    assert E.same(got, base)
    side.close()


def test_emulated_heuristic_rows_are_independent():
    rows_are_independent(EmuSide)


def bad_arguments(Side):
    """Every WRSN_ERR_ARG case leaves the outputs untouched, and the valid call that follows gives the reference's bytes."""
    from multi_agent_rl_wrsn_amd._lib import WrsnError
    N, M = 33, 3
    side = E.BareSide(Side, B0, N, M)
    node, mc, env, ids = rows_for(N, M)
    call = E.HeuristicCall(side, node, mc, env, ids)
    nd, mp, ev = call.ent.ptrs()
    for over in (dict(agent_ptr=0), dict(action=0), dict(ent=None), dict(ent=(0, mp, ev)), dict(ent=(nd, 0, ev)), dict(ent=(nd, mp, 0)),
                 dict(ent=(nd + 4, mp, ev)), dict(ent=(nd, mp + 8, ev)), dict(ent=(nd, mp, ev + 4))):
        with pytest.raises(WrsnError) as ei:
            call.run(**over)
        assert ei.value.code == WRSN_ERR_ARG, over
        R.sync(side)
        assert call.act.untouched() and call.act64.untouched(), over
    want = call.expected(node, mc, env, ids)
    got = call.run()
    assert E.same(got[0], want[0]) and E.same(got[1], want[1])
    only32 = E.HeuristicCall(side, node, mc, env, ids)            # action_f64 may be NULL
    a32, _ = only32.run(action_f64=0)
    assert E.same(a32, want[0]) and only32.act64.untouched()
    assert side.handle.lib.wrsn_entity_heuristic_act(None, None, None, 1.0, None, None) == WRSN_ERR_ARG
    side.close()


def test_emulated_heuristic_bad_arguments():
    bad_arguments(EmuSide)


# ------------------------------------------------------------------------------------------------------------ 4. the simulator's own rows
def simulator_rows(Side):
    """B = 8, N = 33, M = 3 after a few steps: on the registered entity rows (ent == NULL) the call gives the reference's bytes, the
    action lies in the frame, and it is a node's position."""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    side = Side([synth_scenario(70 + e, 33, 30) for e in range(8)], DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True)
    side.reset()
    rng = np.random.default_rng(5)
    for _ in range(4):
        side.step(side._host()["agent_id"], rng.random((8, 3)))
    ids = side._host()["agent_id"]
    assert (ids >= 0).any()
    ent = side.ent if side.device is None else None
    if ent is None:                                            # the device side: the tensors VecWRSN registered
        node, mc, env = (x.cpu().numpy() for x in (side.env.nodes_feat, side.env.chargers_feat, side.env.env_feat))
    else:
        node, mc, env = ent.rows(ent.snap(), slice(None))
    call = E.HeuristicCall(side, node, mc, env, ids)
    got = call.run(ent=None)
    want = call.expected(node, mc, env, ids)
    assert E.same(got[0], want[0]) and E.same(got[1], want[1])
    for e in np.nonzero(ids >= 0)[0]:
        assert ((got[0][e] >= 0) & (got[0][e] <= 1)).all()
        assert any(tuple(got[0][e, :2]) == tuple(r[:2]) for r in node[e])
    side.close()


def test_emulated_heuristic_simulator_rows():
    simulator_rows(EmuSide)
