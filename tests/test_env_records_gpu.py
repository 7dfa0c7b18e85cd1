"""Environment records on a real MI355X: save / load / clone at the headline geometry, under every launch mode, with observation
reuse, prob_gp < 1, the roll-out bookkeeping, 1000-node networks and through the WRSN facade."""
import numpy as np
import pytest
from sides import need_gpu

pytestmark = pytest.mark.gpu

FIELDS = ("agent_id", "reward", "terminal", "now", "status")


def _assert_rows_equal(ra, rb, ia=None, ib=None, state=True):
    """Request rows ia of ra and ib of rb bit for bit (state: rows with a charger only -- the others are left untouched)."""
    torch = need_gpu()
    for k in FIELDS:
        a, b = ra[k], rb[k]
        if ia is not None:
            a, b = a[ia], b[ib]
        assert torch.equal(a, b), k
    if state and ra["state"] is not None:
        sa, sb = ra["state"], rb["state"]
        aid = ra["agent_id"]
        if ia is not None:
            sa, sb, aid = sa[ia], sb[ib], aid[ia]
        m = aid >= 0
        assert torch.equal(sa[m], sb[m])


def test_headline_geometry_resume_is_bit_identical():
    """4096 x 200 nodes x 3 chargers, blocking mode, auto-reset: 40 steps, save every environment, 40 more; the records (through the
    host) loaded into a batch built from other scenarios replay the same 40 steps bit for bit."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    B, U, M, K = 4096, 64, 3, 40
    scs = [synth_scenario(7100 + u, 200, 200) for u in range(U)]
    other = [synth_scenario(7300 + u, 200, 200) for u in range(U)]
    a = VecWRSN([scs[e % U] for e in range(B)], None, M, auto_reset=True)
    g = torch.Generator().manual_seed(11)
    acts = torch.rand((2 * K, B, 3), generator=g, dtype=torch.float64).cuda()
    r = a.reset()
    for k in range(K):
        r = a.step(r["agent_id"].clone(), acts[k])
    rec = a.save_envs().cpu()
    assert rec.shape == (B, a.record_bytes()) and a.record_bytes() % 256 == 0
    b = VecWRSN([other[e % U] for e in range(B)], None, M, auto_reset=True)
    rb = b.reset()
    rb = b.load_envs(rec)
    _assert_rows_equal(r, rb)
    for k in range(K, 2 * K):
        r = a.step(r["agent_id"].clone(), acts[k])
        rb = b.step(rb["agent_id"].clone(), acts[k])
        _assert_rows_equal(r, rb)
    assert np.array_equal(a.nodes()["energy"], b.nodes()["energy"])
    a.close(); b.close()


def _drive(env, acts, K, H, rounds=400):
    """Per environment the first K requests of a run driven by acts[j, e % H] for its j-th decision (a status-4 row's action is not
    looked at, so it is not used up)."""
    torch = need_gpu()
    B = env.num_env
    j = np.zeros(B, dtype=int); busy = env.status.cpu().numpy() == 4
    hist = [[] for _ in range(B)]
    for _ in range(rounds):
        if min(len(h) for h in hist) >= K:
            break
        ids = env.agent_id.cpu().numpy().copy()
        act = np.zeros((B, 3))
        for e in range(B):
            if busy[e]:
                ids[e] = -1
            else:
                act[e] = acts[min(j[e], len(acts) - 1), e % H]; j[e] += 1
        r = env.step(torch.tensor(ids, dtype=torch.int32), torch.tensor(act))
        st = r["status"].cpu().numpy(); aid = r["agent_id"].cpu().numpy(); now = r["now"].cpu().numpy()
        rw = r["reward"].cpu().numpy(); term = r["terminal"].cpu().numpy()
        busy = st == 4
        for e in range(B):
            if not busy[e]:
                hist[e].append((int(aid[e]), float(now[e]), float(rw[e]), int(term[e]), int(st[e])))
    assert min(len(h) for h in hist) >= K
    return [h[:K] for h in hist]


@pytest.mark.parametrize("mode", ["budget", "pipeline", "deadline"])
def test_clone_under_every_launch_mode(mode):
    """Clone the first half of the batch onto the second half (rows in flight and latched actions included) and continue both halves
    with equal actions: agent, time and terminal identical, rewards to round-off."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    B = 256 if mode == "budget" else 512
    H, M, K = B // 2, 3, 5
    kw = {"budget": dict(step_budget=1250), "pipeline": dict(step_budget=1250), "deadline": dict(step_deadline_us=100)}[mode]
    uniq = [synth_scenario(7500 + u, 200, 200) for u in range(32)]
    env = VecWRSN([uniq[e % 32] for e in range(H)] + [uniq[(e + 7) % 32] for e in range(H)], None, M, auto_reset=True, **kw)
    g = np.random.RandomState(2)
    r = env.reset()
    in_flight = 0
    for k in range(30):
        ids = r["agent_id"].clone()
        r = env.step(ids, torch.tensor(g.rand(B, 3) * np.array([1.0, 1.0, 0.5])))
        in_flight = int((r["status"][:H] == 4).sum())
        if k >= 3 and in_flight > 0:
            break
    assert in_flight > 0, "no step in flight to clone"
    env.clone_envs(np.arange(H), np.arange(H, B))
    _assert_rows_equal(env._result(), env._result(), torch.arange(H), torch.arange(H, B))
    acts = g.rand(K + 4, H, 3) * np.array([1.0, 1.0, 0.5])
    hist = _drive(env, acts, K, H, rounds=2000)
    for e in range(H):
        for qa, qb in zip(hist[e], hist[e + H]):
            # agent, time and terminal identical; each half is suspended at its own points (budget taper by launch position, time
            # slices by timing), which re-bases the float32 reward-priority pipeline: rewards to round-off, with the tolerance the
            # launch-mode tests of test_gpu_parity hold a budgeted or time-sliced run to against a blocking one
            assert qa[0] == qb[0] and qa[1] == qb[1] and qa[3] == qb[3], (mode, e, qa, qb)
            assert abs(qa[2] - qb[2]) <= 1e-7 * max(1.0, abs(qa[2])), (mode, e, qa, qb)
    env.close()


def test_observation_reuse_after_load_and_clone_equals_a_full_render():
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    B, M = 64, 3
    scs = [synth_scenario(7700 + e, 200, 200) for e in range(B)]
    a = VecWRSN(scs, None, M, auto_reset=True, reuse_obs=True)
    b = VecWRSN(scs[::-1], None, M, auto_reset=True, reuse_obs=True)
    g = torch.Generator().manual_seed(4)
    r = a.reset(); rb = b.reset()
    for k in range(6):
        r = a.step(r["agent_id"].clone(), torch.rand((B, 3), generator=g, dtype=torch.float64))
        rb = b.step(rb["agent_id"].clone(), torch.rand((B, 3), generator=g, dtype=torch.float64))

    def check(env):
        aid = env.agent_id.clone()
        full = env.render_state(aid)
        m = aid >= 0
        assert int(m.sum()) > 0 and torch.equal(env.state[m], full[m])
    b.load_envs(a.save_envs(np.arange(0, B, 2)), np.arange(1, B, 2))
    check(b)
    a.clone_envs(np.arange(0, B // 2), np.arange(B // 2, B))
    check(a)
    for k in range(4):
        act = torch.rand((B, 3), generator=g, dtype=torch.float64)
        r = a.step(a.agent_id.clone(), act); rb = b.step(b.agent_id.clone(), act)
        check(a); check(b)
    a.close(); b.close()


def test_prob_gp_batch_generator_follows_clone_and_load():
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import DEFAULT_NODE_SPEC, VecWRSN, synth_scenario
    from multi_agent_rl_wrsn_amd import _lib
    spec = dict(DEFAULT_NODE_SPEC); spec["prob_gp"] = 0.5
    B, H, M = 64, 32, 3
    scs = [synth_scenario(7900 + e, 200, 200, node_spec=spec, stochastic_packets=True) for e in range(B)]
    a = VecWRSN(scs, None, M)
    g = torch.Generator().manual_seed(9)
    r = a.reset()
    for k in range(5):
        r = a.step(r["agent_id"].clone(), torch.rand((B, 3), generator=g, dtype=torch.float64))
    rec = a.save_envs(np.arange(H))
    a.clone_envs(np.arange(H), np.arange(H, B))
    st = a._h.peek(_lib.PEEK_RNG_STATE)
    assert np.array_equal(st[:H], st[H:])
    b = VecWRSN(scs[::-1], None, M)
    b.reset()
    b.load_envs(rec)
    assert np.array_equal(b._h.peek(_lib.PEEK_RNG_STATE)[:H], st[:H])
    for k in range(5):
        act = torch.rand((H, 3), generator=g, dtype=torch.float64)
        r = a.step(a.agent_id.clone(), torch.cat([act, act]))
        ids_b = b.agent_id.clone(); ids_b[H:] = -2
        rb = b.step(ids_b, torch.cat([act, act]))
        _assert_rows_equal(r, r, torch.arange(H), torch.arange(H, B))
        _assert_rows_equal(r, rb, torch.arange(H), torch.arange(H))
        st = a._h.peek(_lib.PEEK_RNG_STATE); sb = b._h.peek(_lib.PEEK_RNG_STATE)
        assert np.array_equal(st[:H], st[H:]) and np.array_equal(st[:H], sb[:H])
    a.close(); b.close()


def test_rollout_collect_appends_nothing_for_restored_rows():
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import TransitionBuffers, VecWRSN, synth_scenario
    B, M = 16, 3
    env = VecWRSN([synth_scenario(8100 + e, 100, 80) for e in range(B)], None, M, auto_reset=True)
    buf = TransitionBuffers(env, 64, 3)
    r = env.reset()
    g = torch.Generator().manual_seed(1)
    for k in range(4):
        act = torch.rand((B, 3), generator=g)
        buf.record(r["agent_id"].clone(), act, torch.zeros(B))
        r = env.step(r["agent_id"].clone(), act.double())
        buf.collect()
    rec = env.save_envs(np.arange(4))
    n0 = np.asarray(buf.counts()).copy()
    env.load_envs(rec, np.arange(4, 8))
    buf.collect()
    assert np.array_equal(np.asarray(buf.counts()), n0)
    env.clone_envs(np.arange(8), np.arange(8, 16))
    buf.collect()
    assert np.array_equal(np.asarray(buf.counts()), n0)
    act = torch.rand((B, 3), generator=g)
    buf.record(env.agent_id.clone(), act, torch.zeros(B))
    env.step(env.agent_id.clone(), act.double())
    buf.collect()
    assert np.asarray(buf.counts()).sum() > n0.sum()                 # the bookkeeping goes on as usual after the restored rows stepped
    env.close()


def test_1000_node_8_charger_round_trip():
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    B, U, M = 256, 8, 8
    uniq = [synth_scenario(8300 + u, 1000, 1000) for u in range(U)]
    other = [synth_scenario(8400 + u, 1000, 1000) for u in range(U)]
    a = VecWRSN([uniq[e % U] for e in range(B)], None, M, auto_reset=True)
    g = torch.Generator().manual_seed(6)
    r = a.reset()
    for k in range(3):
        r = a.step(r["agent_id"].clone(), torch.rand((B, 3), generator=g, dtype=torch.float64))
    b = VecWRSN([other[e % U] for e in range(B)], None, M, auto_reset=True)
    b.reset()
    rb = b.load_envs(a.save_envs())
    _assert_rows_equal(r, rb)
    for k in range(3):
        act = torch.rand((B, 3), generator=g, dtype=torch.float64)
        r = a.step(r["agent_id"].clone(), act); rb = b.step(rb["agent_id"].clone(), act)
        _assert_rows_equal(r, rb)
    assert np.array_equal(a.nodes()["energy"], b.nodes()["energy"])
    a.close(); b.close()


def test_facade_lookahead_restores_the_request(tmp_path):
    need_gpu()
    import yaml
    from conftest import load_golden
    from multi_agent_rl_wrsn_amd import WRSN
    from multi_agent_rl_wrsn_amd.scenario import MC_SPEC_KEYS, NODE_SPEC_KEYS
    z = load_golden("hanoi1000n50_m3_s1")
    sp = tmp_path / "scen.yaml"; mp = tmp_path / "mc.yaml"
    sp.write_text(yaml.safe_dump({"node_phy_spe": {k: float(v) for k, v in zip(NODE_SPEC_KEYS, z["node_spec"])}, "seed": int(z["seed"]),
                                  "max_time": float(z["max_time"]), "base_station": [float(v) for v in z["bs_xy"]],
                                  "nodes": z["node_xy"].tolist(), "targets": z["target_xy"].tolist()}))
    mp.write_text(yaml.safe_dump({k: float(v) for k, v in zip(MC_SPEC_KEYS, z["mc_spec"])}))
    env = WRSN(str(sp), str(mp), 3, map_size=100)
    req = env.reset()
    for k in range(2):
        req = env.step(req["agent_id"], z["in_action"][k])
    snap = env.save_env()
    a, b = np.array([0.2, 0.7, 0.3]), np.array([0.9, 0.1, 0.6])
    first = env.step(req["agent_id"], a)
    back = env.load_env(snap)
    assert back["agent_id"] == req["agent_id"] and back["reward"] == req["reward"] and np.array_equal(back["state"], req["state"])
    assert env.env.now == snap.now
    env.step(back["agent_id"], b)                          # another branch from the same state
    env.load_env(snap)
    again = env.step(back["agent_id"], a)
    if first is None:
        assert again is None
        return
    assert set(again) == set(first)
    for k in first:
        if k == "info":
            continue
        x, y = first[k], again[k]
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y), k
        else:
            assert x == y, k


def test_clone_skips_the_request_fields_the_caller_leaves_out():
    import test_env_records as body
    from sides import VecSide
    body.clone_skips_the_request_fields_the_caller_leaves_out(VecSide)
