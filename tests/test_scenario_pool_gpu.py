"""Scenario pools on a real MI355X through VecWRSN: the reference fixtures and the load equivalence in float32 and bfloat16
observations, every launch mode against a blocking twin, the launch configuration of a denser pool, the roll-out bookkeeping and
BatchedIPPO over a pooled environment."""
import numpy as np
import pytest

from multi_agent_rl_wrsn_amd import _lib
from sides import decision_dict, need_gpu

pytestmark = pytest.mark.gpu

FIELDS = ("agent_id", "reward", "terminal", "now", "status")
POOL_FIXTURES = ("hanoi1000n50_m2_cap9000_detour", "sonla1000n50_m2_s4", "redundant_m2_deaths")


def _rows(env):
    """Host copies of the request rows: one tuple (agent, now, reward, terminal, status) per environment."""
    aid = env.agent_id.cpu().numpy(); now = env.now.cpu().numpy(); rw = env.reward.cpu().numpy()
    term = env.terminal.cpu().numpy(); st = env.status.cpu().numpy()
    return [(int(aid[e]), float(now[e]), float(rw[e]), int(term[e]), int(st[e])) for e in range(env.num_env)]


def _same_as_rounded(env16, env32, rows):
    """Request rows bit for bit, bfloat16 observations = the float32 ones rounded to nearest even."""
    torch = need_gpu()
    for k in FIELDS:
        assert torch.equal(getattr(env16, k), getattr(env32, k)), k
    if len(rows):
        idx = torch.as_tensor(rows, device=env32.device, dtype=torch.long)
        assert torch.equal(env16.state[idx], env32.state[idx].to(torch.bfloat16))


def test_terminal_rows_restart_in_the_drawn_fixture_f32_and_bf16():
    """tests/test_scenario_pool.py::test_terminal_rows_restart_in_the_drawn_fixture through VecWRSN.step on the device: a float32 batch
    held to the reference fixtures, a bfloat16 batch in lockstep held to the float32 one."""
    torch = need_gpu()
    from conftest import load_golden
    from multi_agent_rl_wrsn_amd import VecWRSN, build_scenario_pool, pool_draw
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    from parity import check_decision, close
    N, T, M, P, seed = 82, 56, 2, 3, 2
    fx = []
    for n in POOL_FIXTURES:
        z = load_golden(n); sc, mc = scenario_from_golden(z)
        fx.append((z, sc, mc))
    pool = torch.cat([build_scenario_pool([sc], mc, M, n_node=N, n_target=T) for _, sc, mc in fx], 0)
    assert pool.shape[0] == P
    envs = {}
    for dt in ("float32", "bfloat16"):
        env = VecWRSN([sc for _, sc, _ in fx], fx[0][2], M, auto_reset=True, obs_dtype=dt)
        assert (env.n_node, env.n_target) == (N, T) and env.record_bytes() == pool.shape[1]
        env.reset()
        env.load_envs(pool)                                   # environment e starts in fixture e, with that fixture's chargers
        env.set_pool(pool, seed)
        assert np.array_equal(env.pool_info()["record"], [-1] * 3) and np.array_equal(env.pool_info()["swaps"], [0] * 3)
        envs[dt] = env
    ev, e16 = envs["float32"], envs["bfloat16"]
    cur = [0, 1, 2]; k = [0, 0, 0]; swaps = [0, 0, 0]; pending = [False] * 3; episodes = [0, 0, 0]
    noise = []; checked = 0
    for call in range(80):
        if min(episodes) >= 2:
            break
        ids = np.full(3, -2, dtype=np.int32); act = np.zeros((3, 3))
        for e in range(3):
            if pending[e]:
                ids[e] = -1
            elif episodes[e] < 2:
                z = fx[cur[e]][0]
                ids[e] = int(z["in_agent"][k[e]]); act[e] = z["in_action"][k[e]]
        before = _rows(ev)
        for env in (ev, e16):
            env.step(torch.tensor(ids), torch.tensor(act))
        rows = _rows(ev)
        _same_as_rounded(e16, ev, [e for e in range(3) if ids[e] != -2 and rows[e][0] >= 0])
        info = ev.pool_info()
        for e in range(3):
            if pending[e]:
                rec = pool_draw(seed, e, swaps[e], P)
                swaps[e] += 1; cur[e] = rec; k[e] = 0; pending[e] = False
                z, sc, _ = fx[rec]
                assert rows[e][4] == 3 and rows[e][0] == int(z["reset_agent"]) and rows[e][2] == 0.0 and rows[e][3] == 0
                nd = ev.nodes()
                assert close(nd["energy"][e][:sc.n_node], z["reset_node_energy"]) and close(nd["cs"][e][:sc.n_node], z["reset_node_cs"], atol=1e-9)
                assert np.array_equal(nd["status"][e][:sc.n_node], z["reset_node_status"])
                obs = ev.state[e].double().cpu().numpy()
                assert np.max(np.abs(obs - z["reset_obs"])) <= 1e-5 * max(1.0, np.abs(z["reset_obs"]).max())
            elif ids[e] == -2:
                assert rows[e] == before[e]
            else:
                z, sc, _ = fx[cur[e]]
                check_decision(z, k[e], decision_dict(ev._result(), ev.state[e].double().cpu().numpy(), ev._h, e, sc), where="%s (env %d, episode %d)" % (POOL_FIXTURES[cur[e]], e, episodes[e]), noise=noise)
                checked += 1
                if z["terminal"][k[e]]:
                    pending[e] = True; episodes[e] += 1
                k[e] += 1
            assert (int(info["record"][e]), int(info["swaps"][e])) == (cur[e] if swaps[e] else -1, swaps[e]), (call, e)
        assert np.array_equal(e16.pool_info()["record"], info["record"])
    assert min(episodes) >= 2 and min(swaps) >= 1 and checked >= 8 + 7 + 16 + 3 * 7
    assert len(noise) <= 4, noise
    ev.close(); e16.close()


@pytest.mark.parametrize("obs_dtype", ["float32", "bfloat16"])
def test_masked_pool_reset_equals_a_load(obs_dtype):
    """VecWRSN.pool_reset(mask, index) against VecWRSN.load_envs of the same records into the same rows of a twin, more than one
    64-row strip of the select kernel and a batch that is no multiple of it; the bfloat16 rows are the float32 rows rounded."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, build_scenario_pool, synth_scenario
    B, M, P, G = 150, 2, 5, 20
    own = [synth_scenario(31 + e % 7, 60, 40) for e in range(B)]
    others = [synth_scenario(41 + i, 50 + 3 * i, 30 + i) for i in range(P)]
    kw = dict(warm_up_time=5.0, map_size=G)
    pool = build_scenario_pool(others, None, M, n_node=62, n_target=40, chunk=2, **kw)
    assert pool.shape[0] == P
    a = VecWRSN(own + [others[-1]], None, M, obs_dtype=obs_dtype, **kw)          # (the last environment fixes n_node = 62)
    b = VecWRSN(own + [others[-1]], None, M, obs_dtype=obs_dtype, **kw)
    ref = VecWRSN(own + [others[-1]], None, M, **kw) if obs_dtype == "bfloat16" else None
    B += 1
    assert a.record_bytes() == pool.shape[1]
    rng = np.random.RandomState(5)
    envs = [x for x in (a, b, ref) if x is not None]
    act = torch.tensor(rng.rand(B, 3) * np.array([1.0, 1.0, 0.2]))
    for env in envs:
        env.reset(); env.step(env.agent_id.clone(), act)
    a.set_pool(pool, 9)
    if ref is not None:
        ref.set_pool(pool, 9)
    mask = rng.rand(B) < 0.4; mask[[0, 63, 64, 127, 128, B - 1]] = True; mask[[1, 65]] = False
    index = rng.randint(0, P, B); index[~mask] = 1000                    # (indices of rows not selected are not read)
    sel = np.nonzero(mask)[0]; unsel = np.nonzero(~mask)[0]
    for env in envs:
        env.agent_id.fill_(-77); env.status.fill_(-77); env.reward.fill_(-12345.5); env.now.fill_(-12345.5); env.terminal.fill_(99)
        env.state.fill_(-12345.5)
    a.pool_reset(torch.tensor(mask), torch.tensor(index))
    b.load_envs(pool[torch.as_tensor(index[sel], device=pool.device, dtype=torch.long)], sel)
    for k in FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert int((a.status[torch.as_tensor(sel)] == 0).sum()) == len(sel)
    assert torch.equal(a.state, b.state)                                 # replaced rows rendered alike, the others still sentinels
    u = torch.as_tensor(unsel, device=a.device)
    assert bool((a.agent_id[u] == -77).all()) and bool((a.now[u] == -12345.5).all()) and bool((a.terminal[u] == 99).all())
    assert bool((a.state[u].float() == torch.tensor(-12345.5).to(a.state.dtype).float()).all())
    for name, pa in a.nodes().items():
        assert np.array_equal(pa, b.nodes()[name]), name
    assert np.array_equal(a._h.peek(_lib.PEEK_MC), b._h.peek(_lib.PEEK_MC)) and np.array_equal(a._h.peek(_lib.PEEK_ENV), b._h.peek(_lib.PEEK_ENV))
    info = a.pool_info()
    assert np.array_equal(info["record"][sel], index[sel]) and np.array_equal(info["swaps"], mask.astype(np.int32))
    assert np.array_equal(info["record"][unsel], [-1] * len(unsel)) and np.array_equal(b.pool_info()["record"], [-1] * B)
    if ref is not None:
        ref.pool_reset(torch.tensor(mask), torch.tensor(index))
        _same_as_rounded(a, ref, sel)
    for env in envs:                                                       # the rows not selected were mid-episode: their requests back
        env.agent_id[u] = -1; env.status[u] = 0
    for k in range(4):
        act = torch.tensor(rng.rand(B, 3) * np.array([1.0, 1.0, 0.2]))
        ids = a.agent_id.clone()
        for env in envs:
            env.step(ids.clone(), act)
        for f in FIELDS:
            assert torch.equal(getattr(a, f), getattr(b, f)), (k, f)
        m = a.agent_id >= 0
        assert torch.equal(a.state[m], b.state[m]), k
        if ref is not None:
            _same_as_rounded(a, ref, torch.nonzero(m).flatten().tolist())
    assert np.array_equal(a.nodes()["energy"], b.nodes()["energy"])
    for env in envs:
        env.close()


def _pooled_batch(B, P, seed, own_seed=13000, pool_seed=13100, M=3, **kw):
    from multi_agent_rl_wrsn_amd import VecWRSN, build_scenario_pool, synth_scenario
    own = [synth_scenario(own_seed + u, 50, 40) for u in range(32)]
    pool_scs = [synth_scenario(pool_seed + i, 50, 40) for i in range(P)]
    map_size = kw.get("map_size", 100)
    pool = build_scenario_pool(pool_scs, None, M, map_size=map_size, n_node=50, n_target=40)
    env = VecWRSN([own[e % 32] for e in range(B)], None, M, auto_reset=True, **kw)
    env.set_pool(pool, seed)
    return env, [own[e % 32] for e in range(B)], pool_scs, pool


def _drive_pooled(env, acts, K, rounds=4000):
    """Per environment its first K requests (status-3 rows included) of a run in which its j-th request that asks for an action gets
    acts[j, e] (a status-4 row's action is not looked at, so it is not used up), and the pool record of each of its swaps."""
    torch = need_gpu()
    B = env.num_env
    j = np.zeros(B, dtype=int); busy = env.status.cpu().numpy() == 4
    hist = [[] for _ in range(B)]; recs = [[] for _ in range(B)]
    swaps = env.pool_info()["swaps"].copy()
    for _ in range(rounds):
        if min(len(h) for h in hist) >= K:
            break
        ids = env.agent_id.cpu().numpy().copy()
        act = np.zeros((B, 3))
        for e in range(B):
            if busy[e]:
                ids[e] = -1
            else:
                act[e] = acts[min(j[e], len(acts) - 1), e]; j[e] += 1
        env.step(torch.tensor(ids, dtype=torch.int32), torch.tensor(act))
        rows = _rows(env)
        info = env.pool_info()
        for e in range(B):
            if info["swaps"][e] != swaps[e]:
                assert info["swaps"][e] == swaps[e] + 1 and rows[e][4] == 3, (e, rows[e])
                recs[e].append(int(info["record"][e]))
            if rows[e][4] != 4:
                hist[e].append(rows[e])
        busy = np.array([r[4] == 4 for r in rows]); swaps = info["swaps"].copy()
    assert min(len(h) for h in hist) >= K
    return [h[:K] for h in hist], recs


@pytest.mark.parametrize("mode", ["budget", "pipeline", "deadline"])
def test_pooled_auto_reset_under_every_launch_mode(mode, monkeypatch):
    """B = 512 (the smallest batch the pipeline takes) 50-node environments over a pool of 16, random actions, against a blocking pooled
    twin given the same action for the same decision: agent, time, terminal and the sequence of pool records identical, rewards to the
    tolerance the launch-mode tests of test_gpu_parity hold a budgeted or time-sliced run to."""
    need_gpu()
    from multi_agent_rl_wrsn_amd import pool_draw
    B, P, K, seed = 512, 16, 48, 7
    kw = {"budget": dict(step_budget=1250), "pipeline": dict(step_budget=1250), "deadline": dict(step_deadline_us=100)}[mode]
    if mode == "budget":
        monkeypatch.setenv("WRSN_PIPE", "0")                  # (read when the handle is created: one launch per step call)
    env, _, _, _ = _pooled_batch(B, P, seed, **kw)
    monkeypatch.delenv("WRSN_PIPE", raising=False)
    twin, _, _, _ = _pooled_batch(B, P, seed)
    acts = np.random.RandomState(3).rand(K, B, 3)
    env.reset(); twin.reset()
    want, want_recs = _drive_pooled(twin, acts, K)
    got, got_recs = _drive_pooled(env, acts, K)
    n_swaps = np.array([sum(1 for q in h if q[4] == 3) for h in want])
    assert (n_swaps >= 2).sum() >= B // 2, "the run must swap: %d of %d environments swapped twice" % ((n_swaps >= 2).sum(), B)
    for e in range(B):
        n = int(n_swaps[e])
        assert want_recs[e][:n] == [pool_draw(seed, e, k, P) for k in range(n)], e
        assert got_recs[e][:n] == want_recs[e][:n], (mode, e)
        for qa, qb in zip(got[e], want[e]):
            assert qa[0] == qb[0] and qa[1] == qb[1] and qa[3] == qb[3] and qa[4] == qb[4], (mode, e, qa, qb)
            assert abs(qa[2] - qb[2]) <= 1e-7 * max(1.0, abs(qa[2])), (mode, e, qa, qb)
    env.close(); twin.close()


def test_masked_swap_of_a_row_in_flight_drops_the_step():
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN
    B, P = 64, 4
    env, _, pool_scs, _ = _pooled_batch(B, P, 1, step_budget=150)
    g = np.random.RandomState(2)
    r = env.reset()
    flying = []
    for k in range(40):
        r = env.step(r["agent_id"].clone(), torch.tensor(g.rand(B, 3)))
        flying = torch.nonzero(r["status"] == 4).flatten().tolist()
        if flying:
            break
    assert flying, "no step in flight"
    e = flying[0]
    before = _rows(env)
    mask = np.zeros(B, dtype=np.uint8); mask[e] = 1
    env.pool_reset(torch.tensor(mask), torch.full((B,), 3, dtype=torch.int32))
    fresh = VecWRSN([pool_scs[3]], None, 3)
    fresh.reset()
    rows = _rows(env)
    assert rows[e][:4] == _rows(fresh)[0][:4] and rows[e][4] == 0
    assert torch.equal(env.state[e], fresh.state[0])
    assert [rows[x] for x in range(B) if x != e] == [before[x] for x in range(B) if x != e]
    act = g.rand(3)
    fresh.step(fresh.agent_id.clone(), torch.tensor(act[None]))
    ids = torch.full((B,), -2, dtype=torch.int32); ids[e] = rows[e][0]
    for k in range(200):                                      # nothing of the old occupant's step is left: the new one's first step, in as many launches as its budget needs
        r = env.step(ids, torch.tensor(np.tile(act, (B, 1))))
        if int(r["status"][e]) != 4:
            break
        ids[e] = -1
    want = _rows(fresh)[0]; got = _rows(env)[e]
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3] and got[4] == want[4], (got, want)
    assert abs(got[2] - want[2]) <= 1e-7 * max(1.0, abs(want[2]))
    env.close(); fresh.close()


def test_episode_after_a_swap_is_that_scenarios_episode():
    """Blocking mode: every request of the first episode after an environment's first swap is bit-identical to a fresh handle built
    from the drawn scenario with wrsn_set_scenario + reset and given the same actions."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, pool_draw
    B, P, K, seed = 32, 8, 48, 5
    env, _, pool_scs, _ = _pooled_batch(B, P, seed, map_size=20)
    acts = np.random.RandomState(8).rand(K, B, 3)
    env.reset()
    hist = [[] for _ in range(B)]; states = [[] for _ in range(B)]
    for j in range(K):
        ids = env.agent_id.clone()
        env.step(ids, torch.tensor(acts[j]))
        rows = _rows(env); st = env.state.cpu()
        for e in range(B):
            hist[e].append(rows[e]); states[e].append(st[e].clone())
    fresh = VecWRSN([pool_scs[pool_draw(seed, e, 0, P)] for e in range(B)], None, 3, map_size=20)
    fresh.reset()
    first = [next((j for j, q in enumerate(hist[e][:K - 1]) if q[4] == 3), None) for e in range(B)]
    assert sum(f is not None for f in first) >= B // 2
    rows = _rows(fresh); st = fresh.state.cpu()
    step_of = {}
    for e in range(B):
        if first[e] is not None:
            assert hist[e][first[e]][:4] == rows[e][:4], e
            assert torch.equal(states[e][first[e]], st[e]), e
            step_of[e] = first[e] + 1
    compared = 0
    while step_of:
        ids = torch.full((B,), -2, dtype=torch.int32); act = np.zeros((B, 3))
        for e, j in step_of.items():
            ids[e] = int(fresh.agent_id[e]); act[e] = acts[j, e]
        fresh.step(ids, torch.tensor(act))
        rows = _rows(fresh); st = fresh.state.cpu()
        for e, j in list(step_of.items()):
            assert hist[e][j] == rows[e], (e, j, hist[e][j], rows[e])
            if rows[e][0] >= 0:
                assert torch.equal(states[e][j], st[e]), (e, j)
            compared += 1
            if rows[e][3] or j + 1 >= K:
                del step_of[e]
            else:
                step_of[e] = j + 1
    assert compared >= 4 * B // 2
    env.close(); fresh.close()


def _conn_bound(records):
    """WrsnRecHeader.conn_bound of every record (int32 at byte 44)."""
    return records[:, 44:48].cpu().numpy().copy().view(np.int32).reshape(-1)


def test_denser_pool_record_gets_its_launch_configuration():
    """A pool whose network needs longer connected-node lists than any scenario the handle was built with: wrsn_pool_set fits the launch
    configuration, and the swapped environments step to the requests of a fresh handle of that scenario."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import DEFAULT_NODE_SPEC, VecWRSN, build_scenario_pool, synth_scenario
    B, M = 6, 3
    sparse = [synth_scenario(14000 + e, 100, 60) for e in range(B)]
    spec = dict(DEFAULT_NODE_SPEC); spec["com_range"] = 40.1           # half the radio range: twice the nodes around a charging spot
    dense = synth_scenario(14100, 100, 60, side=500.0, node_spec=spec)
    env = VecWRSN(sparse, None, M)
    pool = build_scenario_pool([dense], None, M, n_node=100, n_target=60)
    cb_own = int(_conn_bound(env.save_envs()).max()); cb_pool = int(_conn_bound(pool)[0])
    assert (cb_pool + 3) // 4 > max(1, (cb_own + 3) // 4), (cb_pool, cb_own)      # another WrsnDev.CC: LDS and wave slots of the step kernel
    env.reset()
    env.set_pool(pool)
    mask = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8)
    r = env.pool_reset(mask, torch.zeros(B, dtype=torch.int32))
    fresh = VecWRSN([dense] * B, None, M)
    rf = fresh.reset()
    sel = torch.nonzero(mask).flatten().cuda()
    rng = np.random.RandomState(4)
    for k in range(8):
        for f in FIELDS:
            assert torch.equal(r[f][sel], rf[f][sel]), (k, f)
        m = sel[r["agent_id"][sel] >= 0]
        assert torch.equal(r["state"][m], rf["state"][m]), k
        act = torch.tensor(np.tile(rng.rand(1, 3), (B, 1)))
        r = env.step(r["agent_id"].clone(), act); rf = fresh.step(rf["agent_id"].clone(), act)
    env.close(); fresh.close()


def test_rollout_bookkeeping_over_a_pooled_batch():
    """TransitionBuffers over a pooled batch against a host-side shadow of the run: every stored transition belongs to one episode of
    one pool record (a charger's action of the episode before a swap completes nothing), and the rollout table counts every terminal
    return, because a swapped environment keeps its own roll[]."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import TransitionBuffers
    B, P, M, K = 16, 4, 3, 60
    env, _, _, _ = _pooled_batch(B, P, 3, map_size=20)
    buf = TransitionBuffers(env, 1024, 3)
    g = torch.Generator().manual_seed(1)
    r = env.reset()
    acted = np.zeros((B, M), dtype=bool); want = [set() for _ in range(M)]
    terminals = 0; swapped = 0
    for k in range(K):
        ids = r["agent_id"].clone(); act = torch.rand((B, 3), generator=g)
        buf.record(ids, act, torch.zeros(B))
        hid = ids.cpu().numpy()
        for e in range(B):
            if hid[e] >= 0:
                acted[e, hid[e]] = True
        r = env.step(ids, act.double())
        buf.collect()
        for e, (aid, now, rw, term, st) in enumerate(_rows(env)):
            if term or st == 3:                               # episode over / restarted in another network: what was pending is dropped
                acted[e] = False
                terminals += int(term); swapped += int(st == 3)
            elif aid >= 0 and acted[e, aid]:
                want[aid].add((e, now))
    n = buf.stored()
    assert swapped >= B and sum(n) > 0
    for a in range(M):
        got = list(zip(buf.env_index[a, :n[a]].cpu().tolist(), buf.now[a, :n[a]].cpu().tolist()))
        assert len(got) == len(set(got)) and set(got) == want[a], (a, sorted(set(got) ^ want[a]))
    assert int(env.rollout_table()[:, M].sum()) == terminals
    assert int(env.pool_info()["swaps"].sum()) == swapped == terminals - int(env.terminal.sum())
    env.close()


def test_batched_ippo_rolls_out_over_a_pooled_batch():
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import BatchedIPPO
    torch.manual_seed(0); np.random.seed(0)
    B, M, G = 64, 3, 16
    env, _, _, _ = _pooled_batch(B, 8, 11, map_size=G)
    algo = BatchedIPPO(dict(batch_size=8, minibatch_size=8, n_updates_per_iteration=1), env, capacity=256)
    batches = algo.roll_out(max_launches=200)
    assert min(algo.buffers.counts()) >= 8
    for a in range(M):
        assert batches[a]["states"].shape == (8, 4, G, G) and bool(torch.isfinite(batches[a]["returns"]).all())
    episodes = int(env.rollout_table()[:, M].sum())
    assert int(env.pool_info()["swaps"].sum()) == episodes - int(env.terminal.sum())
    env.close()
