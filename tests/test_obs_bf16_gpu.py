"""bf16 observations (wrsn_set_obs_format, VecWRSN(obs_dtype="bfloat16")) on a real MI355X: the render kernel's bf16 instantiation in
every launch mode, the roll-out copy kernels, the environment records and the trainer, held to the float32 path bit for bit
(round to nearest even) and to the reference within the bound derived in tests/test_obs_bf16.py.

One allowance, because it is hardware behaviour: where the float32 value is subnormal (0 < |x| < 2^-126) the bf16 cell may be the
rounded value or a zero of the same sign.  A test that needed it says so with a warning."""
import warnings

import numpy as np
import pytest

from conftest import load_golden
from sides import need_gpu

pytestmark = pytest.mark.gpu

CANARY = -23101                                               # 0xA5C3 as int16
N_CANARY = 1 << 16


def _guarded(torch, shape, device="cuda:0"):
    """(raw, view): a bf16 tensor of `shape` that ends exactly where a canary region begins."""
    n = int(np.prod(shape))
    raw = torch.full((n + N_CANARY,), CANARY, dtype=torch.int16, device=device)
    raw[:n] = 0
    return raw, raw[:n].view(torch.bfloat16).view(*shape)


def _canary_ok(raw, n):
    return bool((raw[n:] == CANARY).all())


def _guard_state(torch, env):
    raw, view = _guarded(torch, tuple(env.state.shape), env.device)
    env.state = view                                          # VecWRSN hands out state.data_ptr()
    return raw


def _assert_rounded(torch, b16, f32, where):
    """b16 == RNE(f32) bit for bit, except that a float32 subnormal may also have become a zero of its sign."""
    got = b16.contiguous().view(torch.int16); want = f32.to(torch.bfloat16).contiguous().view(torch.int16)
    bad = got != want
    if not bool(bad.any()):
        return 0
    sub = (f32 != 0) & (f32.abs() < 2.0 ** -126)
    zero = torch.where(f32 < 0, torch.full_like(got, -32768), torch.zeros_like(got))
    allowed = bad & sub & (got == zero)
    assert bool((bad == allowed).all()), (where, int((bad & ~allowed).sum()), "cells differ from RNE(float32)")
    n = int(allowed.sum())
    warnings.warn("%s: %d float32-subnormal cells were flushed to zero by the bf16 store" % (where, n))
    return n


def _ref_ok(bits_bf16, ref):
    got = bits_bf16.double().cpu().numpy().reshape(np.shape(ref)); ref = np.asarray(ref, dtype=np.float64)
    peak = max(1.0, float(np.nanmax(np.abs(ref))))
    return bool(np.all(np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + (1 + 2.0 ** -8) * 1e-5 * peak))


def _batch(n, seed0=5200, uniq=64):
    from multi_agent_rl_wrsn_amd import synth_scenario
    u = [synth_scenario(seed0 + k, 200, 200) for k in range(uniq)]
    return [u[e % uniq] for e in range(n)]


@pytest.mark.parametrize("mode", ["blocking", "budget_pipeline"])
def test_bf16_equals_rounded_float32_side_by_side(mode):
    """9 (deterministic modes). B = 1024 synthetic 200-node environments, 3 chargers, random actions, auto-reset, 40 launches: a float32 and
    a bf16 VecWRSN stepped side by side return the same requests, and every bf16 row with a request is the rounded float32 row."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN
    B, M = 1024, 3
    scs = _batch(B)
    kw = dict(auto_reset=True, reuse_obs=True, step_budget=1250 if mode == "budget_pipeline" else 0)
    a = VecWRSN(scs, None, M, **kw)
    b = VecWRSN(scs, None, M, obs_dtype="bfloat16", **kw)
    assert a.state.dtype == torch.float32 and b.state.dtype == torch.bfloat16 and b.obs_dtype == torch.bfloat16
    raw = _guard_state(torch, b)
    g = torch.Generator().manual_seed(4)
    ra = a.reset(); rb = b.reset()
    _assert_rounded(torch, rb["state"], ra["state"], mode + " reset")
    n_rows = n_zero = n_flight = 0
    for k in range(40):
        act = torch.rand((B, 3), generator=g, dtype=torch.float64)
        now0 = ra["now"].clone()
        keep = rb["state"].clone()
        ra = a.step(ra["agent_id"].clone(), act); rb = b.step(rb["agent_id"].clone(), act)
        assert torch.equal(ra["agent_id"], rb["agent_id"]) and torch.equal(ra["now"], rb["now"]) and torch.equal(ra["status"], rb["status"])
        assert torch.equal(ra["reward"], rb["reward"])
        rows = ra["agent_id"] >= 0
        _assert_rounded(torch, rb["state"][rows], ra["state"][rows], "%s launch %d" % (mode, k))
        assert torch.equal(rb["state"][~rows].view(torch.int16), keep[~rows].view(torch.int16))       # no request: row untouched
        n_rows += int(rows.sum()); n_zero += int(((ra["now"] == now0) & (ra["status"] == 0) & rows).sum())
        n_flight += int((ra["status"] == 4).sum())
    assert _canary_ok(raw, b.state.numel())
    assert n_rows > 5 * B and n_zero > 100                    # rows with map 1 reused among them
    assert (n_flight > 0) == (mode == "budget_pipeline")      # steps in flight over several launches with a budget only
    a.close(); b.close()


def test_bf16_time_sliced_launches_render_the_rounded_float32_state():
    """9 (time slices). Which launch reports a request is timing-dependent, so the bf16 batch is compared with its OWN float32 render of the
    same state (raw handle switched to float32 and back): the rows of `state` with a request and a fresh bf16 render_state."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, _lib
    B, M, G = 1024, 3, 100
    env = VecWRSN(_batch(B), None, M, auto_reset=True, reuse_obs=True, step_deadline_us=400, obs_dtype=torch.bfloat16)
    raw = _guard_state(torch, env)
    g = torch.Generator().manual_seed(6)
    r = env.reset()
    f32 = torch.zeros((B, 4, G, G), dtype=torch.float32, device=env.device)
    n_rows = n_flight = 0
    for k in range(40):
        r = env.step(r["agent_id"].clone(), torch.rand((B, 3), generator=g, dtype=torch.float64))
        ids = r["agent_id"].clone()
        rows = ids >= 0
        n_rows += int(rows.sum()); n_flight += int((r["status"] == 4).sum())
        if k % 4 != 3:
            continue
        fresh = env.render_state(ids)
        assert fresh.dtype == torch.bfloat16
        env._h.set_obs_format(_lib.OBS_F32)
        env._h.render(ids.data_ptr(), f32.data_ptr())
        env._h.set_obs_format(_lib.OBS_BF16)
        _assert_rounded(torch, r["state"][rows], f32[rows], "time slices launch %d (state)" % k)
        _assert_rounded(torch, fresh[rows], f32[rows], "time slices launch %d (render_state)" % k)
    assert _canary_ok(raw, env.state.numel()) and n_rows > B and n_flight > 0
    with pytest.raises(ValueError):
        env.render_state(ids, out=f32)                         # render_state checks the dtype of `out`
    env.close()


@pytest.mark.parametrize("name", ["hanoi1000n50_m3_s1", "redundant_m2_map64", "six_m3_bs_charge_ongrid", "hanoi1000n100_m3_s5"])
def test_bf16_matches_the_reference_fixture_on_device(name):
    """10. reset_obs, obs_full[k] and the strided obs_sample[k] of the reference within 2^-8 |ref| + (1 + 2^-8) 1e-5 max(1, peak)."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    z = load_golden(name)
    sc, mc = scenario_from_golden(z)
    kw = dict(map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    env = VecWRSN([sc], mc, int(z["num_agent"]), obs_dtype="bfloat16", **kw)
    twin = VecWRSN([sc], mc, int(z["num_agent"]), **kw)
    r = env.reset(); rt = twin.reset()
    assert _ref_ok(r["state"][0], z["reset_obs"])
    _assert_rounded(torch, r["state"], rt["state"], name + " reset")
    s = int(z["obs_stride"])
    n = 0
    for k in range(len(z["in_action"])):
        ids = torch.tensor([int(z["in_agent"][k])]); act = torch.tensor(z["in_action"][k][None])
        r = env.step(ids, act); rt = twin.step(ids, act)
        if z["is_none"][k] or z["terminal"][k]:
            break
        assert int(r["agent_id"][0]) == int(z["agent_id"][k]) == int(rt["agent_id"][0])
        if int(r["agent_id"][0]) < 0 or np.isinf(z["reward"][k]):
            continue
        _assert_rounded(torch, r["state"], rt["state"], "%s decision %d" % (name, k))
        assert _ref_ok(r["state"][0][:, ::s, ::s], z["obs_sample"][k]), (name, k, "sample")
        if k < z["obs_full"].shape[0]:
            assert _ref_ok(r["state"][0], z["obs_full"][k]), (name, k, "full")
        n += 1
    assert n >= 2
    env.close(); twin.close()


def test_bf16_extent_and_untouched_rows_on_device():
    """11 / 3. canary behind exactly B*4*G*G bf16 cells; -2 rows, terminal returns and rows a masked reset leaves out stay byte-identical."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    sc = synth_scenario(21, 70, 50)
    B = 5
    env = VecWRSN([sc] * B, None, 2, obs_dtype="bfloat16")
    raw = _guard_state(torch, env)
    r = env.reset()
    i16 = lambda t: t.contiguous().view(torch.int16)
    assert bool((i16(r["state"]) != 0).flatten(1).any(1).all())
    g = torch.Generator().manual_seed(3)
    ids = r["agent_id"].clone(); ids[1] = -2
    seen_terminal = False
    for _ in range(400):
        keep = r["state"].clone()
        r = env.step(ids, torch.rand((B, 3), generator=g, dtype=torch.float64))
        untouched = (ids == -2) | (r["agent_id"] < 0)
        assert torch.equal(i16(r["state"][untouched]), i16(keep[untouched]))
        done = r["terminal"].bool()
        if bool(done.any()):
            seen_terminal = True
            break
        ids = r["agent_id"].clone(); ids[1] = -2
    assert seen_terminal and _canary_ok(raw, env.state.numel())
    keep = r["state"].clone()
    mask = torch.zeros(B, dtype=torch.uint8); mask[int(torch.nonzero(done)[0])] = 1; mask[B - 1] = 1     # incl. the row that ends at the canary
    r = env.reset(mask)
    out = ~mask.bool().to(env.device)
    assert torch.equal(i16(r["state"][out]), i16(keep[out])) and _canary_ok(raw, env.state.numel())
    assert int(r["agent_id"][B - 1]) == 0
    env.close()


def test_bf16_reuse_and_format_switch_on_device():
    """11 / 4. bf16 with map-1 reuse equals bf16 without, bit for bit; and a row rendered in one format at an address is not taken for
    map 1 of the other format at the same address (row 0 has the same address in both)."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, _lib
    B, M, G = 96, 3, 100
    scs = _batch(B, seed0=6100, uniq=48)
    a = VecWRSN(scs, None, M, auto_reset=True, step_budget=800, reuse_obs=True, obs_dtype="bfloat16")
    b = VecWRSN(scs, None, M, auto_reset=True, step_budget=800, reuse_obs=False, obs_dtype="bfloat16")
    g = torch.Generator().manual_seed(4)
    ra = a.reset(); rb = b.reset()
    i16 = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(i16(ra["state"]), i16(rb["state"]))
    n_zero = 0
    for k in range(30):
        act = torch.rand((B, 3), generator=g, dtype=torch.float64)
        now0 = ra["now"].clone()
        b.state.fill_(-3.0)
        ra = a.step(ra["agent_id"].clone(), act); rb = b.step(rb["agent_id"].clone(), act)
        rows = ra["agent_id"] >= 0
        assert torch.equal(ra["agent_id"], rb["agent_id"])
        assert torch.equal(i16(ra["state"][rows]), i16(rb["state"][rows])), k
        n_zero += int(((ra["now"] == now0) & (ra["status"] == 0) & rows).sum())
    assert n_zero > 30
    # format switch at one address, on the raw handle of `a` (reuse on)
    ids = torch.zeros(B, dtype=torch.int32, device=a.device)
    buf = torch.zeros((B, 4, G, G), dtype=torch.float32, device=a.device)
    as16 = buf.view(-1).view(torch.int16)[:B * 4 * G * G].view(B, 4, G, G)
    h = a._h
    h.set_obs_format(_lib.OBS_F32); h.render(ids.data_ptr(), buf.data_ptr())
    f32 = buf.clone()
    h.set_obs_format(_lib.OBS_BF16); h.render(ids.data_ptr(), buf.data_ptr())
    got = as16.clone()
    fresh = torch.zeros((B, 4, G, G), dtype=torch.bfloat16, device=a.device)
    h.render(ids.data_ptr(), fresh.data_ptr())
    assert torch.equal(got[0, 0], i16(fresh)[0, 0]) and torch.equal(got, i16(fresh))
    _assert_rounded(torch, fresh, f32, "format switch")
    h.render(ids.data_ptr(), buf.data_ptr())                  # bf16 at `buf`, remembered
    h.set_obs_format(_lib.OBS_F32); h.render(ids.data_ptr(), buf.data_ptr())
    assert torch.equal(buf, f32)
    buf[:, 0].fill_(-3.0); h.render(ids.data_ptr(), buf.data_ptr())      # within one format the reuse still holds
    a.synchronize()
    assert bool((buf[:, 0] == -3.0).all()) and torch.equal(buf[:, 1:], f32[:, 1:])
    h.set_obs_format(_lib.OBS_BF16)
    a.close(); b.close()


def test_bf16_transition_buffers_on_device():
    """11 / 5. TransitionBuffers of a bf16 environment (canaries behind the three state tensors) against the same run in float32: stored
    state / next_state rows are the rounded float32 rows; counts, rewards, now, env, actions, log-probabilities are equal."""
    _transition_buffers_on_device(100)


def test_bf16_transition_buffers_with_rows_that_are_not_16_byte_aligned_on_device():
    """The same at an odd map size: every second bf16 row of the buffers starts 8 bytes past a 16-byte boundary, and the roll-out copies
    go element by element."""
    _transition_buffers_on_device(7)


def _transition_buffers_on_device(G):
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import TransitionBuffers, VecWRSN, _lib, synth_scenario
    from test_ippo import _policy
    B, M, K, CAP = 6, 3, 24, 128
    scs = [synth_scenario(4300 + e, 100, 80) for e in range(B)]
    runs = []
    for dt in ("float32", "bfloat16"):
        env = VecWRSN(scs, None, M, map_size=G, auto_reset=True, step_budget=200, obs_dtype=dt)
        buf = TransitionBuffers(env, CAP, 3)
        assert buf.state.dtype == env.state.dtype == buf.pend_state.dtype == buf.next_state.dtype
        raws = {}
        if dt == "bfloat16":
            assert buf.state.element_size() == 2
            for k in ("pend_state", "state", "next_state"):
                raws[k], view = _guarded(torch, tuple(getattr(buf, k).shape), env.device)
                setattr(buf, k, view)
            buf._c = _lib.WrsnTransitionBuffers(CAP, 3, *[t.data_ptr() for t in (
                buf.pend_state, buf.pend_action, buf.pend_logp, buf.pend_valid, buf.state, buf.action, buf.next_state, buf.reward, buf.logp, buf.now,
                buf.env_index, buf.count)])
        r = env.reset()
        n_dec = np.zeros(B, dtype=int)
        for it in range(600):
            ids = r["agent_id"].cpu().numpy().copy()
            act = np.zeros((B, 3), np.float32); lp = np.zeros(B, np.float32)
            for e in range(B):
                if ids[e] >= 0 and n_dec[e] < K:
                    act[e], lp[e] = _policy(e, n_dec[e]); n_dec[e] += 1
                elif ids[e] >= 0:
                    ids[e] = -2
            tid = torch.tensor(ids, dtype=torch.int32)
            if it == 1:
                buf.record(tid, torch.from_numpy(act), torch.from_numpy(lp), states=env.state.float())   # `states=` is converted to the environment's dtype
            else:
                buf.record(tid, torch.from_numpy(act), torch.from_numpy(lp))
            r = env.step(tid, torch.from_numpy(act).double())
            buf.collect()
            env.synchronize()
            if (n_dec >= K).all() and not bool((r["status"] == 4).any()):
                break
        for k, raw in raws.items():
            assert _canary_ok(raw, getattr(buf, k).numel()), k
        runs.append((env, buf))
    (e32, b32), (e16, b16) = runs
    assert b32.counts() == b16.counts() and min(b16.counts()) > 5
    for k in ("pend_valid", "pend_action", "pend_logp"):
        assert torch.equal(getattr(b32, k), getattr(b16, k)), k
    _assert_rounded(torch, b16.pend_state, b32.pend_state, "pend_state")

    def order(buf, a, n):
        """slots of charger a sorted by (environment, time, log-probability): the blocks of a launch append in no fixed order"""
        en, nw, lg = buf.env_index[a, :n].cpu().numpy(), buf.now[a, :n].cpu().numpy(), buf.logp[a, :n].cpu().numpy()
        return torch.as_tensor(np.lexsort((lg, nw, en)), device=buf.state.device)
    for a in range(M):
        n = b16.counts()[a]
        q32, q16 = order(b32, a, n), order(b16, a, n)
        for k in ("reward", "logp", "now", "env_index", "action"):
            assert torch.equal(getattr(b32, k)[a].index_select(0, q32), getattr(b16, k)[a].index_select(0, q16)), (a, k)
        for k in ("state", "next_state"):
            _assert_rounded(torch, getattr(b16, k)[a].index_select(0, q16), getattr(b32, k)[a].index_select(0, q32), "%s of charger %d" % (k, a))
        assert bool((b16.state[a, :n].view(torch.int16) != 0).flatten(1).any(1).all()) and not bool(b16.state[a, n:].view(torch.int16).any())
    e32.close(); e16.close()


def test_bf16_records_on_device():
    """11 / 6. save + load and clone on bf16 batches: every restored row's `state` equals a full render of it, also over the steps after."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    B, M = 64, 3
    scs = [synth_scenario(7700 + e, 200, 200) for e in range(B)]
    a = VecWRSN(scs, None, M, auto_reset=True, reuse_obs=True, obs_dtype="bfloat16")
    b = VecWRSN(scs[::-1], None, M, auto_reset=True, reuse_obs=True, obs_dtype="bfloat16")
    c = VecWRSN(scs, None, M, auto_reset=True)                # float32 twin of `a`: records carry no format
    raw_a = _guard_state(torch, a)
    g = torch.Generator().manual_seed(4)
    r = a.reset(); rb = b.reset(); c.reset()
    for k in range(6):
        act = torch.rand((B, 3), generator=g, dtype=torch.float64)
        r = a.step(r["agent_id"].clone(), act)
        rb = b.step(rb["agent_id"].clone(), torch.rand((B, 3), generator=g, dtype=torch.float64))
    i16 = lambda t: t.contiguous().view(torch.int16)

    def check(env):
        aid = env.agent_id.clone()
        full = env.render_state(aid)
        m = aid >= 0
        assert int(m.sum()) > 0 and torch.equal(i16(env.state[m]), i16(full[m]))
    rec = a.save_envs(np.arange(0, B, 2))
    b.load_envs(rec, np.arange(1, B, 2))
    check(b)
    src = torch.arange(0, B, 2, device=a.device); dst = torch.arange(1, B, 2, device=a.device)
    m = a.agent_id[src] >= 0
    assert torch.equal(i16(b.state[dst][m]), i16(a.state[src][m]))            # the destination's rendered row equals the source's
    c.load_envs(rec, np.arange(0, B, 2))                       # a record saved by a bf16 batch loads into a float32 one
    _assert_rounded(torch, a.state[src][m], c.state[src][m], "record into a float32 batch")
    a.clone_envs(np.arange(0, B // 2), np.arange(B // 2, B))
    check(a)
    m = (a.agent_id[:B // 2] >= 0)
    assert torch.equal(i16(a.state[B // 2:][m]), i16(a.state[:B // 2][m]))
    for k in range(4):
        act = torch.rand((B, 3), generator=g, dtype=torch.float64)
        a.step(a.agent_id.clone(), act); b.step(b.agent_id.clone(), act)
        check(a); check(b)
    assert _canary_ok(raw_a, a.state.numel())
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("inference_dtype", ["bf16", None])
def test_batched_ippo_on_bf16_observations(inference_dtype):
    """12. BatchedIPPO over a bf16 environment: the stored states are what the policy saw -- the stored log-probabilities are reproduced
    by rollout_logp on the stored bf16 states (tolerance of the float32 test of that property) -- then one roll_out + one update per
    charger with finite losses."""
    torch = need_gpu()
    from multi_agent_rl_wrsn_amd import BatchedIPPO, VecWRSN, synth_scenario
    torch.manual_seed(0); np.random.seed(0)
    B, M, G = 256, 3, 100
    env = VecWRSN([synth_scenario(9100 + e % 64, 200, 200) for e in range(B)], None, M, auto_reset=True, step_budget=1500, reuse_obs=True,
                  obs_dtype="bfloat16")
    algo = BatchedIPPO(dict(batch_size=64, minibatch_size=32, n_updates_per_iteration=1), env, capacity=128, infer_chunk=256, min_bucket=64,
                       inference_dtype=inference_dtype)
    assert algo.buffers.state.element_size() == 2 and algo.buffers.next_state.dtype == torch.bfloat16 == algo.buffers.pend_state.dtype
    # first launch by hand: every environment asks for charger 0 after the reset
    algo.buffers.clear(); algo._req = env.reset()
    ids = algo._req["agent_id"].clone()
    seen = algo._req["state"].clone()
    algo.step_batch()
    rows = torch.nonzero(ids == 0).flatten()
    assert rows.numel() == B
    stored = algo.buffers.pend_state[rows, 0]
    assert stored.dtype == torch.bfloat16 and torch.equal(stored.view(torch.int16), seen.view(torch.int16))
    acts = algo.buffers.pend_action[rows, 0].view(-1, G, G)
    again = algo.rollout_logp(0, stored, acts)
    lp = algo.buffers.pend_logp[rows, 0]
    assert torch.allclose(again, lp, rtol=1e-5, atol=0.05), float((again - lp).abs().max())
    batches = algo.roll_out(max_launches=80)
    assert min(algo.buffers.counts()) >= 64
    for a in range(M):
        b = batches[a]
        assert b["states"].dtype == torch.bfloat16 and b["states"].shape == (64, 4, G, G) and b["next_states"].dtype == torch.bfloat16
        before = [p.detach().clone() for p in algo.actors[a].parameters()]
        stats = algo.update(a, b)
        assert all(np.isfinite(v) for v in stats) and all(np.isfinite(v) for v in algo.loggers[a]["losses"])
        assert any(not torch.equal(p0, p1) for p0, p1 in zip(before, algo.actors[a].parameters()))
    env.close()
