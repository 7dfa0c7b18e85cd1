"""Policy-shaped action streams (tests/action_streams.py) against the oracle: one body, run here on the emulator (the unmodified HIP
sources on tests/emu) and by tests/test_action_streams_gpu.py on the device.

Every request goes through parity.RequestCheck (status, level, energy, consumption rate, charger energy, exclusive reward, reward,
observation, provenance of prev_minfit).  On top of it the body asserts
  * Node.energyRR (PEEK_NODE_RR against the oracle's `rr`) at every request, bit for bit on every node two chargers never held
    together, within RR_SHARED_ULPS ulp of the largest rate seen on the node where they did (derivation at RR_SHARED_ULPS);
  * status >= 0 on every row of every launch; a negative row fails with the step, the error code (PEEK_MC slot 14) and the number of
    non-zero energyRR entries;
  * that the stream did what it is for (zero-time requests, chargers sharing a node, exact stays).
The emulator steps single networks with the residue hatch off (the seeds below were kept because the oracle's own run needs none); the
device steps four networks per handle and allows the sweep's share of residue-dependent rewards, max(2, n_cmp // 200), and no other.

The second half is the capacity of the charging-rate list: more nodes with a non-zero energyRR than the list in LDS ever held must
change nothing."""
import collections

import numpy as np
import pytest

import action_streams
from parity import RequestCheck
from sides import EmuSide

# stream -> (N, M, requests per environment, seed of network 0 and of its stream); networks synth_scenario(seed + 10 e, N, N), stream e
# seeded seed + 10 e.  Per side: networks per handle, residue hatch, cap of residue-dependent rewards.
CASES = {"converge": (200, 5, 120, 31000), "same_spot": (65, 3, 50, 31100), "same_spot_on_node": (64, 2, 80, 31200),
         "zero_charge": (65, 3, 80, 31300), "stay": (64, 2, 80, 31400), "clip_edges": (65, 3, 40, 31500), "repeat": (64, 3, 60, 31600)}
MIXED = {"blocking": dict(), "budget": dict(step_budget=60), "time_sliced": dict(step_deadline_us=20)}
MIXED_CASE = (200, 3, 90, 31700)
STREAM_RUN = {"emu": (1, False, lambda n_cmp: 0), "gpu": (4, True, lambda n_cmp: max(2, n_cmp // 200))}
# Node.energyRR is equal to the oracle's bit for bit on every node that two chargers never held together.  On a node they shared the
# device may differ by RR_SHARED_ULPS ulp of the largest rate seen on that node (either side, any request so far) per request at which
# the node was seen shared -- not per request of the run.  This is not a tolerance on the arithmetic: the device keeps a
# charger's connection standing through the whole seconds of a stay where the reference disconnects and reconnects every second
# (MobileCharger.py:40-48).  With another rate v on the node the reference's pair is v <- fl(fl(v - r) + r): two roundings of at most half
# an ulp of the largest value the node holds, the first time; after it v is a fixed point of the pair.  So a shared stay leaves at most
# 1 ulp of the SUM of the rates, for good (a residue).  The sum itself is not seen at a request -- a charger has disconnected when it
# asks (MobileCharger.py:47-48) --, only its parts are: two rates sum to at most one binade above the larger, hence 2 ulp of what is seen.
# A node is seen shared at a request when the discs of two chargers at action type `charging` cover it; every stay ends in a request,
# so no overlap of two stays goes unseen.
RR_SHARED_ULPS = 2
ZERO_TIME = ("zero_charge", "stay", "mixed")                 # streams that must produce requests at the instant of the one before
SHARING = ("converge", "same_spot", "same_spot_on_node", "mixed")   # ... instants at which two charging chargers share a node


def cover_count(m, node_xy, mc):
    """Per node: the chargers at action type `charging` with connected nodes -- the one whose stay just ended and the ones in the
    middle of theirs -- whose charging range holds it (MobileCharger.py:55-58), from the oracle's charger positions."""
    out = np.zeros(len(node_xy), dtype=int)
    for k in range(len(m["loc_x"])):
        if m["type_charging"][k] == 1 and m["n_conn"][k] > 0:
            d = np.sqrt(((node_xy - np.array([m["loc_x"][k], m["loc_y"][k]])) ** 2).sum(1))
            out += d <= mc["charging_range"]
    return out


def error_code(side, e):
    """WrsnEnvDyn.error of environment e (0: none; wrsn_types.h lists the codes)."""
    return int(side.handle.peek(5)[e, 0, 14])


def old_list_capacity(side, M):
    """M * CC + 32, what the charging-rate list held before it was sized by the node count: CC is the handle's bound of a charger's
    connected nodes (WrsnRecHeader.conn_bound, _lib.REC_CONN_BOUND_OFFSET) rounded up to a multiple of 4, at least 4."""
    from multi_agent_rl_wrsn_amd import _lib
    rec = side.save_envs([0])
    rec = rec.cpu().numpy() if hasattr(rec, "cpu") else rec
    cb = int(rec[0, _lib.REC_CONN_BOUND_OFFSET:_lib.REC_CONN_BOUND_OFFSET + 4].view(np.int32)[0])
    return M * max(4, (cb + 3) // 4 * 4) + 32


def check_status(side, v, step, old_cap):
    st = np.asarray(v["status"])
    if (st < 0).any():
        e = int(np.nonzero(st < 0)[0][0])
        nnz = int((v["nodes"]["rr"][e] != 0).sum())
        raise AssertionError("row %d reports status %d at launch %d: error code %d, %d nodes with a non-zero energyRR (the list in LDS "
                             "once held M * CC + 32 = %d)" % (e, int(st[e]), step, error_code(side, e), nnz, old_cap))


def run_stream(side, scs, mc, M, streams, K, hatch, prepare=None):
    """`side` over `scs` and one oracle per environment; stream e gives the action of every request of environment e.  `prepare(side,
    oracles)` changes both sides alike after the reset.  Returns the RequestCheck and a dict of what was seen."""
    from wrsn_oracle import OracleWRSN
    B = len(scs)
    ors = [OracleWRSN(s.node_xy, s.target_xy, s.bs_xy, s.node_spec, mc, s.max_time, M) for s in scs]
    chk = RequestCheck(scs, hatch=hatch)
    side.reset()
    last = [o.reset() for o in ors]
    if prepare is not None:
        prepare(side, ors)
    v = side.view(); chk.remember(range(B), v, reset=True)
    frames = []
    for e, o in enumerate(ors):
        oi = o.env_info(); frames.append((oi["xmin"], oi["xmax"], oi["ymin"], oi["ymax"]))
        gi = v["env_info"]
        assert frames[e] == (gi["xmin"][e], gi["xmax"][e], gi["ymin"][e], gi["ymax"][e]), ("frame", e)
        assert int(v["agent_id"][e]) == (-1 if last[e]["agent_id"] is None else last[e]["agent_id"]), ("reset", e)
    rr_max = [np.zeros(s.n_node) for s in scs]; shared = [np.zeros(s.n_node, dtype=int) for s in scs]
    old_cap = old_list_capacity(side, M)
    seen = dict(rr_exact=0, rr_worst_ulps=0.0, zero_time=0, sharing=0, rr_cmp=0, rr_nonzero=0, rr_shared=0, finished=0, max_rr_entries=0, min_rr_entries=10 ** 9)
    done = np.zeros(B, dtype=bool); busy = np.zeros(B, dtype=bool); pending = [None] * B
    n_fresh = np.zeros(B, dtype=int); act = np.zeros((B, 3))
    rng_cr = float(mc["charging_range"])
    for step in range(4000 * K):
        ids = np.full(B, -1, dtype=np.int64)
        for e in range(B):
            if done[e]: ids[e] = -2
            elif not busy[e]:
                a = last[e]["agent_id"]
                ids[e] = -1 if a is None else a
                if a is not None:
                    on, om = ors[e].nodes(), ors[e].mcs()
                    req = action_streams.Request(a, on, om, frames[e], scs[e].node_xy, int(n_fresh[e]))
                    act[e] = streams[e](req)
                    sh = action_streams.shared_nodes(req, on["status"], rng_cr)
                    seen["sharing"] += int(len(sh) > 0)
                    seen["rr_shared"] += int(len(sh) > 0 and (on["rr"][sh] != 0).any())
                pending[e] = (a, act[e].copy()); chk.submit(e, a)
        side.step(ids, act)
        v = side.view()
        check_status(side, v, step, old_cap)
        for e in range(B):
            if done[e]: continue
            busy[e] = v["status"][e] == 4
            if busy[e]:
                chk.n_flight += 1
                continue
            t_prev = last[e]["now"]
            last[e] = ors[e].step(*pending[e])
            chk.fresh(step, e, last[e], ors[e], v); n_fresh[e] += 1
            seen["zero_time"] += int(last[e]["now"] == t_prev and pending[e][0] is not None)
            if not last[e]["terminal"]:
                n = scs[e].n_node
                grr, orr = v["nodes"]["rr"][e][:n], ors[e].nodes()["rr"]
                seen["rr_cmp"] += 1; seen["rr_nonzero"] += int((orr != 0).any())
                seen["max_rr_entries"] = max(seen["max_rr_entries"], int((orr != 0).sum()))
                seen["min_rr_entries"] = min(seen["min_rr_entries"], int((orr != 0).sum()))
                rr_max[e] = np.maximum(rr_max[e], np.maximum(np.abs(grr), np.abs(orr)))
                shared[e] += cover_count(ors[e].mcs(), scs[e].node_xy, mc) >= 2
                tol = RR_SHARED_ULPS * np.spacing(rr_max[e]) * shared[e]
                diff = np.abs(grr - orr)
                seen["rr_exact"] += int(np.array_equal(grr, orr))
                with np.errstate(invalid="ignore", divide="ignore"):
                    seen["rr_worst_ulps"] = max(seen["rr_worst_ulps"], float(np.nanmax(np.where(diff > 0, diff / np.spacing(rr_max[e]), 0.0))))
                if (diff > tol).any():
                    bad = np.nonzero(diff > tol)[0]
                    raise AssertionError(("energyRR", step, e, [(int(i), float(grr[i]), float(orr[i]), float(tol[i])) for i in bad[:6]], len(bad)))
            if last[e]["terminal"] or n_fresh[e] >= K:
                done[e] = True; seen["finished"] += int(last[e]["terminal"])
        if done.all(): break
    assert done.all(), "a step stayed in flight for 4000 calls"
    return chk, seen


def stream_matches_oracle(Side, name, mode="blocking"):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    n_env, hatch, noise_cap = STREAM_RUN[Side.name]
    N, M, K, seed = MIXED_CASE if name == "mixed" else CASES[name]
    scs = [synth_scenario(seed + 10 * e, N, N) for e in range(n_env)]
    streams = [action_streams.make(name, seed + 10 * e) for e in range(n_env)]
    side = Side(scs, DEFAULT_MC_SPEC, M, **(MIXED[mode] if name == "mixed" else {}))
    chk, seen = run_stream(side, scs, DEFAULT_MC_SPEC, M, streams, K, hatch)
    side.close()
    print("%s/%s on %s: %d requests compared (%d residue-dependent, %d calls in flight), energyRR compared at %d (%d with a rate, most "
          "entries %d), %d zero-time requests, %d instants with a shared node (%d with its rate standing), %d exact stays, %d episodes "
          "finished; energyRR bit-equal at %d, worst %.1f ulp of the node's largest rate" % (name, mode, Side.name, chk.n_cmp, chk.n_noise, chk.n_flight, seen["rr_cmp"], seen["rr_nonzero"],
                        seen["max_rr_entries"], seen["zero_time"], seen["sharing"], seen["rr_shared"], sum(s.exact_stays for s in streams),
                        seen["finished"], seen["rr_exact"], seen["rr_worst_ulps"]))
    assert chk.n_cmp >= n_env * 10 and chk.n_noise <= noise_cap(chk.n_cmp), (chk.n_cmp, chk.n_noise)   # K requests or the whole episode
    assert seen["rr_cmp"] >= chk.n_cmp // 2
    if name in ZERO_TIME:                                    # (`mixed` spends one request in seven on each of the two)
        assert seen["zero_time"] >= (1 if name == "mixed" else 5), seen
    if name in SHARING:
        assert seen["sharing"] >= 1, seen
    if name == "stay":
        assert sum(s.exact_stays for s in streams) >= 5
    if name == "mixed":
        used = sum((s.used for s in streams), collections.Counter())
        assert all(used[k] > 0 for k in action_streams.NAMES[:-1]), used
        assert (chk.n_flight > 0) == (mode != "blocking"), (mode, chk.n_flight)


# ---- the body above on the emulator (tests/test_action_streams_gpu.py: on the device)
@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_stream_matches_oracle(name, hip_lib):
    stream_matches_oracle(EmuSide, name)


@pytest.mark.parametrize("mode", sorted(MIXED))
def test_emulated_mixed_stream_matches_oracle(mode, hip_lib):
    stream_matches_oracle(EmuSide, "mixed", mode)


# ---- the capacity of the charging-rate list
# (N, M, entries beyond M * CC + 32, requests): both sides of the 64-node slot, the headline size, and the sizes above 512 nodes, where
# the list in LDS is not one entry per node and the rest lives in the energyRR row in HBM
CAPACITY = [(64, 2, 1, 40), (65, 3, 9, 40), (200, 3, 1, 60), (600, 5, 1, 30), (1000, 8, 0, 30), (1000, 8, 1, 30), (1000, 8, 40, 30)]
CAP_SKIP = 3                                                 # the node the chargers are sent to and its two nearest carry nothing: new entries
CAP_SEED = 32000
RESIDUES = (4.44e-16, -4.44e-16, 2.22e-16, -8.88e-16, 1.33e-15, -1.11e-16)   # what (ra + rb) - ra - rb leaves of rates of 0.5 .. 5


def _record_rr_offset(rec, energy, cs, NP):
    """Byte offset of the live energyRR row in a record: the rows of the live node arrays follow each other (E, CS, RR, each NP float64);
    E and CS are found by their content."""
    raw = rec.tobytes()
    oe = raw.find(np.ascontiguousarray(energy).tobytes()); oc = raw.find(np.ascontiguousarray(cs).tobytes(), oe + 1)
    assert oe >= 256 and oc == oe + 8 * NP, (oe, oc, NP)
    return oc + 8 * NP


def list_capacity_matches_oracle(Side, N, M, over, K):
    """As many long-lived entries as the list once held (over = 0: the next connection is the one that did not fit) or more (they did
    not fit when the state was loaded), in every environment: residue-sized rates on the nodes around the one the `converge` stream
    sends every charger to, written into a saved record (and into the oracle) and loaded.  Nothing may be dropped:
    no negative row, energyRR as in the streams (bit for bit but on shared nodes), everything else through RequestCheck.  (Rates of a real size are not written: without a
    connected charger the device skips the charging term of a second, which only residues survive unnoticed -- DESIGN.md 5.)"""
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    from sides import aligned
    n_env, hatch, noise_cap = STREAM_RUN[Side.name]
    scs = [synth_scenario(CAP_SEED + N + 10 * e, N, N) for e in range(n_env)]
    streams = [action_streams.make("converge", CAP_SEED + N + 10 * e) for e in range(n_env)]
    side = Side(scs, DEFAULT_MC_SPEC, M)
    want = []

    def prepare(side, ors):
        n_entries = old_list_capacity(side, M) + over
        assert 32 < n_entries <= N - CAP_SKIP, (n_entries, N)
        rec = side.save_envs()
        host = rec.cpu().numpy().copy() if hasattr(rec, "cpu") else rec.copy()
        nd = side.nodes()
        NP = 64 * [k for k in (1, 2, 4, 8, 16) if 64 * k >= side.N][0]
        for e, o in enumerate(ors):
            on = o.nodes()
            assert (on["status"] == 1).all() and not on["rr"].any()
            w = int(np.argmin(on["energy"]))
            near = np.argsort(((scs[e].node_xy - scs[e].node_xy[w]) ** 2).sum(1), kind="stable")[CAP_SKIP:CAP_SKIP + n_entries]
            rr = np.zeros(N); rr[near] = [RESIDUES[k % len(RESIDUES)] for k in range(n_entries)]
            o.set_node_rr(rr)
            row = np.zeros(NP); row[:N] = rr
            pad = np.zeros(NP); pad[:side.N] = nd["energy"][e]; pc = np.zeros(NP); pc[:side.N] = nd["cs"][e]
            off = _record_rr_offset(host[e], pad[:N], pc[:N], NP)
            host[e, off:off + 8 * NP] = row.view(np.uint8)
            want.append(n_entries)
        if hasattr(rec, "cpu"):
            import torch
            side.load_envs(torch.from_numpy(host))
        else:
            al = aligned(host.shape); al[:] = host
            side.load_envs(al)
        for e, o in enumerate(ors):
            assert np.array_equal(side.nodes()["rr"][e][:N], o.nodes()["rr"]), ("loaded energyRR", e)

    chk, seen = run_stream(side, scs, DEFAULT_MC_SPEC, M, streams, K, hatch, prepare=prepare)
    side.close()
    print("capacity N=%d M=%d on %s: %d entries written (M * CC + 32 + %d), %d..%d non-zero energyRR at the %d requests compared, %d instants "
          "with a shared node" % (N, M, Side.name, want[0], over, seen["min_rr_entries"], seen["max_rr_entries"], chk.n_cmp, seen["sharing"]))
    assert chk.n_cmp >= 10 * n_env and chk.n_noise <= noise_cap(chk.n_cmp)
    assert seen["min_rr_entries"] > 32 and seen["max_rr_entries"] > want[0]     # they stay, and the chargers add entries of their own
    assert seen["rr_nonzero"] == seen["rr_cmp"]


@pytest.mark.parametrize("N,M,over,K", CAPACITY)
def test_emulated_list_capacity_matches_oracle(N, M, over, K, hip_lib):
    list_capacity_matches_oracle(EmuSide, N, M, over, K)
