"""Shared comparison helpers: golden fixture / oracle versus an implementation under test.

Tolerances (BASELINE.json north_star: node-energy and reward trajectories within 1e-5 relative):
  * agent id, terminal flag, node status, charger status / action type: exact;
  * simulated time: 1e-9 relative (float64 on both sides);
  * node energy, consumption rate, charger energy / position, reward: RTOL = 1e-5 (+ tiny absolute floors);
  * observation (float32 on the device): 1e-5 of the map's peak value, absolute.
"""
import numpy as np

RTOL = 1e-5


def close(a, b, rtol=RTOL, atol=0.0):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    both_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    ok = np.abs(a - b) <= atol + rtol * np.abs(b)
    return bool(np.all(ok | both_nan | both_inf))


_TOPO = {}


def _topology(z):
    import fitness_ref
    key = (z["node_xy"].tobytes(), z["target_xy"].tobytes())
    if key not in _TOPO:
        _TOPO[key] = fitness_ref.Topology(z["node_xy"], z["target_xy"], z["bs_xy"], float(z["node_spec"][2]), float(z["node_spec"][3]))
    return _TOPO[key]


def _reward_depends_on_residue(z, k, got, tag):
    """The fixture's reward and the implementation's differ.  Accept it only when the reference's own arithmetic is
    ill-conditioned there -- an alive node carries a rounding-residue energyCS (fitness_ref docstring) -- AND the node
    state matches the fixture AND the implementation's fitness and reward are exactly what the reference's algorithm
    (WRSN.py:188-227) gives on the implementation's own node state."""
    import fitness_ref
    if "node_cs" not in got or "min_fitness" not in got:
        return False
    noisy = fitness_ref.residue_nodes(z["node_cs"][k], z["node_status"][k]) | fitness_ref.residue_nodes(got["node_cs"], got["node_status"])
    if not noisy.any():
        return False
    thr = float(z["node_spec"][1])
    fit = fitness_ref.network_fitness(_topology(z), got["node_energy"], got["node_cs"], got["node_status"], thr)
    assert close(got["min_fitness"], fit.min(), rtol=1e-9), (tag, "fitness on own state", got["min_fitness"], fit.min())
    a = got["agent_id"]
    mtm, ctm, avg = float(z["consts"][0]), float(z["consts"][1]), float(z["consts"][2])
    want = fitness_ref.reward(fit.min(), got["prev_minfit"][a], got["excl"][a], avg, ctm, mtm)
    scale = (0.8 * abs(fit.min() - got["prev_minfit"][a]) + 0.2 * abs(got["excl"][a]) / avg) / (ctm + mtm)
    assert abs(got["reward"] - want) <= 1e-5 * max(abs(want), scale) + 1e-12, (tag, "reward on own state", got["reward"], want)
    return True


def check_decision(z, k, got, where="", noise=None):
    """`got`: dict with agent_id, now, reward, terminal and (optional) node/mc arrays + obs for decision k.
    `noise`: list that collects the decisions whose reward hangs on the sign of a rounding-residue energyCS (see
    _reward_depends_on_residue); without it such a decision fails like any other mismatch."""
    tag = "%s decision %d" % (where, k)
    exp_id = int(z["agent_id"][k])
    assert got["agent_id"] == exp_id, (tag, "agent", got["agent_id"], exp_id)
    assert bool(got["terminal"]) == bool(z["terminal"][k]), (tag, "terminal")
    assert close(got["now"], z["now"][k], rtol=1e-9), (tag, "now", got["now"], float(z["now"][k]))
    terminal = bool(z["terminal"][k])
    if "targets_active" in got:                             # Network.targets_active: what the last setLevels reached (also at the terminal return)
        nt = len(z["targets_active"][k])
        assert np.array_equal(np.asarray(got["targets_active"]).astype(int)[:nt], z["targets_active"][k]), (tag, "targets_active")
    reward_ok = True
    if exp_id >= 0:
        r = float(z["reward"][k])
        reward_ok = close(got["reward"], r, atol=1e-9)
    if "node_energy" in got and not terminal:
        # after the network is declared dead the product freezes node state (documented deviation)
        assert np.array_equal(got["node_status"], z["node_status"][k]), (tag, "node status")
        assert close(got["node_energy"], z["node_energy"][k]), (tag, "node energy", np.max(np.abs(got["node_energy"] - z["node_energy"][k]) / z["node_energy"][k]))
        assert close(got["node_cs"], z["node_cs"][k], atol=1e-9), (tag, "node cs")
    if "mc_energy" in got and not terminal:
        assert close(got["mc_energy"], z["mc_energy"][k], atol=1e-6), (tag, "mc energy")
        assert close(got["mc_loc"], z["mc_loc"][k], atol=1e-6), (tag, "mc loc")
        assert np.array_equal(np.asarray(got["mc_status"]).astype(int), z["mc_status"][k]), (tag, "mc status")
        assert np.array_equal(np.asarray(got["mc_charging"]).astype(int), z["mc_charging"][k]), (tag, "mc action type")
        assert np.array_equal(np.asarray(got["mc_nconn"]).astype(int), z["mc_nconn"][k]), (tag, "connected nodes")
        assert close(got["excl"], z["excl"][k], atol=1e-7), (tag, "exclusive reward", got["excl"], z["excl"][k])
    if not reward_ok:
        if noise is not None and not terminal and _reward_depends_on_residue(z, k, got, tag):
            noise.append((where, k))
        else:
            raise AssertionError((tag, "reward", got["reward"], float(z["reward"][k])))
    if got.get("obs") is not None and exp_id >= 0 and not terminal:
        s = int(z["obs_stride"])
        ref = z["obs_sample"][k]
        sample = np.asarray(got["obs"], dtype=np.float64)[:, ::s, ::s]
        scale = max(1.0, float(np.nanmax(np.abs(ref))))
        assert np.max(np.abs(sample - ref)) <= 1e-5 * scale, (tag, "obs sample", np.max(np.abs(sample - ref)), scale)
        if k < z["obs_full"].shape[0]:
            full = z["obs_full"][k]
            assert np.max(np.abs(np.asarray(got["obs"], dtype=np.float64) - full)) <= 1e-5 * max(1.0, float(np.abs(full).max())), (tag, "obs full")


class RequestCheck:
    """One batch stepped side by side with one OracleWRSN per environment: the comparison of every fresh request, on plain
    numpy values, so that the emulator and the GPU (sides.EmuSide / sides.VecSide) feed the same code.  Per environment it keeps
      * `tainted`: an alive node carried a rounding-residue energyCS at some decision of this episode -- the fitness of THAT instant may
        have gone into agents_prev_fitness (WRSN.py:304) and comes back in the reward of a later decision, when the residue is gone;
      * the device's own min_fitness at its last fresh return / reset, and the agent the call in flight gave an action to: WRSN.py:304
        stores the fitness of exactly that state (no simulated time passes between a return and the next call), so at the fresh return
        of that call prev_minfit[agent] must be the remembered number, bit for bit -- the device copies it (wrsn_sim.h: `prev_minfit =
        last_minfit`), it does not compute it a second time -- in blocking, budgeted, pipelined and time-sliced launches alike.
    `hatch=False`: a reward that differs fails, whatever the residues (tests whose seeds need no hatch)."""

    def __init__(self, scs, hatch=True):
        B = len(scs)
        self.scs = scs; self.hatch = hatch
        self.tainted = np.zeros(B, dtype=bool); self.minfit = np.full(B, np.nan); self.given = np.full(B, -1, dtype=np.int64)
        self.n_cmp = self.n_noise = self.n_prov = self.n_flight = 0; self.worst_rew = self.worst_obs = 0.0
        self._topo = {}

    def remember(self, envs, view, reset=False):
        """after a reset of `envs` (reset=True: a new episode) or a fresh return: the fitness the next action's prev_minfit must be"""
        for e in envs:
            self.minfit[e] = view["env_info"]["min_fitness"][e]; self.given[e] = -1
            if reset: self.tainted[e] = False

    def submit(self, e, agent):
        """the call about to be made gives environment e (not in flight) an action for `agent` (None / -1: just run)"""
        self.given[e] = -1 if agent is None else int(agent)

    def _fitness_topology(self, e):
        import fitness_ref
        if e not in self._topo:
            s = self.scs[e]
            self._topo[e] = fitness_ref.Topology(s.node_xy, s.target_xy, s.bs_xy, float(s.node_spec["com_range"]), float(s.node_spec["sen_range"]))
        return self._topo[e]

    def fresh(self, step, e, x, oracle, view):
        """environment e returned a request (status != 4): `x` is the oracle's return of the same WRSN.step, `view` the device's arrays
        (a side's view()).  Raises AssertionError on a mismatch; returns False when the reward hangs on a rounding residue (counted)."""
        n = self.scs[e].n_node
        ag, now, rew, term = view["agent_id"], view["now"], view["reward"], view["terminal"]
        nd, gm, gi = view["nodes"], view["mcs"], view["env_info"]
        self.n_cmp += 1
        assert int(ag[e]) == (-1 if x["agent_id"] is None else x["agent_id"]), ("agent", step, e, int(ag[e]), x["agent_id"])
        assert bool(term[e]) == x["terminal"] and close(float(now[e]), x["now"], rtol=1e-9), ("time/terminal", step, e, now[e], x["now"])
        given = int(self.given[e])
        if given >= 0:                                          # provenance of prev_minfit (WRSN.py:304), terminal return included
            got_prev = gm["prev_minfit"][e][given]
            assert got_prev == self.minfit[e] or (np.isnan(got_prev) and np.isnan(self.minfit[e])), \
                ("prev_minfit is not the fitness reported when the action was given", step, e, given, got_prev, self.minfit[e])
            self.n_prov += 1
        self.remember([e], view)
        if x["terminal"]:
            return True
        on = oracle.nodes(); om = oracle.mcs(); oi = oracle.env_info()
        gst, gen, gcs = nd["status"][e][:n], nd["energy"][e][:n], nd["cs"][e][:n]
        assert np.array_equal(gst, on["status"]), ("status", step, e)
        assert np.array_equal(nd["level"][e][:n], on["level"]), ("level", step, e)
        assert close(gen, on["energy"]), ("energy", step, e)
        assert close(gcs, on["cs"], atol=1e-9), ("cs", step, e)
        ocs = on["cs"]; alive_ = gst == 1
        scale = max(np.abs(gcs).max(), 1e-30)
        noisy = alive_ & (((np.abs(gcs) < 1e-9 * scale) & (gcs != 0)) | ((np.abs(ocs) < 1e-9 * scale) & (ocs != 0)))
        self.tainted[e] |= bool(noisy.any())
        # charger state: excl does not depend on the residue (a sum of energy differences), so neither check is excused in a tainted episode
        assert close(gm["excl"][e], om["excl"], atol=1e-7), ("excl", step, e, gm["excl"][e], om["excl"])
        assert close(gm["energy"][e], om["energy"], atol=1e-6), ("charger energy", step, e, gm["energy"][e], om["energy"])
        if given >= 0 and not self.tainted[e]:
            assert close(gm["prev_minfit"][e][given], om["prev_minfit"][given]), ("prev_minfit", step, e, given, gm["prev_minfit"][e][given], om["prev_minfit"][given])
        if x["agent_id"] is None:
            return True
        a_ = x["agent_id"]
        d = abs(float(rew[e]) - x["reward"]); self.worst_rew = max(self.worst_rew, d / max(1e-9, abs(x["reward"])) if abs(x["reward"]) > 1e-6 else 0.0)
        # get_reward (WRSN.py:222-227) = (0.8 (fit - prev) + 0.2 excl / avg) / (ctm + mtm): the two terms can nearly cancel, so
        # the 1e-5 is taken relative to their magnitudes, not to the (possibly tiny) difference
        scale_ = (0.8 * abs(oi["min_fitness"] - om["prev_minfit"][a_]) + 0.2 * abs(om["excl"][a_]) / oi["avg_nodes_agent"]) / (oi["charging_time_max"] + oi["moving_time_max"])
        if abs(float(rew[e]) - x["reward"]) > 1e-5 * max(abs(x["reward"]), scale_) + 1e-12:
            # The reference divides by energyCS in get_network_fitness (WRSN.py:196-209).  Once a node has been idle for
            # 10 s its energyCS is the rounding residue of the sliding mean (Node.py:71-77), +-1e-16 instead of 0, and
            # (E - thr) / energyCS is +-1e19 with the sign of that residue: a negative one turns the node into a
            # bottleneck.  The residue depends on the last bit of every packet cost (SciPy/BLAS distances included), so
            # no two implementations -- or BLAS builds -- agree on it.  Such requests are counted, not failed.
            if self.hatch and (noisy.any() or self.tainted[e]):
                # the escape hatch is pinned: node state (status, energies) matched above, and the device's fitness / reward must be
                # exactly what the reference's algorithm (tests/fitness_ref.py: WRSN.py:188-227) gives on the device's OWN node state
                # -- with a prev_minfit whose provenance was checked above
                import fitness_ref
                fit = fitness_ref.network_fitness(self._fitness_topology(e), gen, gcs, gst, float(self.scs[e].node_spec["threshold"]))
                assert close(gi["min_fitness"][e], fit.min(), rtol=1e-9), ("fitness on own state", step, e, gi["min_fitness"][e], fit.min())
                want = fitness_ref.reward(fit.min(), gm["prev_minfit"][e][a_], gm["excl"][e][a_], gi["avg_nodes_agent"][e], gi["charging_time_max"][e], gi["moving_time_max"][e])
                sc_ = (0.8 * abs(fit.min() - gm["prev_minfit"][e][a_]) + 0.2 * abs(gm["excl"][e][a_]) / gi["avg_nodes_agent"][e]) / (gi["charging_time_max"][e] + gi["moving_time_max"][e])
                assert abs(float(rew[e]) - want) <= 1e-5 * max(abs(want), sc_) + 1e-12, ("reward on own state", step, e, float(rew[e]), want)
                self.n_noise += 1
                return False
            print("REWARD MISMATCH step %s env %d agent %d: gpu %.12g oracle %.12g" % (step, e, int(ag[e]), rew[e], x["reward"]))
            print("  gpu   excl %s prev_minfit %s min_fitness %.12g" % (gm["excl"][e], gm["prev_minfit"][e], gi["min_fitness"][e]))
            print("  oracle excl %s prev_minfit %s min_fitness %.12g" % (om["excl"], om.get("prev_minfit"), oi["min_fitness"]))
            raise AssertionError("reward mismatch (see output)")
        ref = x["state"]
        if ref is not None and view.get("obs") is not None:
            o = view["obs"](e)
            err = np.max(np.abs(o - ref)) / max(1.0, np.abs(ref).max()); self.worst_obs = max(self.worst_obs, err)
            assert err <= 1e-5, ("obs", step, e, err)
        return True


def run_requests(side, scs, mc, M, K, seed, third=1.0, check_topology=False, hatch=False):
    """`side` (a sides.EmuSide / sides.VecSide over `scs`) and one oracle per environment, K decisions per environment with the actions of
    RandomState(seed) (one draw of [B, 3] per call; third component scaled by `third`: short charging times, chargers return often),
    every fresh request through RequestCheck.  An environment that is finished or has had its K requests is left alone (-2).  Works for
    blocking and budgeted handles (a row in flight keeps its action and is ignored by the call).  Returns the RequestCheck and the
    number of compared requests at which some node was dead (non-terminal deaths)."""
    from wrsn_oracle import OracleWRSN
    B = len(scs)
    ors = [OracleWRSN(s.node_xy, s.target_xy, s.bs_xy, s.node_spec, mc, s.max_time, M) for s in scs]
    chk = RequestCheck(scs, hatch=hatch)
    side.reset()
    last = [o.reset() for o in ors]
    v = side.view()
    chk.remember(range(B), v, reset=True)
    for e, o in enumerate(ors):
        assert int(v["agent_id"][e]) == (-1 if last[e]["agent_id"] is None else last[e]["agent_id"]) and close(v["now"][e], last[e]["now"], rtol=1e-9), ("reset", e)
        on = o.nodes()
        assert np.array_equal(v["nodes"]["level"][e][:o.N], on["level"]) and close(v["nodes"]["energy"][e][:o.N], on["energy"]), ("reset state", e)
    if check_topology:
        tp = side.handle.topology()
        for e, o in enumerate(ors):
            t = o.topology()
            assert np.array_equal(tp["degree"][e, :o.N], t["degree"]), ("degree", e)
            assert np.array_equal(tp["n_cover"][e, :o.N], t["n_cover"]) and np.array_equal(tp["direct"][e, :o.N], t["direct"]), ("cover/direct", e)
    rng = np.random.RandomState(seed)
    done = np.zeros(B, dtype=bool); busy = np.zeros(B, dtype=bool); pending = [None] * B
    deaths_seen = 0; n_fresh = np.zeros(B, dtype=int)
    for step in range(4000 * K):
        act = rng.rand(B, 3) * np.array([1.0, 1.0, third])
        ids = np.full(B, -1, dtype=np.int64)
        for e in range(B):
            if done[e]: ids[e] = -2
            elif not busy[e]:
                a = last[e]["agent_id"]
                ids[e] = -1 if a is None else a
                pending[e] = (a, act[e].copy()); chk.submit(e, a)
        side.step(ids, act)
        v = side.view()
        for e in range(B):
            if done[e]: continue
            busy[e] = v["status"][e] == 4
            if busy[e]:
                chk.n_flight += 1
                continue
            last[e] = ors[e].step(*pending[e])
            chk.fresh(step, e, last[e], ors[e], v); n_fresh[e] += 1
            if last[e]["terminal"] or n_fresh[e] >= K: done[e] = True
            if not last[e]["terminal"]: deaths_seen += int((ors[e].nodes()["status"] == 0).any())
        if done.all(): break
    assert done.all(), "a step stayed in flight for 4000 calls"
    return chk, deaths_seen


def check_density_action(z, k, act, nodes, where=""):
    """Fixture with `density_map=True` (the reference ran WRSN.step on G x G policy maps, WRSN.py:293-297, 229-287):
    `act` is what the implementation derived from map k on the node state `nodes` (energy / cs / status of the decision
    before: the state the reference optimised on).  Pinned by the fixture: third component (exact arithmetic on the map:
    arg-max value / mass above the 99.9th percentile), the box of the arg-max cell, and the objective value, which must
    not be below what SciPy's L-BFGS-B reached inside the reference (the spot itself is not reproducible across SciPy
    versions).  tests/density_ref.objective is itself pinned here against the reference's objective_function at the two
    points the fixture holds (box centre and the optimiser's result)."""
    import density_ref
    tag = "%s decision %d (density map)" % (where, k)
    frame = z["frame"]; W, H = frame[1] - frame[0], frame[3] - frame[2]
    ref3 = z["in_action"][k]                                   # the reference's 3-vector after np.clip (WRSN.py:299)
    assert abs(act[2] - ref3[2]) <= 1e-12 * max(ref3[2], 1e-300) or (ref3[2] == 1.0 and act[2] >= 1.0), (tag, "third", act[2], ref3[2])
    (lx, ux), (ly, uy) = z["dm_bounds"][k]
    spot = np.array([act[0] * W + frame[0], act[1] * H + frame[2]])
    tol = 1e-9 * max(ux - lx, uy - ly)
    assert lx - tol <= spot[0] <= ux + tol and ly - tol <= spot[1] <= uy + tol, (tag, "box", spot, z["dm_bounds"][k])
    args = (z["node_xy"], nodes["status"] == 1, nodes["energy"], nodes["cs"], float(z["node_spec"][1]), float(z["mc_spec"][4]),
            float(z["mc_spec"][5]), float(z["mc_spec"][6]))
    ref_best = -float(z["dm_fun"][k])
    # the checker's objective == the reference's own objective_function (values recorded inside the reference run)
    assert close(density_ref.objective(z["dm_x0"][k], *args), -float(z["dm_fun_x0"][k]), rtol=1e-7, atol=1e-12), (tag, "objective at the box centre")
    assert close(density_ref.objective(z["dm_x"][k], *args), ref_best, rtol=1e-7, atol=1e-12), (tag, "objective at SciPy's optimum")
    mine = density_ref.objective(np.clip(spot, [lx, ly], [ux, uy]), *args)
    assert mine >= ref_best * (1 - 1e-7) - 1e-12, (tag, "objective", mine, ref_best)
    return mine, ref_best


def replay_reference_fixture(Side, name):
    """The reference run tests/golden/<name>.npz on `Side` (sides.EmuSide / sides.VecSide): the frame and the constants of the network, the
    reset state, every decision through check_decision, and -- for a density_map=True run -- the action derived from the policy map of
    each decision."""
    from sides import load_fixture
    z, sc, mc = load_fixture(name)
    side = Side([sc], mc, int(z["num_agent"]), map_size=int(z["map_size"]), warm_up_time=float(z["warm_up"]))
    info = side.handle.env_info()
    assert close([info["xmin"][0], info["xmax"][0], info["ymin"][0], info["ymax"][0]], z["frame"], rtol=1e-14)
    assert close([info["moving_time_max"][0], info["charging_time_max"][0], info["avg_nodes_agent"][0], info["nodes_density"][0]], z["consts"], rtol=1e-12)
    side.reset()
    noise = []
    agent, _, reward, _, _ = side.rows()[0]
    assert agent == int(z["reset_agent"]) and reward == 0.0
    nd = side.handle.nodes()
    assert close(nd["energy"][0], z["reset_node_energy"]) and close(nd["cs"][0], z["reset_node_cs"], atol=1e-9)
    assert np.array_equal(nd["status"][0], z["reset_node_status"]) and np.array_equal(nd["level"][0], z["reset_node_level"])
    assert np.max(np.abs(side.obs_row(0) - z["reset_obs"])) <= 1e-5 * max(1.0, np.abs(z["reset_obs"]).max())
    for k in range(len(z["in_action"])):
        if "in_map" in z.files:                              # density_map=True fixture: the policy map of this decision
            nd = side.handle.nodes()
            act = side.density_action([int(z["in_agent"][k])], z["in_map"][k].astype(np.float64)[None])
            check_density_action(z, k, act[0], {"energy": nd["energy"][0], "cs": nd["cs"][0], "status": nd["status"][0]}, where=name)
        side.step([int(z["in_agent"][k])], z["in_action"][k][None])   # the reference's own 3-vector: the physics follow the fixture
        agent, _, reward, _, status = side.rows()[0]
        if z["is_none"][k]:
            assert status == 1 and agent == -1
            break
        assert status == 0
        if np.isinf(z["reward"][k]):
            assert reward == float(z["reward"][k])
            continue
        check_decision(z, k, side.decision(), where=name, noise=noise)
        if z["terminal"][k]:
            break
    print("%s on %s: %d of %d decisions replayed, %d rewards hang on a residue" % (name, Side.name, k + 1, len(z["in_action"]), len(noise)))
    assert len(noise) <= max(1, len(z["in_action"]) // 8), noise     # rewards that hang on the sign of a rounding residue stay rare
    side.close()
