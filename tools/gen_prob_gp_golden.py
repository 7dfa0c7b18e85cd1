"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/prob_gp/*.npz: reference runs with prob_gp < 1 (Node.py:61 draws
Python's MT19937 once per live node per second).

    python tools/gen_prob_gp_golden.py [case-name-substring ...]

Runs the reference's own classes through `run_case` of oracle/refharness/gen_golden.py (imported, not changed; only its
output folder and the number of full observations kept are set on the imported module) and adds to every fixture:
  * rng_draws_reset: random.random() calls since the last random.seed when reset() returned (the warm-up's draws),
  * rng_draws[k]: the same count after decision k,
  * seed64: the scenario seed as int64 (run_case keeps an int32 copy).
A wrapper around random.random counts the draws and records which node drew at which instant; for the case with the
node list reversed it asserts that at least one node alive at the start of an instant did not draw at that instant
(it was killed earlier in the same instant by the packets of a lower-id source: rule 4 of DESIGN.md section 2).

Seeds: 0 and the scenarios' own.  The reference cannot run a negative seed (np.random.seed in NetworkIO.py:22 refuses it) and
run_case stores the seed as int32; negative and two-word seeds are held to Python's `random` directly (tests/test_prob_gp.py).

The files are written with fixed zip timestamps so that a rerun gives byte-identical files.  The subfolder keeps them
away from tests/conftest.py:golden_names(), which globs tests/golden/*.npz only (the oracle refuses prob_gp < 1).
"""
import io
import os
import random
import sys
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "refharness"))
import gen_golden as gg  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "prob_gp")
gg.OUT = OUT
gg.OBS_FULL_DECISIONS = 1            # keeps every file well below 1 MB

_orig_random = random.random
_orig_seed = random.seed
_state = {"n": 0, "log": None}


def _counted_random():
    _state["n"] += 1
    if _state["log"] is not None:
        nd = sys._getframe(1).f_locals.get("self")
        if nd is not None and hasattr(nd, "net"):
            _state["log"].append((nd.env.now, nd.id, tuple(n.status for n in nd.net.listNodes)))
    return _orig_random()


def _counted_seed(*a, **kw):
    _state["n"] = 0
    return _orig_seed(*a, **kw)


random.random = _counted_random
random.seed = _counted_seed


def _recording(WRSN):
    class Rec(WRSN):
        draws = []

        def reset(self):
            r = super().reset()
            Rec.draws_reset = _state["n"]; Rec.draws = []
            return r

        def step(self, agent_id, action):
            r = super().step(agent_id, action)
            Rec.draws.append(_state["n"])
            return r
    return Rec


def _save(path, arrays):
    """np.savez_compressed with a fixed timestamp on every member."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def _skipped_draws(log):
    """Nodes alive at the first draw of an instant that did not draw at that instant."""
    by = {}
    for t, i, st in log:
        by.setdefault(t, []).append((i, st))
    skipped = 0
    for t, lst in by.items():
        alive0 = {k for k, s in enumerate(lst[0][1]) if s == 1}
        drew = {i for i, _ in lst}
        skipped += len([k for k in alive0 if k not in drew and k > lst[0][0]])
    return skipped


def with_pgp(s, p, seed=None, **kw):
    s = dict(s)
    spec = dict(s["node_phy_spe"]); spec["prob_gp"] = p
    for k, v in kw.items():
        spec[k] = v
    s["node_phy_spe"] = spec
    if seed is not None:
        s["seed"] = seed
    return s


def main():
    WRSN, _, _ = gg.load_reference()
    Rec = _recording(WRSN)
    mc = gg.mc_default()
    s6 = gg.six_node()
    a_bs = gg.bs_action(s6, 0.01)

    def short(seed, tmax):
        rng = np.random.RandomState(seed)
        return lambda i, req: np.array([rng.rand(), rng.rand(), tmax * rng.rand()])

    red = gg.redundant_net()
    red_rev = dict(red); red_rev["nodes"] = list(red["nodes"])[::-1]
    cases = [
        # name, scenario, M, policy, decisions, run_case keywords, check rule 4
        ("hanoi1000n50_m3_p05", with_pgp(gg.scen("hanoi1000n50"), 0.5), 3, gg.rnd(1), 40, {}, False),
        ("sonla1000n50_m2_p01", with_pgp(gg.scen("sonla1000n50"), 0.1), 2, gg.rnd(4), 40, {}, False),
        ("hanoi1000n100_m3_p09", with_pgp(gg.scen("hanoi1000n100"), 0.9), 3, gg.rnd(5), 40, {}, False),
        ("redundant_m2_p05", with_pgp(red, 0.5), 2, short(21, 0.6), 60, {}, False),
        ("redundant_rev_m2_p05", with_pgp(red_rev, 0.5), 2, short(21, 0.6), 60, {}, True),
        ("redundant_m2_maxtime130_p07", with_pgp(gg.redundant_net(max_time=130), 0.7), 2, short(23, 0.8), 24, {}, False),
        ("six_m1_bs_charge_ongrid_p05", with_pgp(s6, 0.5), 1, lambda i, r: a_bs, 12, {}, False),
        ("hanoi1000n50_m2_com100_p05", with_pgp(gg.scen("hanoi1000n50"), 0.5, com_range=100.0), 2, gg.rnd(12), 20, {}, False),
        ("hanoi1000n50_m1_warmup10_p05", with_pgp(gg.scen("hanoi1000n50"), 0.5), 1, gg.rnd(11), 2, dict(warm_up=10), False),
        ("hanoi1000n50_m1_warmup37_p05", with_pgp(gg.scen("hanoi1000n50"), 0.5), 1, gg.rnd(11), 2, dict(warm_up=37), False),
        ("hanoi1000n50_m2_p0_seed0", with_pgp(gg.scen("hanoi1000n50"), 0.0, seed=0), 2, gg.rnd(13), 20, {}, False),
    ]
    sel = sys.argv[1:]
    os.makedirs(OUT, exist_ok=True)
    for name, s, M, pol, n, kw, rule4 in cases:
        if sel and not any(x in name for x in sel):
            continue
        _state["log"] = [] if rule4 else None
        gg.run_case(name, s, mc, M, pol, n, Rec, **kw)
        path = os.path.join(OUT, name + ".npz")
        with np.load(path) as z:
            arrays = {k: z[k] for k in z.files}
        arrays["rng_draws_reset"] = np.int64(Rec.draws_reset)
        arrays["rng_draws"] = np.array(Rec.draws[:len(arrays["now"])], dtype=np.int64)
        arrays["seed64"] = np.int64(s["seed"])
        if rule4:
            sk = _skipped_draws(_state["log"])
            assert sk >= 1, "%s: no draw was skipped within an instant" % name
            arrays["rule4_skipped"] = np.int64(sk)
        _state["log"] = None
        _save(path, arrays)
        print("%-34s draws at reset %d, at the end %d, %.0f KB" % (name, Rec.draws_reset, Rec.draws[-1], os.path.getsize(path) / 1024), flush=True)


if __name__ == "__main__":
    main()
