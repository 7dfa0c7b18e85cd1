"""TEST INFRASTRUCTURE -- wide parity sweep (uses the test oracle; also run small by test_gpu_parity.py): B synthetic environments stepped side by side on the GPU (blocking
and budgeted) and by the CPU oracle, whole episodes with resets, every request compared.  Far more cases than the -m gpu
tests run; intended for spare GPU time after a change to the exact-second / scheduling code."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from concurrent.futures import ThreadPoolExecutor
from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
from wrsn_oracle import OracleWRSN
from parity import RequestCheck
from sides import VecSide


def run(B=192, K=60, budget=0, seed0=20000, N=200, verbose=True, M=None, deadline_us=None, sizes=None, node_spec=None, side=None):
    """returns (requests compared, finished episodes, noise-dependent requests); raises AssertionError on a mismatch.
    sizes: list of (n_node, n_target) cycled over the environments (a ragged batch in one handle; None: N nodes and N targets everywhere);
    node_spec: the node parameters of every network (None: the shipped ones); side: sides.VecSide (the GPU, default) or sides.EmuSide."""
    M = int(os.environ.get("WRSN_M", "3")) if M is None else M
    deadline_us = int(os.environ.get("WRSN_DEADLINE_US", "0")) if deadline_us is None else deadline_us
    sizes = [(N, N)] if sizes is None else list(sizes)
    scs = [synth_scenario(seed0 + e, sizes[e % len(sizes)][0], sizes[e % len(sizes)][1], node_spec=node_spec) for e in range(B)]
    env = (VecSide if side is None else side)(scs, DEFAULT_MC_SPEC, M, step_budget=budget, step_deadline_us=deadline_us)
    ors = [OracleWRSN(s.node_xy, s.target_xy, s.bs_xy, s.node_spec, DEFAULT_MC_SPEC, s.max_time, M) for s in scs]
    chk = RequestCheck(scs)
    env.reset()
    last = [o.reset() for o in ors]
    chk.remember(range(B), env.view(), reset=True)
    rng = np.random.RandomState(seed0)
    pool = ThreadPoolExecutor(max_workers=min(64, os.cpu_count() or 8))
    n_term = 0; t0 = time.time()
    busy = np.zeros(B, dtype=bool); pending = [None] * B
    for step in range(K):
        act = rng.rand(B, 3)
        ids = np.full(B, -1, dtype=np.int64)
        for e in range(B):
            if busy[e]: continue
            if last[e]["terminal"]:
                last[e] = None
        mask = np.array([last[e] is None and not busy[e] for e in range(B)], dtype=np.uint8)
        if mask.any():                                          # reset finished episodes on both sides
            env.reset(mask)
            for e in np.nonzero(mask)[0]:
                last[e] = ors[e].reset(); n_term += 1
            chk.remember(np.nonzero(mask)[0], env.view(), reset=True)
        for e in range(B):
            if not busy[e]:
                ids[e] = -1 if last[e]["agent_id"] is None else last[e]["agent_id"]
                pending[e] = (last[e]["agent_id"], act[e].copy()); chk.submit(e, last[e]["agent_id"])
        env.step(ids, act)
        v = env.view(); st = v["status"]
        fresh = [e for e in range(B) if st[e] != 4]
        def ostep(e):
            a, x = pending[e]
            return ors[e].step(a, x)
        res = list(pool.map(ostep, fresh))
        for e, x in zip(fresh, res):
            last[e] = x
            chk.fresh(step, e, x, ors[e], v)
        busy = st == 4
        if verbose and step % 10 == 9:
            print("step %d: %d requests compared (%d noise-dependent), %d episodes finished, worst reward rel err %.2e, worst obs err %.2e, %.0f s" % (step + 1, chk.n_cmp, chk.n_noise, n_term, chk.worst_rew, chk.worst_obs, time.time() - t0), flush=True)
    n_cmp, n_noise = chk.n_cmp, chk.n_noise
    print("parity sweep ok: %d requests, %d finished episodes; %d requests with a reward that depends on the sign of a rounding-noise energyCS (not comparable)" % (n_cmp, n_term, n_noise))
    print("prev_minfit traced back to the fitness reported with the request: %d actions" % chk.n_prov)
    env.close(); pool.shutdown()
    assert n_noise <= max(2, n_cmp // 200), "more than 0.5 %% of the requests hang on a rounding-residue energyCS: %d of %d" % (n_noise, n_cmp)
    return n_cmp, n_term, n_noise


if __name__ == "__main__":
    run(B=int(os.environ.get("WRSN_B", "192")), K=int(os.environ.get("WRSN_K", "60")), budget=int(os.environ.get("WRSN_BUDGET", "0")),
        seed0=int(os.environ.get("WRSN_SEED", "20000")), N=int(os.environ.get("WRSN_N", "200")))
