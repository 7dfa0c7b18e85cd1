"""Cost of scenario pools (wrsn_pool_set / wrsn_pool_reset) at the headline geometry: 4096 environments x 200 nodes x 200 targets x
3 chargers.  Three measurements, all in one run:

  1. a wrsn_pool_reset that replaces nothing (NULL mask, no row terminal; observation pointer set, as VecWRSN.step calls it);
  2. a wrsn_pool_reset that replaces every row, next to wrsn_load_envs of the same records into the same rows and wrsn_clone_envs of as
     many environments (observation pointer NULL in all three: the copy, not the render pass).  Bytes as tools/bench_state.py counts them;
  3. VecWRSN.step with auto_reset=True on a pooled and an unpooled batch over the same scenarios, in alternating windows.

HIP events on the handle's stream, --warmup calls, the median of --reps (1, 2); wall clock per window, medians over the windows (3).

    python tools/bench_pool.py [--envs 4096] [--nodes 200] [--out profiles/pool_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "windows": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--targets", type=int, default=200)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-budget", type=int, default=1250)
    ap.add_argument("--windows", type=int, default=5, help="windows per batch (they alternate)")
    ap.add_argument("--launches", type=int, default=100, help="step calls per window")
    ap.add_argument("--step-warmup", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import VecWRSN, build_scenario_pool, synth_scenario
    B, M, U = a.envs, a.agents, 64
    dev = torch.device("cuda:0")
    uniq = [synth_scenario(9000 + u, a.nodes, a.targets) for u in range(U)]
    scs = [uniq[e % U] for e in range(B)]
    stream = torch.cuda.current_stream(dev)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream); fn(); e1.record(stream)
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3); ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), statistics.median(wall)

    out = {"config": {"envs": B, "nodes": a.nodes, "targets": a.targets, "chargers": M, "reps": a.reps, "warmup": a.warmup,
                      "step_budget": a.step_budget, "windows_per_batch": a.windows, "launches_per_window": a.launches,
                      "step_warmup_launches": a.step_warmup},
           "device": torch.cuda.get_device_name(0)}

    # ---- 1, 2: one batch of B environments for the pool reset and the load, one of 2B for the clone (sources are no destinations)
    env = VecWRSN(scs, None, M, auto_reset=True, step_budget=a.step_budget, reuse_obs=True)
    env.reset()
    R = env.record_bytes(); seg = R - 256
    rec = env.save_envs()                                     # B records saved right after reset(): the pool
    env.set_pool(rec, 1)
    ptrs = env._out_ptrs()
    no_obs = dict(ptrs); no_obs["obs"] = 0
    ones = torch.ones(B, dtype=torch.uint8, device=dev); index = torch.arange(B, dtype=torch.int32, device=dev)
    ids = torch.zeros(B, dtype=torch.int32, device=dev)
    all_rows = np.arange(B, dtype=np.int32)
    full_ms, full_wall = timed(lambda: env._h.pool_reset(ones.data_ptr(), index.data_ptr(), ids.data_ptr(), **no_obs))
    load_ms, load_wall = timed(lambda: env._h.load_envs(all_rows, rec.data_ptr(), **no_obs))
    assert int(env.terminal.sum()) == 0                       # every row is a fresh reset: a NULL mask selects nothing
    none_ms, none_wall = timed(lambda: env._h.pool_reset(0, 0, ids.data_ptr(), **ptrs))
    assert int(env.pool_info()["swaps"].sum()) == B * (a.reps + a.warmup)
    env.set_pool(None)
    env.close(); del rec
    env2 = VecWRSN(scs + scs, None, M, auto_reset=True, step_budget=a.step_budget, reuse_obs=True)
    env2.reset()
    p2 = env2._out_ptrs(); p2["obs"] = 0
    clone_ms, clone_wall = timed(lambda: env2._h.clone_envs(all_rows, all_rows + B, **p2))
    env2.close()
    out["record_bytes"] = R
    for name, ms, wall, nbytes in (("pool_reset_nothing", none_ms, none_wall, 0), ("pool_reset_all", full_ms, full_wall, B * (R + seg)),
                                   ("load", load_ms, load_wall, B * (R + seg)), ("clone", clone_ms, clone_wall, 2 * B * seg)):
        out[name] = {"ms": round(ms, 4), "wall_ms": round(wall, 4), "bytes": nbytes, "GB_s": round(nbytes / (ms * 1e-3) / 1e9, 1)}
    out["pool_reset_all_over_load"] = round(full_ms / load_ms, 3)

    # ---- 3: the step call, pooled against unpooled, alternating windows
    pool = build_scenario_pool(uniq, None, M, n_node=a.nodes, n_target=a.targets)

    class Run:
        def __init__(self, pooled):
            self.env = VecWRSN(scs, None, M, auto_reset=True, step_budget=a.step_budget, reuse_obs=True)
            if pooled:
                self.env.set_pool(pool, 7)
            self.gen = torch.Generator(device=dev).manual_seed(7)
            self.r = self.env.reset()
            self.step(a.step_warmup)
            torch.cuda.synchronize(dev)

        def step(self, n):
            for _ in range(n):
                self.r = self.env.step(self.r["agent_id"], torch.rand((B, 3), generator=self.gen, device=dev, dtype=torch.float64))

    runs = {"unpooled": Run(False), "pooled": Run(True)}
    res = {k: {"step_call_ms": [], "env_steps_per_s": []} for k in runs}
    for w in range(a.windows):
        for k, r in runs.items():
            torch.cuda.synchronize(dev)
            c0 = r.env.counters()["env_steps"]; t0 = time.perf_counter()
            r.step(a.launches)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            res[k]["step_call_ms"].append(1e3 * dt / a.launches)
            res[k]["env_steps_per_s"].append((r.env.counters()["env_steps"] - c0) / dt)
    for k in runs:
        out[k] = {m: spread(v) for m, v in res[k].items()}
    out["pooled"]["swaps"] = int(runs["pooled"].env.pool_info()["swaps"].sum())
    out["pooled_over_unpooled"] = {m: out["pooled"][m]["median"] / out["unpooled"][m]["median"] for m in ("step_call_ms", "env_steps_per_s")}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as w:
            w.write(line + "\n")
    for r in runs.values():
        r.env.close()


if __name__ == "__main__":
    main()
