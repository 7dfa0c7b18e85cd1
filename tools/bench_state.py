"""Throughput of environment records (wrsn_clone_envs, wrsn_save_envs + wrsn_load_envs) at the headline geometry: 4096 environments x
200 nodes x 200 targets x 3 chargers.  HIP events on the handle's stream around each call, a warm-up, the median of --reps repetitions.
Bytes are counted from the record layout: a clone reads and writes every segment of an environment (record bytes - 256 each way), a
save reads the segments and writes the record, a load reads the record and writes the segments.  Kernel time alone: run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_state.py`.

    python tools/bench_state.py [--envs 4096] [--nodes 200] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPEC_TBPS = 8.0          # MI355X HBM3E peak
STEP_MS = 0.64           # one headline step call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--targets", type=int, default=200)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    B, U = a.envs, 64
    uniq = [synth_scenario(9000 + u, a.nodes, a.targets) for u in range(U)]
    # 2B environments: a clone needs destinations that are not sources, so B sources [0, B) are cloned onto [B, 2B)
    env = VecWRSN([uniq[e % U] for e in range(2 * B)], None, a.agents, auto_reset=True, step_budget=1250, reuse_obs=True)
    g = torch.Generator().manual_seed(1)
    r = env.reset()
    for _ in range(8):
        r = env.step(r["agent_id"].clone(), torch.rand((2 * B, 3), generator=g, dtype=torch.float64))
    env.synchronize()
    R = env.record_bytes()
    rec = torch.empty((B, R), dtype=torch.uint8, device=env.device)
    src, dst = np.arange(B, dtype=np.int32), np.arange(B, 2 * B, dtype=np.int32)
    ptrs = env._out_ptrs()
    req = dict(ptrs); req.pop("obs")
    stream = torch.cuda.current_stream(env.device)

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

    # render=False in the copies below (obs pointer 0): the copy itself, not the observation pass
    no_obs = dict(ptrs); no_obs["obs"] = 0
    clone_ms, clone_wall = timed(lambda: env._h.clone_envs(src, dst, **no_obs))
    save_ms, save_wall = timed(lambda: env._h.save_envs(src, rec.data_ptr(), **req))
    load_ms, load_wall = timed(lambda: env._h.load_envs(dst, rec.data_ptr(), **no_obs))
    seg = R - 256
    out = {"envs": B, "nodes": a.nodes, "targets": a.targets, "agents": a.agents, "record_bytes": R, "reps": a.reps}
    for name, ms, wall, nbytes in (("clone", clone_ms, clone_wall, 2 * B * seg), ("save", save_ms, save_wall, B * (seg + R)),
                                   ("load", load_ms, load_wall, B * (R + seg))):
        gbs = nbytes / (ms * 1e-3) / 1e9
        out[name] = {"ms": round(ms, 4), "wall_ms": round(wall, 4), "bytes": nbytes, "GB_s": round(gbs, 1),
                     "spec_share": round(gbs / (SPEC_TBPS * 1e3), 3)}
    out["clone_vs_step_call"] = round(clone_ms / STEP_MS, 3)
    print(json.dumps(out), flush=True)
    env.close()


if __name__ == "__main__":
    main()
