"""Throughput of the stochastic kernels (prob_gp < 1) on bench.py's workload: B synthetic networks of N nodes / N targets, M chargers,
auto-reset, the default step budget, a random policy -- with every environment at the given prob_gp (seed of env e: seed + e).
Prints one JSON line: env-steps per second of the timed region, the same for prob_gp == 1 on the same networks (the headline path) in
the same process, and the per-kernel times of the library's own event pass.

    python tools/bench_prob_gp.py [--envs 4096 --nodes 200 --mcs 3 --prob-gp 0.5 --steps 100 --warmup 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_prob_gp.py --steps 20 --skip-plain
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(torch, scenarios, M, budget, steps, warmup, kernel_steps, seed):
    from multi_agent_rl_wrsn_amd import VecWRSN
    B = len(scenarios)
    env = VecWRSN(scenarios, None, M, auto_reset=True, step_budget=budget, reuse_obs=True)
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    r = env.reset()
    for _ in range(max(1, warmup)):
        r = env.step(r["agent_id"], torch.rand((B, 3), generator=gen, device=dev, dtype=torch.float64))
    torch.cuda.synchronize(dev)
    c0 = env.counters()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = env.step(r["agent_id"], torch.rand((B, 3), generator=gen, device=dev, dtype=torch.float64))
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    c1 = env.counters()
    env._h.set_timing(True)
    t_env = t_obs = 0.0
    for _ in range(kernel_steps):
        r = env.step(r["agent_id"], torch.rand((B, 3), generator=gen, device=dev, dtype=torch.float64))
        kt = env._h.kernel_times()
        t_env += (kt["step_ms"] + kt["continuation_ms"]); t_obs += kt["obs_ms"]
    env._h.set_timing(False)
    out = {"env_steps_per_s": (c1["env_steps"] - c0["env_steps"]) / el, "elapsed_s": el, "env_steps": c1["env_steps"] - c0["env_steps"],
           "sim_seconds": c1["sim_seconds_total"] - c0["sim_seconds_total"],
           "step_kernel_ms": t_env / max(1, kernel_steps), "obs_kernel_ms": t_obs / max(1, kernel_steps)}
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--mcs", type=int, default=3)
    ap.add_argument("--prob-gp", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernel-steps", type=int, default=10)
    ap.add_argument("--step-budget", type=int, default=1250)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-plain", action="store_true", help="measure the stochastic kernels only")
    args = ap.parse_args()
    import torch
    from multi_agent_rl_wrsn_amd import DEFAULT_NODE_SPEC, Scenario, synth_scenario
    spec = dict(DEFAULT_NODE_SPEC); spec["prob_gp"] = args.prob_gp
    plain = [synth_scenario(args.seed + e, args.nodes, args.nodes) for e in range(args.envs)]
    stoch = [Scenario(s.node_xy, s.target_xy, s.bs_xy, spec, s.max_time, args.seed + e, stochastic_packets=True) for e, s in enumerate(plain)]
    res = {"metric": "env_steps_per_s", "envs": args.envs, "nodes": args.nodes, "targets": args.nodes, "chargers": args.mcs, "prob_gp": args.prob_gp,
           "step_budget": args.step_budget, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    res["stochastic"] = run(torch, stoch, args.mcs, args.step_budget, args.steps, args.warmup, args.kernel_steps, args.seed)
    if not args.skip_plain:
        res["prob_gp_1"] = run(torch, plain, args.mcs, args.step_budget, args.steps, args.warmup, args.kernel_steps, args.seed)
        res["ratio"] = res["stochastic"]["env_steps_per_s"] / res["prob_gp_1"]["env_steps_per_s"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
