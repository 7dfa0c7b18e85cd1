"""Image against entity observations at the headline geometry: 4096 environments x 200 nodes x 200 targets x 3 chargers, G = 100, the
seeded synthetic networks and random policy of bench.py, auto-reset, step_budget 1250.  One handle per configuration and launch shape in
the same process:

  image     VecWRSN(render=True)                    the 4 x G x G observation (reuse_obs, as bench.py)
  entities  VecWRSN(render=False, entities=True)    the entity observation alone
  both      VecWRSN(render=True, entities=True)
  neither   VecWRSN(render=False)

The configurations take turns in windows of --launches step calls, so that drift of the machine hits all alike.  Per configuration and
window: wrsn_kernel_times (means over the window's calls, on handles created with WRSN_PIPE=0: one step launch, then the observation
and entity launches over the whole batch; ms[3] holds both) and, on handles with the default launch shape, the wall clock of a step
call and env-steps/s.  All handles get the same action stream.

    python tools/bench_entities.py [--envs 4096] [--windows 5] [--launches 100] [--out profiles/entity_obs_bench.json]

Duration of the entity kernel per dispatch: `rocprofv3 --kernel-trace --stats -d DIR -f csv -- python tools/bench_entities.py`, then
`python tools/bench_entities.py --summarize DIR OUT.csv`: the dispatches of the observation and entity kernels grouped by kernel and grid
size (a grid of 256 x envs threads is a launch over the whole batch, the smaller ones are the halves of the pipeline).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"image": dict(render=True, reuse_obs=True), "entities": dict(render=False, entities=True),
           "both": dict(render=True, reuse_obs=True, entities=True), "neither": dict(render=False)}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "windows": list(v)}


def summarize(d, out):
    import collections, csv, glob
    tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(tr[0])):
        name = r["Kernel_Name"].split("(")[0]
        if "wrsn_obs" in name or "wrsn_entity" in name:
            agg[(name, int(r["Grid_Size_X"]))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    with open(out, "w") as w:
        w.write("kernel,grid_threads,dispatches,mean_us,median_us,min_us,max_us\n")
        for (name, grid), v in sorted(agg.items()):
            w.write('"%s",%d,%d,%.3f,%.3f,%.3f,%.3f\n' % (name, grid, len(v), statistics.mean(v), statistics.median(v), min(v), max(v)))
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--targets", type=int, default=200)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--map-size", type=int, default=100)
    ap.add_argument("--step-budget", type=int, default=1250)
    ap.add_argument("--windows", type=int, default=5, help="windows per configuration (they alternate)")
    ap.add_argument("--launches", type=int, default=100, help="step calls per window")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    ap.add_argument("--summarize", nargs=2, metavar=("DIR", "OUT"), default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(*a.summarize)
    import torch
    from multi_agent_rl_wrsn_amd import ENT_ENV_F, ENT_MC_F, ENT_NODE_F, VecWRSN, synth_scenario
    B, M, G, U = a.envs, a.agents, a.map_size, 64
    uniq = [synth_scenario(9000 + u, a.nodes, a.targets) for u in range(U)]
    scs = [uniq[e % U] for e in range(B)]
    dev = torch.device("cuda:0")

    class Run:
        def __init__(self, cfg, pipe):
            old = os.environ.get("WRSN_PIPE")
            os.environ["WRSN_PIPE"] = "1" if pipe else "0"      # read when the handle is created
            try:
                self.env = VecWRSN(scs, None, M, map_size=G, auto_reset=True, step_budget=a.step_budget, **CONFIGS[cfg])
            finally:
                if old is None:
                    os.environ.pop("WRSN_PIPE")
                else:
                    os.environ["WRSN_PIPE"] = old
            self.gen = torch.Generator(device=dev).manual_seed(7)
            self.r = self.env.reset()
            self.step(a.warmup)
            torch.cuda.synchronize(dev)

        def step(self, n, timed=False):
            acc = {"order_ms": 0.0, "step_ms": 0.0, "obs_ms": 0.0}
            for _ in range(n):
                self.r = self.env.step(self.r["agent_id"], torch.rand((B, 3), generator=self.gen, device=dev, dtype=torch.float64))
                if timed:
                    t = self.env._h.kernel_times()
                    for k in acc:
                        acc[k] += t[k]
            return {k: v / max(1, n) for k, v in acc.items()}

    piped = {c: Run(c, True) for c in CONFIGS}
    plain = {c: Run(c, False) for c in CONFIGS}
    for c in CONFIGS:
        plain[c].env._h.set_timing(True)
    res = {c: {"order_ms": [], "step_ms": [], "obs_ms": [], "step_call_ms": [], "env_steps_per_s": []} for c in CONFIGS}
    for w in range(a.windows):
        for c in CONFIGS:
            for k, v in plain[c].step(a.launches, timed=True).items():
                res[c][k].append(v)
            p = piped[c]
            torch.cuda.synchronize(dev)
            c0 = p.env.counters()["env_steps"]; t0 = time.perf_counter()
            p.step(a.launches)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            res[c]["step_call_ms"].append(1e3 * dt / a.launches)
            res[c]["env_steps_per_s"].append((p.env.counters()["env_steps"] - c0) / dt)
    out = {"config": {"envs": B, "nodes": a.nodes, "targets": a.targets, "chargers": M, "map_size": G, "step_budget": a.step_budget,
                      "windows_per_configuration": a.windows, "launches_per_window": a.launches, "warmup_launches": a.warmup,
                      "kernel_times": "wrsn_kernel_times means per window on WRSN_PIPE=0 handles; obs_ms = ms[3]: image and entity launches"},
           "device": torch.cuda.get_device_name(0),
           "bytes_per_row": {"image": 4 * G * G * 4, "entities": 4 * (a.nodes * ENT_NODE_F + M * ENT_MC_F + ENT_ENV_F)}}
    for c in CONFIGS:
        out[c] = {k: spread(v) for k, v in res[c].items()}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as w:
            w.write(line + "\n")
    for r in list(piped.values()) + list(plain.values()):
        r.env.close()


if __name__ == "__main__":
    main()
