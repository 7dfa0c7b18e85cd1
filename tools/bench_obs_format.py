"""float32 against bf16 observations (wrsn_set_obs_format) at the headline geometry: 4096 environments x 200 nodes x 200 targets x
3 chargers, G = 100, seeded synthetic networks, random actions, auto-reset, step_budget 1250, reuse_obs.  One handle per format and
per launch shape in the same process; the formats take turns in windows of --launches step calls, so that drift of the machine hits
both alike.  Per format, the median and the min / max over the windows of

  * obs_kernel_ms        wrsn_kernel_times ms[3]: the observation kernel of a step call, on handles created with the pipeline off
                         (WRSN_PIPE=0: one observation launch over the whole batch behind the step kernel);
  * step_call_ms, env_steps_per_s   wall clock of a window of step calls with the pipeline on (the default launch shape);

and the bytes of the observation tensors: `VecWRSN.state` and the three state tensors of `TransitionBuffers` with bench_ippo.py's
settings (capacity 4096), computed from the shapes and the element size.  The two handles of a launch shape get the same action stream:
their trajectories are identical, so they render the same rows.

    python tools/bench_obs_format.py [--envs 4096] [--windows 5] [--launches 100] [--out profiles/obs_bf16_bench.json]

Kernel time of both instantiations alone: `rocprofv3 --kernel-trace --stats -- python tools/bench_obs_format.py`; bytes written:
`rocprofv3 --pmc WRITE_SIZE -- python tools/bench_obs_format.py` in a run of its own.  `--summarize DIR TAG` turns the csv files of
those two runs (DIR/stats, DIR/write) into profiles-style summaries DIR/TAG_kernel_stats.csv and DIR/TAG_write_size.json.
"""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"float32": "wrsn_obs_kernel", "bfloat16": "wrsn_obs_bf16_kernel"}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "windows": len(v)}


def summarize(d, tag, envs):
    """rocprofv3 csv output -> per-kernel durations and WRITE_SIZE (KiB per dispatch) of the two observation kernels; dispatches over the
    whole batch only (grid = 256 threads x envs: the pipeline-off handles), which render the same rows in both formats."""
    out = {}
    st = glob.glob(os.path.join(d, "stats", "**", "*kernel_stats.csv"), recursive=True)
    if st:
        rows = [r for r in csv.DictReader(open(st[0])) if "wrsn_" in r["Name"]]
        with open(os.path.join(d, tag + "_kernel_stats.csv"), "w") as w:
            w.write("Name,Calls,TotalDurationNs,AverageNs,MinNs,MaxNs\n")
            for r in rows:
                w.write('"%s",%s,%s,%s,%s,%s\n' % (r["Name"], r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["MinNs"], r["MaxNs"]))
    tr = glob.glob(os.path.join(d, "stats", "**", "*kernel_trace.csv"), recursive=True)
    if tr:                                                      # full-batch dispatches only, like the counters below
        agg = collections.defaultdict(list)
        for r in csv.DictReader(open(tr[0])):
            for fmt, k in KERNELS.items():
                if k in r["Kernel_Name"] and int(r["Grid_Size_X"]) >= 256 * envs:
                    agg[fmt].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        out["full_batch_dispatch_us"] = {f: {"dispatches": len(v), "mean": statistics.mean(v), "median": statistics.median(v)} for f, v in agg.items()}
    pm = glob.glob(os.path.join(d, "write", "**", "*counter_collection.csv"), recursive=True)
    if pm:
        agg = collections.defaultdict(list)
        for r in csv.DictReader(open(pm[0])):
            if r["Counter_Name"] != "WRITE_SIZE":
                continue
            for fmt, k in KERNELS.items():
                if k in r["Kernel_Name"] and int(r["Grid_Size"]) >= 256 * envs:
                    agg[fmt].append(float(r["Counter_Value"]))
        out["write_size_kib_per_full_batch_dispatch"] = {f: {"dispatches": len(v), "mean": statistics.mean(v)} for f, v in agg.items()}
        if len(agg) == 2:
            out["write_size_ratio_bf16_over_f32"] = statistics.mean(agg["bfloat16"]) / statistics.mean(agg["float32"])
    json.dump(out, open(os.path.join(d, tag + "_write_size.json"), "w"), indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--targets", type=int, default=200)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--map-size", type=int, default=100)
    ap.add_argument("--step-budget", type=int, default=1250)
    ap.add_argument("--windows", type=int, default=5, help="windows per format (they alternate)")
    ap.add_argument("--launches", type=int, default=100, help="step calls per window")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    ap.add_argument("--summarize", nargs=2, metavar=("DIR", "TAG"), default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize[0], a.summarize[1], a.envs)
    import torch
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    B, M, G, U = a.envs, a.agents, a.map_size, 64
    uniq = [synth_scenario(9000 + u, a.nodes, a.targets) for u in range(U)]
    scs = [uniq[e % U] for e in range(B)]
    dev = torch.device("cuda:0")

    class Run:
        def __init__(self, fmt, pipe):
            old = os.environ.get("WRSN_PIPE")
            os.environ["WRSN_PIPE"] = "1" if pipe else "0"      # read when the handle is created
            try:
                self.env = VecWRSN(scs, None, M, map_size=G, auto_reset=True, step_budget=a.step_budget, reuse_obs=True, obs_dtype=fmt)
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
            ms = 0.0
            for _ in range(n):
                self.r = self.env.step(self.r["agent_id"], torch.rand((B, 3), generator=self.gen, device=dev, dtype=torch.float64))
                if timed:
                    ms += self.env._h.kernel_times()["obs_ms"]
            return ms / max(1, n)

    fmts = ("float32", "bfloat16")
    piped = {f: Run(f, True) for f in fmts}
    plain = {f: Run(f, False) for f in fmts}
    for f in fmts:
        plain[f].env._h.set_timing(True)
    res = {f: {"obs_kernel_ms": [], "step_call_ms": [], "env_steps_per_s": []} for f in fmts}
    for w in range(a.windows):
        for f in fmts:
            res[f]["obs_kernel_ms"].append(plain[f].step(a.launches, timed=True))
            p = piped[f]
            torch.cuda.synchronize(dev)
            c0 = p.env.counters()["env_steps"]; t0 = time.perf_counter()
            p.step(a.launches)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            res[f]["step_call_ms"].append(1e3 * dt / a.launches)
            res[f]["env_steps_per_s"].append((p.env.counters()["env_steps"] - c0) / dt)
    cap = 4096
    out = {"config": {"envs": B, "nodes": a.nodes, "targets": a.targets, "chargers": M, "map_size": G, "step_budget": a.step_budget, "reuse_obs": True,
                      "windows_per_format": a.windows, "launches_per_window": a.launches, "warmup_launches": a.warmup},
           "device": torch.cuda.get_device_name(0)}
    for f in fmts:
        es = piped[f].env.state.element_size()
        out[f] = {k: spread(v) for k, v in res[f].items()}
        out[f]["bytes"] = {"VecWRSN.state": B * 4 * G * G * es, "TransitionBuffers.pend_state": B * M * 4 * G * G * es,
                           "TransitionBuffers.state + next_state (capacity %d)" % cap: 2 * M * cap * 4 * G * G * es}
    out["bf16_over_f32"] = {k: out["bfloat16"][k]["median"] / out["float32"][k]["median"] for k in ("obs_kernel_ms", "step_call_ms", "env_steps_per_s")}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as w:
            w.write(line + "\n")
    for r in list(piped.values()) + list(plain.values()):
        r.env.close()


if __name__ == "__main__":
    main()
