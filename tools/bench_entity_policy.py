"""Acting from entity rows on the device against the PyTorch loop at the headline geometry: 4096 environments x 200 nodes x 3 chargers,
the seeded synthetic networks of bench.py, the entity rows a reset leaves.  The two kinds take turns in windows of the same run on the
same rows, the same ids and the same weights (the learner's initial ones):
  fused  VecWRSN.entity_act (wrsn_entity_act: three launches), the HIP-event time around the call;
  torch  what BatchedEntityIPPO.step_batch does per launch without the fused option -- nonzero, index_select, pack, get_action per charger,
         index_copy_, .double() -- the synchronised wall time around the loop (it synchronises on its own: nonzero).
3 warm-up calls per window, then the median, minimum and maximum of 20.

    python tools/bench_entity_policy.py [--envs 4096] [--windows 5] [--out profiles/entity_act_bench.json]

What would be a defect rather than a number: the fused call not faster than the torch loop of the same run.  The line also says how many
times the floor of the layout the fused call takes: 1.93 MFLOP a row, 7.9 GFLOP for 4096 rows, about 50 us at the 157 TFLOP/s float32
matrix rate."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flop_per_row(N, M):
    """Multiply-adds x 2 of one row of the actor."""
    return 2 * (N * (8 * 64 + 64 * 64) + M * (12 * 32 + 32 * 32) + 200 * 128 + 128 * 128 + 2 * 128 * 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--infer-chunk", type=int, default=512)
    ap.add_argument("--windows", type=int, default=5, help="windows per kind (they alternate)")
    ap.add_argument("--calls", type=int, default=20, help="timed calls per window")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls at the start of every window")
    ap.add_argument("--peak-tflops", type=float, default=157.0, help="float32 matrix rate the floor is taken at")
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    import torch
    from multi_agent_rl_wrsn_amd import EntityPPOLearner, EntityTransitionBuffers, VecWRSN, synth_scenario
    B, N, M, U = a.envs, a.nodes, a.agents, 64
    uniq = [synth_scenario(9000 + u, N, N) for u in range(U)]
    dev = torch.device("cuda:0")
    env = VecWRSN([uniq[e % U] for e in range(B)], None, M, render=False, entities=True, auto_reset=True)
    torch.manual_seed(0)
    lr = EntityPPOLearner({}, M, dev, infer_chunk=a.infer_chunk, min_bucket=a.infer_chunk)
    packed = lr.packed_actors()
    r = env.reset()
    # a reset asks for charger 0 everywhere: spread the requests over the chargers and write the rows those chargers would see
    ids = (torch.arange(B, device=dev) % M).to(torch.int32)
    rows = env.entity_state(ids)
    env.nodes_feat.copy_(rows["nodes"]); env.chargers_feat.copy_(rows["chargers"]); env.env_feat.copy_(rows["env_feat"])
    eps = torch.randn((B, 3), dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def fused(timed):
        ev[0].record(); env.entity_act(ids, packed, eps); ev[1].record()
        if not timed:
            return None
        torch.cuda.synchronize(dev)
        return ev[0].elapsed_time(ev[1])

    def loop(timed):
        torch.cuda.synchronize(dev); t0 = time.perf_counter()
        act3 = torch.zeros((B, 3), dtype=torch.float32, device=dev); logp = torch.zeros((B,), dtype=torch.float32, device=dev)
        for c in range(M):
            sel = torch.nonzero(ids == c).flatten()
            if sel.numel() == 0:
                continue
            x = EntityTransitionBuffers.pack(env.nodes_feat.index_select(0, sel), env.chargers_feat.index_select(0, sel), env.env_feat.index_select(0, sel))
            act, lp = lr.get_action(c, x)
            act3.index_copy_(0, sel, act.float()); logp.index_copy_(0, sel, lp.float())
        act3.double()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 if timed else None

    kinds = {"fused": fused, "torch": loop}
    res = {k: [] for k in kinds}
    for _ in range(a.windows):
        for kind, f in kinds.items():
            for _ in range(a.warmup):
                f(False)
            s = [f(True) for _ in range(a.calls)]
            res[kind].append({"median": statistics.median(s), "min": min(s), "max": max(s)})
    flop = flop_per_row(N, M) * B
    floor_ms = flop / (a.peak_tflops * 1e12) * 1e3
    out = {"config": {"envs": B, "nodes": N, "chargers": M, "infer_chunk": a.infer_chunk, "windows_per_kind": a.windows, "timed_calls_per_window": a.calls,
                      "warmup_calls_per_window": a.warmup, "fused_sample": "HIP-event time around VecWRSN.entity_act, ms",
                      "torch_sample": "synchronised wall time around the per-charger get_action loop of step_batch, ms"},
           "device": torch.cuda.get_device_name(0), "flop_per_call": flop, "floor_ms_at_peak": floor_ms, "peak_tflops": a.peak_tflops}
    for kind in kinds:
        w = res[kind]
        out[kind + "_ms"] = {"windows": w, "median_of_window_medians": statistics.median(x["median"] for x in w), "min": min(x["min"] for x in w),
                             "max": max(x["max"] for x in w)}
    f_ms, t_ms = out["fused_ms"]["median_of_window_medians"], out["torch_ms"]["median_of_window_medians"]
    out["torch_over_fused"] = t_ms / f_ms
    out["fused_over_floor"] = f_ms / floor_ms
    out["fused_tflops"] = flop / (f_ms * 1e-3) / 1e12
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as w:
            w.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
