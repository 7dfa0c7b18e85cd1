"""Acting with the node-pointer policy on the device against the PyTorch loop at the headline geometry: 4096 environments x 200 nodes x 3
chargers, the seeded synthetic networks of bench.py, the entity rows a reset leaves.  The two kinds take turns in windows of the same run
on the same rows, the same ids and the same weights (the learner's initial ones):
  fused  VecWRSN.entity_pointer_act (wrsn_entity_pointer_act: four launches) with Gumbel noise and draws made beforehand, the HIP-event
         time around the call;
  torch  what BatchedEntityPointerIPPO.step_batch does per launch without the fused option -- nonzero, index_select, pack, get_action per
         charger (its noise included), index_copy_ -- the synchronised wall time around the loop.
3 warm-up calls per window, then the median, minimum and maximum of 20.

    python tools/bench_entity_pointer.py [--envs 4096] [--windows 5] [--only fused] [--out profiles/entity_pointer_act_bench.json]

--mask-claimed adds a third kind, `masked`: the fused call under wrsn_set_entity_pointer_mask(WRSN_POINTER_MASK_CLAIMED), alternating with
the others (the mode is set in front of every window); `--only masked` runs it alone.  The torch loop stays unmasked.

What would be a defect rather than a number: the fused call slower than the torch loop of the same run beyond the spread of the windows.
For context the line carries the ratio to wrsn_entity_act's recorded time (profiles/entity_act_bench.json) when that file is there: the
second pass over the nodes makes up to about 2 x plausible."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--infer-chunk", type=int, default=512)
    ap.add_argument("--windows", type=int, default=5, help="windows per kind (they alternate)")
    ap.add_argument("--calls", type=int, default=20, help="timed calls per window")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls at the start of every window")
    ap.add_argument("--min-charge", type=float, default=0.02)
    ap.add_argument("--only", default=None, choices=[None, "fused", "torch", "masked"], help="run one kind alone (for a kernel trace)")
    ap.add_argument("--mask-claimed", action="store_true", help="also time the fused call with the candidate mask on (kind `masked`)")
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    import torch
    from multi_agent_rl_wrsn_amd import EntityPointerPPOLearner, EntityTransitionBuffers, VecWRSN, synth_scenario
    B, N, M, U = a.envs, a.nodes, a.agents, 64
    uniq = [synth_scenario(9000 + u, N, N) for u in range(U)]
    dev = torch.device("cuda:0")
    env = VecWRSN([uniq[e % U] for e in range(B)], None, M, render=False, entities=True, auto_reset=True)
    torch.manual_seed(0)
    lr = EntityPointerPPOLearner({}, M, dev, infer_chunk=a.infer_chunk, min_bucket=a.infer_chunk)
    packed = lr.packed_actors()
    env.reset()
    # a reset asks for charger 0 everywhere: spread the requests over the chargers and write the rows those chargers would see
    ids = (torch.arange(B, device=dev) % M).to(torch.int32)
    rows = env.entity_state(ids)
    env.nodes_feat.copy_(rows["nodes"]); env.chargers_feat.copy_(rows["chargers"]); env.env_feat.copy_(rows["env_feat"])
    g = -torch.log(-torch.log(torch.rand((B, N), dtype=torch.float32, device=dev)))
    eps = torch.randn((B,), dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def fused(timed):
        ev[0].record(); env.entity_pointer_act(ids, packed, g, eps, a.min_charge); ev[1].record()
        if not timed:
            return None
        torch.cuda.synchronize(dev)
        return ev[0].elapsed_time(ev[1])

    def loop(timed):
        torch.cuda.synchronize(dev); t0 = time.perf_counter()
        stored = torch.zeros((B, 2), dtype=torch.float32, device=dev); logp = torch.zeros((B,), dtype=torch.float32, device=dev)
        for c in range(M):
            sel = torch.nonzero(ids == c).flatten()
            if sel.numel() == 0:
                continue
            x = EntityTransitionBuffers.pack(env.nodes_feat.index_select(0, sel), env.chargers_feat.index_select(0, sel), env.env_feat.index_select(0, sel))
            act, lp = lr.get_action(c, x)
            stored.index_copy_(0, sel, act.float()); logp.index_copy_(0, sel, lp.float())
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 if timed else None

    kinds = {k: f for k, f in (("fused", fused), ("torch", loop)) if a.only in (None, k)}
    if a.only == "masked" or (a.mask_claimed and a.only is None):
        kinds["masked"] = fused
    res = {k: [] for k in kinds}
    for _ in range(a.windows):
        for kind, f in kinds.items():
            env.set_entity_pointer_mask(1 if kind == "masked" else 0)
            for _ in range(a.warmup):
                f(False)
            s = [f(True) for _ in range(a.calls)]
            res[kind].append({"median": statistics.median(s), "min": min(s), "max": max(s)})
    out = {"config": {"envs": B, "nodes": N, "chargers": M, "infer_chunk": a.infer_chunk, "windows_per_kind": a.windows, "timed_calls_per_window": a.calls,
                      "warmup_calls_per_window": a.warmup, "min_charge": a.min_charge,
                      "fused_sample": "HIP-event time around VecWRSN.entity_pointer_act, ms",
                      "torch_sample": "synchronised wall time around the per-charger get_action loop of step_batch, ms"},
           "device": torch.cuda.get_device_name(0)}
    for kind in kinds:
        w = res[kind]
        out[kind + "_ms"] = {"windows": w, "median_of_window_medians": statistics.median(x["median"] for x in w), "min": min(x["min"] for x in w),
                             "max": max(x["max"] for x in w)}
    f_ms = out["fused_ms"]["median_of_window_medians"] if "fused" in kinds else None
    if "masked" in kinds and f_ms is not None:
        out["masked_over_fused"] = out["masked_ms"]["median_of_window_medians"] / f_ms
    if a.only is None:
        out["torch_over_fused"] = out["torch_ms"]["median_of_window_medians"] / f_ms
    prior = os.path.join(ROOT, "profiles", "entity_act_bench.json")
    if f_ms is not None and os.path.exists(prior):
        with open(prior) as r:
            out["over_recorded_entity_act"] = f_ms / json.loads(r.readline())["fused_ms"]["median_of_window_medians"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as w:
            w.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
