"""Roll-out bookkeeping on entity rows against image rows at the headline geometry: 4096 environments x 200 nodes x 200 targets x 3
chargers, G = 100, the seeded synthetic networks and random policy of bench.py, auto-reset, step_budget 1250.  ONE environment with the
image and the entity observation on, and both kinds of transition buffers; the kinds take turns in windows of the same run.  In a
window every step call is  record -> step -> collect  with the window's buffers, and the HIP-event time of the record launch plus that
of the collect launch is one sample: 3 warm-up calls, then the median, minimum and maximum of 20 calls.  The counters are cleared
before every call (outside the timed region) and the capacity defaults to the number of environments -- the most one call can return
for one charger -- so that every collect stores every transition it counts; with a smaller --capacity the excess is counted and not
copied, for both kinds alike.

    python tools/bench_entity_rollout.py [--envs 4096] [--windows 5] [--out profiles/entity_rollout_bench.json]

What would be a defect rather than a number: the entity pair slower than the image pair of the same run -- it moves about 1/24 of the
bytes."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--targets", type=int, default=200)
    ap.add_argument("--agents", type=int, default=3)
    ap.add_argument("--map-size", type=int, default=100)
    ap.add_argument("--step-budget", type=int, default=1250)
    ap.add_argument("--capacity", type=int, default=None, help="transitions per charger in both kinds of buffers (default: --envs, what one call can return at most)")
    ap.add_argument("--windows", type=int, default=5, help="windows per kind (they alternate)")
    ap.add_argument("--calls", type=int, default=20, help="timed step calls per window")
    ap.add_argument("--warmup", type=int, default=3, help="untimed step calls at the start of every window")
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    import torch
    from multi_agent_rl_wrsn_amd import EntityTransitionBuffers, TransitionBuffers, VecWRSN, synth_scenario
    B, M, G, U = a.envs, a.agents, a.map_size, 64
    a.capacity = a.capacity or B
    uniq = [synth_scenario(9000 + u, a.nodes, a.targets) for u in range(U)]
    dev = torch.device("cuda:0")
    env = VecWRSN([uniq[e % U] for e in range(B)], None, M, map_size=G, auto_reset=True, step_budget=a.step_budget, entities=True)
    bufs = {"entity": EntityTransitionBuffers(env, a.capacity, 3), "image": TransitionBuffers(env, a.capacity, 3)}
    gen = torch.Generator(device=dev).manual_seed(7)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    r = env.reset()
    stored = {k: 0 for k in bufs}

    def call(kind, timed):
        nonlocal r
        buf = bufs[kind]
        ids = r["agent_id"].clone()
        act = torch.rand((B, 3), generator=gen, device=dev, dtype=torch.float32)
        logp = torch.zeros(B, dtype=torch.float32, device=dev)
        buf.clear(keep_pending=True)
        ev[0].record(); buf.record(ids, act, logp); ev[1].record()
        r = env.step(ids, act.double())
        ev[2].record(); buf.collect(); ev[3].record()
        if not timed:
            return None
        torch.cuda.synchronize(dev)
        stored[kind] += int(buf.count.clamp(max=buf.capacity).sum())
        return ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])

    res = {k: {"record_ms": [], "collect_ms": [], "pair_ms": []} for k in bufs}
    for _ in range(a.windows):
        for kind in bufs:
            bufs[kind].clear()                                 # what the other kind's window left pending belongs to requests long gone
            for _ in range(a.warmup):
                call(kind, False)
            s = [call(kind, True) for _ in range(a.calls)]
            for name, v in (("record_ms", [x[0] for x in s]), ("collect_ms", [x[1] for x in s]), ("pair_ms", [x[0] + x[1] for x in s])):
                res[kind][name].append({"median": statistics.median(v), "min": min(v), "max": max(v)})
    out = {"config": {"envs": B, "nodes": a.nodes, "targets": a.targets, "chargers": M, "map_size": G, "step_budget": a.step_budget,
                      "capacity": a.capacity, "windows_per_kind": a.windows, "timed_calls_per_window": a.calls, "warmup_calls_per_window": a.warmup,
                      "sample": "HIP-event time of the record launch + HIP-event time of the collect launch of one step call"},
           "device": torch.cuda.get_device_name(0),
           "bytes_per_row": {"image": 4 * G * G * 4, "entity": 4 * bufs["entity"].row_elems},
           "transitions_stored_in_timed_calls": stored}
    for kind in bufs:
        out[kind] = {name: {"windows": w, "median_of_window_medians": statistics.median(x["median"] for x in w), "min": min(x["min"] for x in w),
                            "max": max(x["max"] for x in w)} for name, w in res[kind].items()}
    out["entity_pair_over_image_pair"] = out["entity"]["pair_ms"]["median_of_window_medians"] / out["image"]["pair_ms"]["median_of_window_medians"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as w:
            w.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
