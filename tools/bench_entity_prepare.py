"""The preparation tail of a roll-out alone -- selection, gathers, values, GAE of every charger's batch -- at bench_ippo.py's shapes (batch 512,
N = 200 nodes) for M = 3 and M = 8 chargers: `BatchedEntityIPPO._prepare_batches` with fused_prepare=True (one host read, the selection, one
upload, one wrsn_entity_prepare) against the per-charger path (fused_prepare=False: select_batch on a host copy, six index_selects, two
wrsn_entity_eval passes and the reference's GAE loop per charger) on the SAME filled transition buffers.  Both sides include the host
read, the selection and the upload.  Alternating windows, 1 warm-up call per side, `--calls` timed calls per window (synchronised wall time per
call); median, minimum and maximum per window, and the medians of the window medians.  Writes profiles/entity_prepare_bench.json.
python tools/bench_entity_prepare.py [--windows 3] [--calls 5] [--chargers 3 8] [--only fused|per_charger] [--out PATH]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--chargers", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--only", default=None, choices=[None, "fused", "per_charger"], help="one side only (a kernel trace of that side alone)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entity_prepare_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, VecWRSN, synth_scenario
    N, B = 200, args.envs
    ppo = dict(batch_size=512, minibatch_size=64, n_updates_per_iteration=5)
    out = {"workload": "the preparation tail of one roll-out for every charger: batch %d, N = %d nodes" % (ppo["batch_size"], N),
           "calls_per_window": args.calls, "warmup_calls": 1, "chargers": {}}
    for M in args.chargers:
        torch.manual_seed(0); np.random.seed(0)
        env = VecWRSN([synth_scenario(e, N, N) for e in range(B)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
        dev = env.device
        out["device"] = torch.cuda.get_device_name(dev)
        kw = dict(fused_policy=True, fused_update=True, joint_update=True)
        per = BatchedEntityIPPO(ppo, env, **kw)
        fused = BatchedEntityIPPO(ppo, env, fused_prepare=True, **kw)
        per.roll_out(max_launches=2000)
        fused.buffers = per.buffers                           # the same filled buffers
        stored = per.buffers.stored()

        def window(f):
            ts = []
            for _ in range(args.calls):
                torch.cuda.synchronize(dev); t0 = time.perf_counter(); f(); torch.cuda.synchronize(dev); ts.append((time.perf_counter() - t0) * 1e3)
            return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}

        sides = [(k, f) for k, f in (("per_charger", per._prepare_batches), ("fused", fused._prepare_batches)) if args.only in (None, k)]
        for _, f in sides:
            f()
        res = {"stored_per_charger": stored, "windows": {k: [] for k, _ in sides}}
        for _ in range(args.windows):
            for k, f in sides:
                res["windows"][k].append(window(f))
        for k, _ in sides:
            res[k + "_median_ms"] = float(np.median([w["median_ms"] for w in res["windows"][k]]))
        if args.only is None:
            res["per_charger_over_fused"] = res["per_charger_median_ms"] / res["fused_median_ms"]
        out["chargers"][str(M)] = res
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as w:
        json.dump(out, w, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
