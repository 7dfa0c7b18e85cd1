"""A whole PPO update of every charger's entity policy, joint against per-charger, at bench_ippo.py's hyper-parameters (batch 512, minibatch 64,
5 epochs) and 200 nodes, for M = 3 and M = 8 chargers: `BatchedEntityIPPO.update_all` (one wrsn_entity_ppo_update for all chargers) against M
`update` calls (`DeviceUpdateDriver._update_charger`: three calls per minibatch step and charger) on the same batches.  Both sides include packing the modules,
writing them back and the one read of the statistics table.  Alternating windows, 1 warm-up update per side, `--updates` timed updates per window
(synchronised wall time per update); median, minimum and maximum per window, and the medians of the window medians.  Writes
profiles/entity_update_joint_bench.json.
python tools/bench_entity_update_joint.py [--windows 3] [--updates 5] [--chargers 3 8] [--only joint|per_charger] [--out PATH]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--chargers", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--only", default=None, choices=[None, "joint", "per_charger"], help="one side only (a kernel trace of that side alone)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entity_update_joint_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, VecWRSN, synth_scenario
    N, B = 200, args.envs
    ppo = dict(batch_size=512, minibatch_size=64, n_updates_per_iteration=5)
    out = {"workload": "one PPO update of every charger: batch %d, minibatch %d, %d epochs, N = %d nodes" % (
        ppo["batch_size"], ppo["minibatch_size"], ppo["n_updates_per_iteration"], N), "updates_per_window": args.updates, "warmup_updates": 1,
        "chargers": {}}
    for M in args.chargers:
        torch.manual_seed(0); np.random.seed(0)
        env = VecWRSN([synth_scenario(e, N, N) for e in range(B)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
        dev = env.device
        out["device"] = torch.cuda.get_device_name(dev)
        per = BatchedEntityIPPO(ppo, env, fused_policy=True, fused_update=True)
        joint = BatchedEntityIPPO(ppo, env, fused_policy=True, fused_update=True, joint_update=True)
        batches = per.roll_out(max_launches=2000)

        def per_charger():
            for a in range(M):
                per.update(a, batches[a])

        def joint_all():
            joint.update_all(batches)

        def window(f):
            ts = []
            for _ in range(args.updates):
                torch.cuda.synchronize(dev); t0 = time.perf_counter(); f(); torch.cuda.synchronize(dev); ts.append((time.perf_counter() - t0) * 1e3)
            return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}

        sides = [(k, f) for k, f in (("per_charger", per_charger), ("joint", joint_all)) if args.only in (None, k)]
        for _, f in sides:
            f()
        res = {"windows": {k: [] for k, _ in sides}}
        for _ in range(args.windows):
            for k, f in sides:
                res["windows"][k].append(window(f))
        for k, _ in sides:
            res[k + "_median_ms"] = float(np.median([w["median_ms"] for w in res["windows"][k]]))
        if args.only is None:
            res["per_charger_over_joint"] = res["per_charger_median_ms"] / res["joint_median_ms"]
        out["chargers"][str(M)] = res
        env.close()
    with open(args.out, "w") as w:
        json.dump(out, w, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
