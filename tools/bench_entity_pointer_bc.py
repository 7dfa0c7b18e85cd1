"""One behaviour-cloning update of every charger's node-pointer actor at 4096 environments x 200 nodes x 3 chargers with bench_ippo.py's
batch sizes (batch 512, minibatch 64, 5 epochs: 40 Adam steps per charger): `entity_pointer_bc_update` (wrsn_entity_pointer_bc_update, one
call for all chargers) against the float32 PyTorch autograd loop of the same loss, -mean(logp) - ent_coef * mean(H), with
clip_grad_norm_ and torch.optim.Adam per charger, on the same rows and labels (one `pretrain` collection with beta = 1).

HIP-event time of a whole update, alternating windows, medians of window medians, ONE PROCESS PER KIND (`--only device|torch` is what the
parent starts; without it this script starts both children in turn and merges what they print).  Writes
profiles/entity_pointer_bc_bench.json.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/bench_entity_pointer_bc.py --only device --windows 1
python tools/bench_entity_pointer_bc.py [--windows 3] [--updates 5] [--envs 4096] [--only device|torch] [--out PATH]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PPO = dict(batch_size=512, minibatch_size=64, n_updates_per_iteration=5)


def one_kind(args):
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO, VecWRSN, synth_scenario
    N, M = 200, 3
    torch.manual_seed(0); np.random.seed(0)
    env = VecWRSN([synth_scenario(e, N, N) for e in range(args.envs)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
    dev = env.device
    algo = BatchedEntityPointerIPPO(PPO, env, capacity=4096, fused_policy=True, device_update=True)
    algo._check_status = False
    stats = algo.pretrain(1, beta=1.0)                         # fills the buffers with the heuristic's labels (and is the warm-up of the device side)
    bs, mb, epochs = PPO["batch_size"], PPO["minibatch_size"], PPO["n_updates_per_iteration"]
    steps = epochs * (bs // mb)
    rows = [algo.buffers.state[a, :bs].clone() for a in range(M)]
    stored = [algo.buffers.action[a, :bs].clone() for a in range(M)]
    idx = torch.from_numpy(np.stack([np.stack([np.random.permutation(bs) for _ in range(epochs)]) for _ in range(M)]).astype(np.int32)).to(dev)
    lr, max_norm = algo.args["lr"], algo.max_grad_norm

    if args.only == "device":
        blocks = algo.packed_actors().contiguous()
        table = torch.zeros((M, steps, 8), dtype=torch.float32, device=dev)
        groups = [dict(actor=blocks[a], grad=algo._grad_all[a], rows=rows[a], stored=stored[a], m_a=algo._adam[a]["m_a"], v_a=algo._adam[a]["v_a"],
                       step=algo._adam[a]["step"]) for a in range(M)]

        def update():
            env.entity_pointer_bc_update(groups, idx, mb, 0.0, table, lr, max_norm)
            for g in groups:
                g["step"] += steps
    else:
        opts = [torch.optim.Adam(a.parameters(), lr=lr, eps=1e-8) for a in algo.actors]
        lidx = idx.long()

        def update():
            for a in range(M):
                for e in range(epochs):
                    for s in range(0, bs, mb):
                        sel = lidx[a, e, s:s + mb]
                        st = stored[a].index_select(0, sel)
                        logp, ent = algo.actors[a](rows[a].index_select(0, sel), st[:, 0], st[:, 1])
                        loss = -logp.mean() - 0.0 * ent.mean()
                        opts[a].zero_grad(); loss.backward()
                        torch.nn.utils.clip_grad_norm_(algo.actors[a].parameters(), max_norm)
                        opts[a].step()

    update()                                                   # the warm-up call
    windows = []
    for _ in range(args.windows):
        ts = []
        for _ in range(args.updates):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev); t0.record(); update(); t1.record(); torch.cuda.synchronize(dev)
            ts.append(t0.elapsed_time(t1))
        windows.append({"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))})
    out = {"kind": args.only, "device": torch.cuda.get_device_name(dev), "windows": windows,
           "median_ms": float(np.median([w["median_ms"] for w in windows])), "adam_steps_per_charger": steps,
           "first_collection": {"top1": [r["first"][5] for r in stats], "loss": [r["first"][0] for r in stats]}}
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--only", default=None, choices=[None, "device", "torch"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entity_pointer_bc_bench.json"))
    args = ap.parse_args()
    if args.only is not None:
        print("RESULT " + json.dumps(one_kind(args)), flush=True)
        return
    # the parent never opens the GPU: one fresh child per kind and window set, alternating kinds
    kinds = {"device": [], "torch": []}
    meta = {}
    for _ in range(args.windows):
        for k in kinds:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", k, "--windows", "1", "--updates", str(args.updates), "--envs",
                                str(args.envs)], capture_output=True, text=True, check=True)
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            kinds[k].extend(res["windows"]); meta = res
    import statistics
    out = {"workload": "one behaviour-cloning update of 3 chargers: batch %d, minibatch %d, %d epochs, %d envs x 200 nodes; HIP-event time of the "
                       "whole update" % (PPO["batch_size"], PPO["minibatch_size"], PPO["n_updates_per_iteration"], args.envs),
           "device": meta.get("device"), "updates_per_window": args.updates, "warmup_calls": 1, "windows": kinds,
           "adam_steps_per_charger": meta.get("adam_steps_per_charger")}
    for k, w in kinds.items():
        out[k + "_median_ms"] = statistics.median(x["median_ms"] for x in w)
    out["torch_over_device"] = out["torch_median_ms"] / out["device_median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as w:
        json.dump(out, w, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
