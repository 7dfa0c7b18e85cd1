"""One minibatch step of the entity policy's PPO update at n = 64 rows, N = 200 nodes, M = 3 chargers: the fused step (wrsn_entity_ppo_grad plus
two wrsn_entity_adam) against minibatch_loss + backward + apply_gradients on the same rows and weights.  Alternating windows, 3 warm-up steps,
20 timed steps per window (synchronised wall time per step); median, minimum and maximum per window.  Writes profiles/entity_update_bench.json.
python tools/bench_entity_update.py [--windows 3] [--only fused|torch] [--out PATH]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, choices=[None, "fused", "torch"], help="one side only (a kernel trace of the fused step alone)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entity_update_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, VecWRSN, pack_entity_actor, pack_entity_critic, synth_scenario
    n, N, M, B = 64, 200, 3, 128
    torch.manual_seed(0); np.random.seed(0)
    env = VecWRSN([synth_scenario(e, N, N) for e in range(B)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
    algo = BatchedEntityIPPO(dict(batch_size=n, minibatch_size=n, n_updates_per_iteration=1), env, fused_policy=True, fused_update=True)
    batch = algo.roll_out(max_launches=200)[0]
    dev = env.device
    mb = torch.arange(n, device=dev)
    idx = mb.to(torch.int32)
    f32 = lambda x: x.to(torch.float32).contiguous()
    b = {"actions": f32(batch["actions"]), "log_probs": f32(batch["log_probs"]), "advantages": f32(batch["advantages"]), "returns": f32(batch["returns"]),
         "values": f32(batch["values"])}
    rows = f32(batch["states"])
    hyper = dict(clip=algo.clip, ent_coef=algo.ent_coef, vf_coef=algo.vf_coef, norm_adv=algo.norm_adv, clip_vloss=algo.clip_vloss)
    ba, bc = f32(pack_entity_actor(algo.actors[0])), f32(pack_entity_critic(algo.critics[0]))
    Pa, Pc = ba.numel(), bc.numel()
    grad = torch.zeros(Pa + Pc, device=dev); stats = torch.zeros(8, device=dev)
    mom = [torch.zeros(Pa, device=dev), torch.zeros(Pa, device=dev), torch.zeros(Pc, device=dev), torch.zeros(Pc, device=dev)]
    step = [0]

    def fused():
        step[0] += 1
        env.entity_ppo_grad(ba, bc, rows, idx, b, hyper, grad, stats)
        env.entity_adam(ba, grad[:Pa], mom[0], mom[1], step[0], algo.args["lr"], algo.max_grad_norm)
        env.entity_adam(bc, grad[Pa:], mom[2], mom[3], step[0], algo.args["lr"], algo.max_grad_norm)

    def eager():
        loss = algo.minibatch_loss(0, batch, mb)[0]
        algo.optimizers[0].zero_grad(); loss.backward(); algo.apply_gradients(0)

    def window(f):
        ts = []
        for _ in range(args.steps):
            torch.cuda.synchronize(dev); t0 = time.perf_counter(); f(); torch.cuda.synchronize(dev); ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}

    sides = [(k, f) for k, f in (("fused", fused), ("torch", eager)) if args.only in (None, k)]
    for _, f in sides:
        for _ in range(3): f()
    out = {"workload": "one minibatch step, n = %d rows, N = %d nodes, M = %d chargers" % (n, N, M), "device": torch.cuda.get_device_name(dev),
           "steps_per_window": args.steps, "warmup_steps": 3, "windows": {k: [] for k, _ in sides}}
    for _ in range(args.windows):
        for k, f in sides:
            out["windows"][k].append(window(f))
    for k, _ in sides:
        out[k + "_median_ms"] = float(np.median([w["median_ms"] for w in out["windows"][k]]))
    if args.only is None:
        out["speedup"] = out["torch_median_ms"] / out["fused_median_ms"]
    with open(args.out, "w") as w:
        json.dump(out, w, indent=1)
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    main()
