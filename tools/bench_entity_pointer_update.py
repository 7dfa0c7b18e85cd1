"""The node-pointer policy's PPO update and batch preparation, new paths against the per-charger ones, at bench_ippo.py's hyper-parameters
(batch 512, minibatch 64, 5 epochs) and 200 nodes.  Three parts:
  step     one minibatch step of ONE charger at n = 64, M = 3: `entity_pointer_ppo_grad` + two `entity_adam` (device) against
           `minibatch_loss` + backward + `apply_gradients` (torch) on the same rows
  update   a whole update of every charger, M = 3 and M = 8: M `update` calls (per_charger: `DeviceUpdateDriver._update_charger`, three calls per minibatch step and
           charger) against one `update_all` (joint: one wrsn_entity_pointer_ppo_update).  Both sides include packing the modules, writing
           them back and the one read of the statistics table
  prepare  the tail of a roll-out on the SAME filled transition buffers, M = 3 and M = 8: `_prepare_batches` of the default path (default)
           against fused_prepare=True (fused).  Both sides include the host read, the selection and the upload
Alternating windows, 1 warm-up call per side, `--updates` timed calls per window (synchronised wall time per call); median, minimum and
maximum per window, and the medians of the window medians.  Writes profiles/entity_pointer_joint_bench.json.
python tools/bench_entity_pointer_update.py [--windows 3] [--updates 5] [--chargers 3 8] [--only PART_OR_SIDE] [--out PATH]
--only: a part (step, update, prepare) or one side of a part alone (device, torch; per_charger, joint; default, fused), for a kernel trace."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = {"step": ("torch", "device"), "update": ("per_charger", "joint"), "prepare": ("default", "fused")}
PPO = dict(batch_size=512, minibatch_size=64, n_updates_per_iteration=5)


def measure(sides, only, windows, calls, sync):
    """Alternating windows over the (name, function) pairs of one part; `only`: None, the part's name or one side's."""
    import numpy as np
    sides = [(k, f) for k, f in sides if only is None or only in PARTS or only == k]

    def window(f):
        ts = []
        for _ in range(calls):
            sync(); t0 = time.perf_counter(); f(); sync(); ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}

    for _, f in sides:
        f()                                                   # the warm-up call
    res = {"windows": {k: [] for k, _ in sides}}
    for _ in range(windows):
        for k, f in sides:
            res["windows"][k].append(window(f))
    for k, _ in sides:
        res[k + "_median_ms"] = float(np.median([w["median_ms"] for w in res["windows"][k]]))
    if len(sides) == 2:
        (a, _), (b, _) = sides
        res["%s_over_%s" % (a, b)] = res[a + "_median_ms"] / res[b + "_median_ms"]
    return res


def run(make_env, ppo=PPO, step_rows=64, chargers=(3, 8), windows=3, updates=5, only=None, device=None, max_launches=2000):
    """The three parts on the environments `make_env(M)` gives (a VecWRSN with entities=True, or the tests' emulated stand-in); `device`:
    what the trainers are given (None: the environment's).  Returns the result dict."""
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityPointerIPPO, pack_entity_critic, pack_entity_pointer_actor
    want = lambda part: only is None or only == part or only in PARTS[part]
    out = {"workload": "node-pointer policy: batch %d, minibatch %d, %d epochs; one minibatch step at n = %d" % (
        ppo["batch_size"], ppo["minibatch_size"], ppo["n_updates_per_iteration"], step_rows), "calls_per_window": updates, "warmup_calls": 1,
        "chargers": {}}
    for M in chargers:
        torch.manual_seed(0); np.random.seed(0)
        env = make_env(M)
        dev = env.device
        on_gpu = getattr(dev, "type", "cpu") == "cuda"
        sync = (lambda: torch.cuda.synchronize(dev)) if on_gpu else (lambda: None)      # the emulated calls are synchronous
        if on_gpu:
            out["device"] = torch.cuda.get_device_name(dev)
        kw = dict(device=device, fused_policy=True, device_update=True)
        per = BatchedEntityPointerIPPO(ppo, env, **kw)
        joint = BatchedEntityPointerIPPO(ppo, env, joint_update=True, **kw)
        fused = BatchedEntityPointerIPPO(ppo, env, joint_update=True, fused_prepare=True, **kw)
        batches = per.roll_out(max_launches=max_launches)
        res = {"stored_per_charger": per.buffers.stored()}
        if M == chargers[0] and want("step"):                 # ---- (a) one minibatch step of charger 0
            plain = BatchedEntityPointerIPPO(ppo, env, device=device, fused_policy=True)
            b0 = batches[0]
            n = min(step_rows, ppo["batch_size"])
            f32 = lambda x: x.to(device=dev, dtype=torch.float32).contiguous()
            blk_a, blk_c = f32(pack_entity_pointer_actor(per.actors[0])), f32(pack_entity_critic(per.critics[0]))
            rows = f32(b0["states"])
            bb = {"actions": f32(b0["actions"]).reshape(-1, 2), "log_probs": f32(b0["log_probs"]), "advantages": f32(b0["advantages"]),
                  "returns": f32(b0["returns"]), "values": f32(b0["values"])}
            hyper = dict(clip=per.clip, ent_coef=per.ent_coef, vf_coef=per.vf_coef, norm_adv=per.norm_adv, clip_vloss=per.clip_vloss)
            idx = torch.arange(n, dtype=torch.int32, device=dev)
            mb = torch.arange(n, dtype=torch.long, device=b0["states"].device)
            st, table = per._adam[0], torch.zeros(8, dtype=torch.float32, device=dev)
            step = [0]

            def step_device():
                env.entity_pointer_ppo_grad(blk_a, blk_c, rows, idx, bb, hyper, per._grad, table)
                step[0] += 1
                env.entity_adam(blk_a, per._grad[:per._pa], st["m_a"], st["v_a"], step[0], per.args["lr"], per.max_grad_norm)
                env.entity_adam(blk_c, per._grad[per._pa:], st["m_c"], st["v_c"], step[0], per.args["lr"], per.max_grad_norm)

            def step_torch():
                loss = plain.minibatch_loss(0, b0, mb)[0]
                plain.optimizers[0].zero_grad()
                loss.backward()
                plain.apply_gradients(0)

            out["step"] = dict(measure([("torch", step_torch), ("device", step_device)], only, windows, updates, sync), rows=n, chargers=M)
            for k in ("m_a", "v_a", "m_c", "v_c"):
                st[k].zero_()                                 # the update part starts from fresh moments on both sides
        if want("update"):                                    # ---- (b) a whole update of every charger

            def per_charger():
                for a in range(M):
                    per.update(a, batches[a])

            res["update"] = measure([("per_charger", per_charger), ("joint", lambda: joint.update_all(batches))], only, windows, updates, sync)
        if want("prepare"):                                   # ---- (c) the roll-out tail on the same filled buffers
            fused.buffers = per.buffers
            res["prepare"] = measure([("default", per._prepare_batches), ("fused", fused._prepare_batches)], only, windows, updates, sync)
        out["chargers"][str(M)] = res
        if on_gpu:
            env.close()                                       # an emulated stand-in is closed by whoever made it
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--chargers", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--only", default=None, choices=[None] + list(PARTS) + [s for v in PARTS.values() for s in v],
                    help="one part, or one side of a part alone (a kernel trace of that side)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entity_pointer_joint_bench.json"))
    args = ap.parse_args()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    N, B = 200, args.envs
    make_env = lambda M: VecWRSN([synth_scenario(e, N, N) for e in range(B)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
    out = run(make_env, chargers=tuple(args.chargers), windows=args.windows, updates=args.updates, only=args.only)
    out["nodes"], out["envs"] = N, B
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as w:
        json.dump(out, w, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
