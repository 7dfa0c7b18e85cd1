"""bench_ippo.py -- BASELINE.json configs[2]: 4096 environments x 200 nodes x 3 chargers, IPPO (alg_args/ippo.yaml) roll-out + train
on one MI355X, environment time and policy time reported separately (SURVEY.md 8d "Config 3/4 note": the roll-out is
policy-bound -- the UNet forward is ~5 GFLOP per decision against ~1e-3 GFLOP-equivalents of environment work).

    python bench_ippo.py [--iters 1] [--envs 4096] [--batch-size 512]

Prints ONE JSON line: per training iteration the wall time split into environment launches (VecWRSN.step incl. the
observation), policy inference (UNet forward + sampling for every environment that carries a request), roll-out glue
(transition buffers, density map -> action) and the PPO update; env-steps/s of the roll-out alone and with training.
`python bench.py` stays the headline (random policy) measurement.

`python bench_ippo.py --gpus N` (BASELINE configs[3]: N = 8, 8 x 4096 environments) starts the N ranks itself; under torchrun
(`python -m torch.distributed.run --nproc-per-node N bench_ippo.py --gpus N`) it joins the launcher's group.  Every rank rolls out its own environment shard, the actor / critic gradients are averaged with one RCCL all-reduce per minibatch
(`PPOLearner`), the roll-out returns table is all-gathered once per run, and rank 0 prints the line with whole-job totals."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one per GPU); without a launcher (WORLD_SIZE unset) this process starts them itself")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup-iters", type=int, default=1, help="untimed iterations first (MIOpen kernel search for every new convolution shape)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--minibatch-size", type=int, default=64)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--step-budget", type=int, default=1250)
    ap.add_argument("--infer-chunk", type=int, default=512)
    ap.add_argument("--inference-dtype", default=None, choices=[None, "bf16", "fp16"], help="reduced-precision roll-out inference (update stays float32)")
    ap.add_argument("--obs-dtype", default="float32", choices=["float32", "bfloat16"], help="observation format of the environment and the roll-out buffers")
    ap.add_argument("--policy", default="image", choices=["image", "entity", "pointer"], help="image: UNet / CNN critic on the 4 x G x G observation (default); "
                    "entity: the set policy on entity rows, no image rendered (VecWRSN(render=False, entities=True), BatchedEntityIPPO); "
                    "pointer: the node-pointer policy on the same rows (BatchedEntityPointerIPPO; --fused-policy: wrsn_entity_pointer_act)")
    ap.add_argument("--fused-policy", action="store_true", help="with --policy entity: the device samples the actions itself (wrsn_entity_act, "
                    "BatchedEntityIPPO(fused_policy=True)) instead of one PyTorch forward pass per charger")
    ap.add_argument("--fused-update", action="store_true", help="with --policy entity: the PPO update runs on the device (wrsn_entity_ppo_grad, "
                    "wrsn_entity_adam, BatchedEntityIPPO(fused_update=True)) instead of PyTorch autograd and torch.optim.Adam")
    ap.add_argument("--joint-update", action="store_true", help="implies --fused-update: every charger's update goes through the same launches behind "
                    "one call (wrsn_entity_ppo_update, BatchedEntityIPPO(joint_update=True)); with --policy pointer it implies --device-update "
                    "(wrsn_entity_pointer_ppo_update, BatchedEntityPointerIPPO(joint_update=True))")
    ap.add_argument("--fused-prepare", action="store_true", help="implies --fused-update: values, GAE and the gathers of every charger's batch in one device "
                    "call (wrsn_entity_prepare, BatchedEntityIPPO(fused_prepare=True)) instead of index_select and cal_rt_adv per charger; with --policy pointer "
                    "it implies --device-update (BatchedEntityPointerIPPO(fused_prepare=True))")
    ap.add_argument("--device-update", action="store_true", help="with --policy pointer: the PPO update runs on the device (wrsn_entity_pointer_ppo_grad, "
                    "wrsn_entity_adam, BatchedEntityPointerIPPO(device_update=True)) instead of PyTorch autograd and torch.optim.Adam")
    ap.add_argument("--min-charge", type=float, default=0.02, help="with --policy pointer: the least third component of an action "
                    "(BatchedEntityPointerIPPO(min_charge=...))")
    ap.add_argument("--mask-claimed", action="store_true", help="with --policy pointer: the actors choose among the nodes no other charger serves "
                    "(wrsn_set_entity_pointer_mask, BatchedEntityPointerIPPO(mask_claimed=True))")
    ap.add_argument("--report-updates", action="store_true", help="add peak device memory and the statistics of every update (first minibatch included) to the line")
    args = ap.parse_args()
    if args.joint_update or args.fused_prepare:
        if args.policy == "pointer":
            args.device_update = True
        else:
            args.fused_update = True
    if args.fused_policy and args.policy not in ("entity", "pointer"):
        raise SystemExit("--fused-policy needs --policy entity or --policy pointer")
    if args.fused_update and args.policy != "entity":
        raise SystemExit("--fused-update needs --policy entity")
    if args.device_update and args.policy != "pointer":
        raise SystemExit("--device-update needs --policy pointer")
    if args.mask_claimed and args.policy != "pointer":
        raise SystemExit("--mask-claimed needs --policy pointer")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:       # launcher-free multi-rank entry: before this process touches torch or the GPU
        from multi_agent_rl_wrsn_amd.sharding import launch_ranks
        raise SystemExit(launch_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, BatchedEntityPointerIPPO, BatchedIPPO, RolloutStats, VecWRSN, init_distributed, synth_scenario
    rank, world, local_rank = init_distributed()
    if world != args.gpus and not (args.gpus == 1 and "WORLD_SIZE" in os.environ):      # torchrun without --gpus: WORLD_SIZE rules
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    dist = torch.distributed if world > 1 else None
    if dist:                                                   # the RCCL group the ranks really formed
        one = torch.ones(1, dtype=torch.float64, device=torch.device("cuda", local_rank)); dist.all_reduce(one)
        if int(one[0]) != world or dist.get_backend() != "nccl":
            raise SystemExit("process group has %d ranks on backend %s, expected %d on nccl" % (int(one[0]), dist.get_backend(), world))
    torch.manual_seed(0); np.random.seed(rank)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    B, N, M = args.envs, args.nodes, 3
    entity, pointer = args.policy == "entity", args.policy == "pointer"
    updates = []                                               # --report-updates: every row train() logs, with the first minibatch's statistics
    ppo_args = dict(batch_size=args.batch_size, minibatch_size=args.minibatch_size, n_updates_per_iteration=args.updates)
    if pointer:
        env = VecWRSN([synth_scenario(rank * B + e, N, N) for e in range(B)], None, M, auto_reset=True, step_budget=args.step_budget, device=str(dev),
                      render=False, entities=True)
        algo = BatchedEntityPointerIPPO(ppo_args, env, capacity=max(2 * args.batch_size, 4096), infer_chunk=args.infer_chunk, min_bucket=args.infer_chunk,
                                        fused_policy=args.fused_policy, min_charge=args.min_charge,
                                        **({"device_update": True} if args.device_update else {}), **({"joint_update": True} if args.joint_update else {}),
                                        **({"fused_prepare": True} if args.fused_prepare else {}), **({"mask_claimed": True} if args.mask_claimed else {}))
    elif entity:
        env = VecWRSN([synth_scenario(rank * B + e, N, N) for e in range(B)], None, M, auto_reset=True, step_budget=args.step_budget, device=str(dev),
                      render=False, entities=True)             # no image at all: 6.6 KB of entity rows per request
        algo = BatchedEntityIPPO(ppo_args, env, capacity=max(2 * args.batch_size, 4096), infer_chunk=args.infer_chunk, min_bucket=args.infer_chunk,
                                 **({"fused_policy": True} if args.fused_policy else {}), **({"fused_update": True} if args.fused_update else {}),
                                 **({"joint_update": True} if args.joint_update else {}), **({"fused_prepare": True} if args.fused_prepare else {}))
    else:
        env = VecWRSN([synth_scenario(rank * B + e, N, N) for e in range(B)], None, M, auto_reset=True, step_budget=args.step_budget, device=str(dev),
                      reuse_obs=True, obs_dtype=args.obs_dtype)                             # BatchedIPPO only reads the state tensor (index_select / copies)
        algo = BatchedIPPO(ppo_args, env,
                           capacity=max(2 * args.batch_size, 4096), infer_chunk=args.infer_chunk, inference_dtype=args.inference_dtype,
                           min_bucket=args.infer_chunk)           # ONE batch shape for every inference pass: MIOpen searches its convolution kernels per shape (seconds each)
    if args.report_updates:                                    # the statistics of the first minibatch of every update: the weights the roll-out ran with
        first, inner = {}, algo.minibatch_loss

        def minibatch_loss(id, batch, mb):
            res = inner(id, batch, mb)
            first.setdefault(id, dict(approx_kl=float(res[4]), clipfrac=float(res[5])))
            return res
        algo.minibatch_loss = minibatch_loss
        algo.log = lambda row: updates.append(dict(row, first_minibatch=first.pop(row["agent"], {})))
        if args.fused_update or args.device_update:            # no minibatch_loss is called: the device table's first row
            algo.log = lambda row: updates.append(dict(row, first_minibatch=dict(approx_kl=algo.first_minibatch_stats[row["agent"]][4],
                                                                                 clipfrac=algo.first_minibatch_stats[row["agent"]][5])))
    if args.warmup_iters > 0:
        algo.train(args.warmup_iters - 1)
        for k in algo.timers: algo.timers[k] = 0 if isinstance(algo.timers[k], int) else 0.0
        del updates[:]
    torch.cuda.synchronize(dev)
    if args.report_updates:
        torch.cuda.reset_peak_memory_stats(dev)
    c0 = env.counters(); t0 = time.perf_counter()
    rows = algo.train(args.iters - 1)                          # train() runs iterations 0..n inclusive like the reference's loop (IPPO.py:220)
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0
    c1 = env.counters(); t = algo.timers; it = args.iters
    steps = c1["env_steps"] - c0["env_steps"]
    table = RolloutStats.gather_table(env.rollout_table())     # the one exchange of the environment path (RCCL all-gather)
    if dist:
        tot = torch.tensor([steps], dtype=torch.float64, device=dev); dist.all_reduce(tot); steps_all = float(tot[0])
        wl = torch.tensor([wall], dtype=torch.float64, device=dev); dist.all_reduce(wl, op=dist.ReduceOp.MAX); wall = float(wl[0])
    else:
        steps_all = float(steps)
    if rank != 0:
        if dist: dist.destroy_process_group()
        return
    out = {"metric": "IPPO roll-out + train, 4096 envs/GPU x 200 nodes x 3 MC (BASELINE configs[2]; configs[3] under torchrun)", "n_gpus": world,
           "returns_table_rows": int(table.shape[0]), "env_steps_all_ranks": steps_all, "env_steps_per_s_with_training_all_ranks": steps_all / wall, "iterations": it, "warmup_iterations": args.warmup_iters,
           "config": {"workload": "%d envs x %d nodes x %d MC, UNet actor + CNN critic per charger, density-map actions, batch %d / minibatch %d / %d epochs" %
                      (B, N, M, args.batch_size, args.minibatch_size, args.updates), "step_budget": args.step_budget, "obs_dtype": args.obs_dtype,
                      "policy": "float32, channels-last%s" % ("" if not args.inference_dtype else ", %s roll-out inference" % args.inference_dtype)},
           "per_iteration_s": {"environment": t["env_s"] / it, "policy_inference": t["policy_s"] / it, "rollout_glue": t["glue_s"] / it, "batch_preparation": t["prepare_s"] / it, "ppo_update": t["train_s"] / it,
                               "wall": wall / it},
           "launches_per_iteration": t["launches"] / it, "requests_served": t["requests"], "env_steps": steps,
           "env_steps_per_s_environment_only": steps / max(t["env_s"], 1e-9), "env_steps_per_s_rollout": steps / max(t["env_s"] + t["policy_s"] + t["glue_s"], 1e-9),
           "env_steps_per_s_with_training": steps / wall, "transitions_per_agent": algo.buffers.counts(),
           "last_rows": rows[-M:], "dtype": "f32 policy / f64 physics", "data": "synthetic"}
    if entity:
        out["config"]["workload"] = "%d envs x %d nodes x %d MC, set actor + critic per charger on entity rows, 3-vector actions, batch %d / minibatch %d / %d epochs" % (
            B, N, M, args.batch_size, args.minibatch_size, args.updates)
        out["config"]["policy"] = "float32, entity rows, no image" + (", actions sampled on the device (wrsn_entity_act)" if args.fused_policy else "") + (
            ", update on the device (wrsn_entity_ppo_grad, wrsn_entity_adam)" if args.fused_update else "") + (
            ", every charger in one call (wrsn_entity_ppo_update)" if args.joint_update else "") + (
            ", batch prepared on the device (wrsn_entity_prepare)" if args.fused_prepare else "")
    if pointer:
        out["config"]["workload"] = "%d envs x %d nodes x %d MC, node-pointer actor + set critic per charger on entity rows, (node, x) actions, batch %d / minibatch %d / %d epochs" % (
            B, N, M, args.batch_size, args.minibatch_size, args.updates)
        out["config"]["policy"] = "float32, entity rows, no image" + (", actions sampled on the device (wrsn_entity_pointer_act)" if args.fused_policy else "") + (
            ", update on the device (wrsn_entity_pointer_ppo_grad, wrsn_entity_adam)" if args.device_update else "") + (
            ", every charger in one call (wrsn_entity_pointer_ppo_update)" if args.joint_update else "") + (
            ", batch prepared on the device (wrsn_entity_prepare)" if args.fused_prepare else "") + (
            ", candidate mask on (wrsn_set_entity_pointer_mask)" if args.mask_claimed else "")
    if args.report_updates:
        out["peak_memory_bytes"] = int(torch.cuda.max_memory_allocated(dev)); out["updates"] = updates
    print(json.dumps(out, default=float), flush=True)
    if dist: dist.destroy_process_group()


if __name__ == "__main__":
    main()
