"""Whole-episode evaluation of the entity policy against its baselines, and the cost of the episode ledger.

Default mode: `evaluate_policy` on a HELD-OUT set -- `--eval-envs` (256) synthetic 200-node networks whose seeds the trainer never sees --
for: uniform actions, the heuristic (`HeuristicPolicy`, as the kernel's rule stands and with `--min-charge`), the untrained actors (mode
and sampled) and the actors after `--iters` (200) iterations of BatchedEntityIPPO with the fused options of bench_ippo.py (mode and
sampled).  `--policy pointer` does the same for the node-pointer policy: uniform and heuristic as above, then the untrained pointer
actors (mode and sampled) and the actors after `--iters` iterations of BatchedEntityPointerIPPO (fused acting, the PyTorch update; mode
and sampled), every pointer row with `--min-charge`; it writes profiles/entity_pointer_eval.json.  A policy that uses up `--max-launches` is recorded with its partial log and the number of environments standing still (a
deterministic policy that repeats an action of zero duration gets the same request again at the same instant).  Writes
profiles/entity_eval.json.
`--policy pointer --mask-claimed` runs every pointer row twice in the same run -- without the candidate mask (the names above) and with it
(`masked_...`; `wrsn_set_entity_pointer_mask`, BatchedEntityPointerIPPO(mask_claimed=True)) --, each trainer on a training batch of its
own from the same seeds and with the same flags (`--device-update --joint-update --fused-prepare` choose the update; acting is always
fused), and writes profiles/entity_pointer_mask_eval.json.
`--policy pointer --device-update --pretrain N [--beta B] [--beta-end B] [--critic-iters K]` adds, in the same run and from the same seeds,
the heuristic acted out as its pointer label (`heuristic_as_label`, HeuristicLabelPolicy) and a second trainer on a training batch of its
own: the pointer after N iterations of `BatchedEntityPointerIPPO.pretrain` alone (`bc_mode`, `bc_sampled`) and after `--iters` PPO
iterations on top (`bc_ppo_mode`, `bc_ppo_sampled`), next to the PPO-only rows (`trained_...`); with `--mask-claimed` all of them once
more under the mask (`masked_...`).  The cloning statistics of every iteration are kept as a compact table (`pretrain_table`): loss and
top-1 of the device table's first and last row per charger, the loss parts and the entropy of its last row.  Writes profiles/entity_pointer_bc_eval.json.

`--lookahead K [--lookahead K ...] [--horizon T ...]`: the lookahead expert against the heuristic it improves on, in one run on the held-out
set: `heuristic_min_charge`, then `LookaheadPolicy(K, horizon)` for every K and horizon (default horizons: 1, 3 and 10 times the
heuristic's mean interval between requests in this run, lifetime / decisions from its own ledger) on a simulation batch of K * eval-envs
environments.  Per row: the lifetime summary, the share of decisions with choice != 0 and which key decided them (a longer survival, or
the return at equal survival), launches of the simulation batch per real launch and wall time per real launch against the heuristic's.
Writes profiles/lookahead_eval.json.

--bench: the evaluation loop per launch at `--envs` (4096) x 200 nodes x 3 chargers with the heuristic policy, in two forms: with
wrsn_episodes_collect, and with the same bookkeeping in elementwise torch on calls that existed before it (`step`, `reset(mask)`).
Alternating windows of `--launches` launches (synchronised wall time of a window / launches), medians of the window medians.  Writes
profiles/episodes_bench.json.  `--only fused|torch` runs one form (for a kernel trace).
python tools/eval_entity_policy.py [--iters 200] [--episodes 1] [--bench] [--windows 3] [--only fused]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_loop(env, policy, episodes, time_limit, park=True):
    """The bookkeeping of the ledger in elementwise torch: a generator that performs one launch per next().  park=False: `episodes`
    slots are stored, later episodes only counted, nothing is parked (the ledger's quota 0)."""
    t = env.torch
    B, M, E = env.num_env, env.num_agent, episodes
    z = lambda shape, dt: t.zeros(shape, dtype=dt, device=env.device)
    run_ret, run_dec, finished = z((B, M), t.float64), z((B, M), t.int32), z((B,), t.int64)
    life, ep_ret, dec, ended = z((E, B), t.float64), z((E, B, M), t.float64), z((E, B, M), t.int32), z((E, B), t.int32)
    ar = t.arange(B, device=env.device)
    ids = env.reset()["agent_id"].clone()
    while True:
        r = env.step(ids, policy(env, ids))
        agent, status, now, reward, terminal = r["agent_id"], r["status"], r["now"], r["reward"], r["terminal"]
        stepped = ids != -2
        flying = stepped & (status == 4)
        term = stepped & ~flying & (terminal != 0)
        fresh = stepped & ~flying & (terminal == 0)
        hot = (t.nn.functional.one_hot(agent.clamp(0, M - 1).long(), M) * (fresh & (agent >= 0) & (agent < M))[:, None])
        run_ret += hot * reward[:, None]; run_dec += hot.int()
        code = t.where(term, 1, t.where(fresh & (status == 1), 3, t.where(fresh & (now >= time_limit), 2, 0)))
        closing = (code > 0) & (finished < E)
        k = finished.clamp(max=E - 1)
        life[k, ar] = t.where(closing, now, life[k, ar]); ended[k, ar] = t.where(closing, code.int(), ended[k, ar])
        ep_ret[k, ar] = t.where(closing[:, None], run_ret, ep_ret[k, ar]); dec[k, ar] = t.where(closing[:, None], run_dec, dec[k, ar])
        finished += (code > 0)
        keep = (code == 0)[:, None]
        run_ret *= keep; run_dec *= keep
        restart = (code > 0) & ((finished < E) if park else (finished >= 0))
        ids = t.where(code > 0, -2, t.where(flying, -1, t.where(fresh, agent, ids))).int()
        r = env.reset(mask=restart.to(t.uint8))
        ids = t.where(restart, r["agent_id"], ids).int().contiguous()
        yield finished


def ledger_loop(env, policy, episodes, time_limit, park=True):
    log = env.new_episode_log(episodes, quota=episodes if park else 0)
    env.reset()
    ids, restart = env.episodes_collect(log, time_limit)
    while True:
        env.step(ids, policy(env, ids))
        ids, restart = env.episodes_collect(log, time_limit)
        env.reset(mask=restart)
        ids, restart = env.episodes_collect(log, time_limit)
        yield log.finished


def bench(args):
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import HeuristicPolicy, VecWRSN, synth_scenario
    N, M = 200, 3
    scs = [synth_scenario(e, N, N) for e in range(args.envs)]
    tl = min(s.max_time for s in scs)
    forms = [(k, f) for k, f in (("fused", ledger_loop), ("torch", torch_loop)) if args.only in (None, k)]
    envs = {k: VecWRSN(scs, None, M, render=False, entities=True, step_budget=1250) for k, _ in forms}
    pol = HeuristicPolicy(min_charge=args.min_charge)
    loops = {k: f(envs[k], pol, 8, tl, park=False) for k, f in forms}   # nothing parks: every launch steps every environment
    dev = envs[forms[0][0]].device
    out = {"workload": "evaluation loop, %d envs x %d nodes x %d chargers, heuristic policy (min_charge %g), step budget 1250" % (args.envs, N, M, args.min_charge),
           "device": torch.cuda.get_device_name(dev), "launches_per_window": args.launches, "windows": {k: [] for k, _ in forms}}
    for k, _ in forms:
        for _ in range(10):
            next(loops[k])
    for _ in range(args.windows):
        for k, _ in forms:
            torch.cuda.synchronize(dev); t0 = time.perf_counter()
            for _ in range(args.launches):
                next(loops[k])
            torch.cuda.synchronize(dev)
            out["windows"][k].append((time.perf_counter() - t0) * 1e3 / args.launches)
    for k, _ in forms:
        w = out["windows"][k]
        out[k + "_ms_per_launch"] = float(np.median(w)); out[k + "_spread_ms"] = float(max(w) - min(w))
    if args.only is None:
        out["torch_over_fused"] = out["torch_ms_per_launch"] / out["fused_ms_per_launch"]
    return out


def pretrain_table(stats, names, M):
    """The rows `pretrain` returns as a compact table: per statistic and charger ONE string of the iterations' values ("%.3g", space
    separated, iteration 0 first), for the first and the last row of every iteration's device table; `beta` likewise, one value per
    iteration."""
    fmt = lambda xs: " ".join("%.3g" % x for x in xs)
    rows = sorted(stats, key=lambda r: (r["agent"], r["iteration"]))
    tab = {"layout": "per statistic: first / last row of each iteration's table (first: loss and top1 only), one string per charger, iterations in order",
           "beta": fmt(r["beta"] for r in rows if r["agent"] == 0)}
    for j, name in enumerate(names):
        if name == "nll":                                      # loss + ent_coef * entropy: not kept twice
            continue
        if name == "kv_share":                                 # 1 wherever the labels are the heuristic's on live networks: its minimum is kept
            tab["kv_share_min"] = [min(min(r["first"][j], r["last"][j]) for r in rows if r["agent"] == a) for a in range(M)]
            continue
        rows_kept = ("first", "last") if name in ("loss", "top1") else ("last",)      # the parts and the entropy: after the iteration's update only
        tab[name] = {w: [fmt(r[w][j] for r in rows if r["agent"] == a) for a in range(M)] for w in rows_kept}
    return tab


def device_envs(args, N=200, M=3):
    """(training batch, held-out evaluation batch) on the device."""
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario
    train_env = VecWRSN([synth_scenario(e, N, N) for e in range(args.envs)], None, M, render=False, entities=True, auto_reset=True, step_budget=1250)
    eval_env = VecWRSN([synth_scenario(1_000_000 + e, N, N) for e in range(args.eval_envs)], None, M, render=False, entities=True, step_budget=1250)
    return train_env, eval_env


def compare(args, make_envs=device_envs):
    """The policy comparison; `make_envs(args)` gives the two batches (the tests pass emulated ones)."""
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import (BatchedEntityIPPO, BatchedEntityPointerIPPO, EntityPolicy, HeuristicLabelPolicy, HeuristicPolicy, PointerPolicy,
                                         UniformPolicy, evaluate_policy)
    from multi_agent_rl_wrsn_amd.evaluate import LaunchCapReached
    torch.manual_seed(0); np.random.seed(0)
    train_env, eval_env = make_envs(args)
    N, M = train_env.n_node, train_env.num_agent
    pointer = args.policy == "pointer"
    ppo = dict(batch_size=args.batch_size, minibatch_size=args.minibatch_size, n_updates_per_iteration=5)
    if pointer:
        def pointer_algo(env, mask):
            torch.manual_seed(0); np.random.seed(0)           # the same seeds for every trainer of the run
            return BatchedEntityPointerIPPO(ppo, env, capacity=max(4096, 2 * args.batch_size), fused_policy=True, log_episodes=True,
                                            min_charge=args.min_charge, device_update=args.device_update, joint_update=args.joint_update,
                                            fused_prepare=args.fused_prepare, mask_claimed=mask)
        algo = pointer_algo(train_env, False)
        Policy = lambda det, g=None: PointerPolicy(algo.packed_actors(), det, g, args.min_charge)
    else:
        algo = BatchedEntityIPPO(ppo, train_env, capacity=max(4096, 2 * args.batch_size), fused_policy=True,
                                 fused_update=True, joint_update=True, fused_prepare=True, log_episodes=True)
        Policy = lambda det, g=None: EntityPolicy(algo.packed_actors(), det, g)
    gen = lambda: torch.Generator(device=eval_env.device).manual_seed(7)
    out = {"eval_set": "%d synthetic %d-node networks, seeds 1000000.., %d chargers, %d episode(s) each, time limit %g s" %
                       (args.eval_envs, N, M, args.episodes, min(s.max_time for s in eval_env.scenarios)),
           "device": torch.cuda.get_device_name(eval_env.device) if eval_env.device.type == "cuda" else str(eval_env.device),
           "max_launches": args.max_launches, "policy": args.policy, "policies": {}}
    if pointer:
        out["min_charge"] = args.min_charge
        out["training_flags"] = {k: bool(getattr(args, k)) for k in ("device_update", "joint_update", "fused_prepare")}

    def run(name, policy):
        t0 = time.perf_counter()
        try:
            res, capped = evaluate_policy(eval_env, policy, episodes=args.episodes, max_launches=args.max_launches), False
        except LaunchCapReached as ex:
            res, capped = ex.result, True
        row = dict(res["summary"], launches=int(res["launches"]), launch_cap_reached=capped, seconds=time.perf_counter() - t0)
        if capped:
            row.update(environments_finished=int((res["finished"] >= args.episodes).sum()), environments_standing_still=int(res["standing"].sum()))
        out["policies"][name] = row
        print(name, json.dumps(row), flush=True)

    run("uniform", UniformPolicy(gen()))
    run("heuristic", HeuristicPolicy())
    run("heuristic_min_charge", HeuristicPolicy(min_charge=args.min_charge))
    if pointer and args.pretrain > 0:
        run("heuristic_as_label", HeuristicLabelPolicy(1.0, args.min_charge, args.x_clip))
    def train_and_run(algo, train_env, Policy, prefix=""):
        run(prefix + "untrained_mode", Policy(True))
        run(prefix + "untrained_sampled", Policy(False, gen()))
        record = train(algo, train_env)
        run(prefix + "trained_mode", Policy(True))
        run(prefix + "trained_sampled", Policy(False, gen()))
        return record

    def train(algo, train_env):
        t0 = time.perf_counter()
        # The trainer raises when a row comes back with a negative status (an environment whose step reported an error: seen after a handful
        # of iterations at these shapes).  Here such rows are counted, not fatal: they are a few of thousands and ask nobody for an action.
        algo._check_status = False
        errors = torch.zeros((), dtype=torch.int64, device=train_env.device)
        step = train_env.step

        def counting_step(ids, act):
            r = step(ids, act)
            errors.add_((r["status"] < 0).sum())
            return r

        train_env.step = counting_step
        rows = algo.train(args.iters - 1) if args.iters > 0 else []
        train_env.step = step
        return {"iterations": len(rows) // M, "error_status_rows_summed_over_launches": int(errors), "launches": algo.timers["launches"],
                "seconds": time.perf_counter() - t0,
                "last_rows": [{k: r[k] for k in ("iteration", "agent", "mean_reward", "avg_ep_lifetime", "avg_ep_lens", "episodes")} for r in rows[-M:]]}

    def pretrain_and_run(mask, prefix):
        """A trainer of its own from the same seeds: cloning alone, then PPO on top."""
        env_b, spare = make_envs(args)
        spare.close() if hasattr(spare, "close") else None
        algo_b = pointer_algo(env_b, mask)
        algo_b._check_status = False                          # as `train` below: rows with an error status are not fatal here
        Pol = lambda det, g=None: PointerPolicy(algo_b.packed_actors(), det, g, args.min_charge, mask)
        t0 = time.perf_counter()
        stats = algo_b.pretrain(args.pretrain, beta=args.beta, beta_end=args.beta_end, critic_iters=args.critic_iters, x_clip=args.x_clip,
                                max_launches=25 * args.max_launches)
        names = ("loss", "nll", "node_part", "charge_part", "entropy", "top1", "kv_share")
        record = {"iterations": args.pretrain, "beta": args.beta, "beta_end": args.beta if args.beta_end is None else args.beta_end,
                  "critic_iters": args.critic_iters, "x_clip": args.x_clip, "seconds": time.perf_counter() - t0,
                  "per_iteration": pretrain_table(stats, names, M)}
        run(prefix + "bc_mode", Pol(True))
        run(prefix + "bc_sampled", Pol(False, gen()))
        record["fine_tuning"] = train(algo_b, env_b)
        run(prefix + "bc_ppo_mode", Pol(True))
        run(prefix + "bc_ppo_sampled", Pol(False, gen()))
        return record

    out["training"] = train_and_run(algo, train_env, Policy)
    if pointer and args.pretrain > 0:
        out["pretraining"] = pretrain_and_run(False, "")
    if pointer and args.mask_claimed:
        train_m, spare = make_envs(args)                      # a training batch of its own, from the same seeds
        spare.close() if hasattr(spare, "close") else None
        algo_m = pointer_algo(train_m, True)
        out["masked_training"] = train_and_run(algo_m, train_m, lambda det, g=None: PointerPolicy(algo_m.packed_actors(), det, g, args.min_charge, True),
                                               "masked_")
        if args.pretrain > 0:
            out["masked_pretraining"] = pretrain_and_run(True, "masked_")
    return out


def lookahead_compare(args):
    """The heuristic and the lookahead policy over it on the held-out set, in the same run."""
    import numpy as np
    import torch
    from multi_agent_rl_wrsn_amd import HeuristicPolicy, LookaheadPolicy, VecWRSN, evaluate_policy, synth_scenario
    from multi_agent_rl_wrsn_amd.evaluate import LaunchCapReached
    N, M = 200, 3
    scs = [synth_scenario(1_000_000 + e, N, N) for e in range(args.eval_envs)]
    env = VecWRSN(scs, None, M, render=False, entities=True, step_budget=1250)
    out = {"eval_set": "%d synthetic %d-node networks, seeds 1000000.., %d chargers, %d episode(s) each, time limit %g s, ONE seed" %
                       (args.eval_envs, N, M, args.episodes, min(s.max_time for s in scs)),
           "device": torch.cuda.get_device_name(env.device), "max_launches": args.max_launches, "min_charge": args.min_charge, "record_bytes": env.record_bytes(), "policies": {}}

    def run(name, policy, extra=None):
        torch.cuda.synchronize(env.device); t0 = time.perf_counter()
        try:
            res, capped = evaluate_policy(env, policy, episodes=args.episodes, max_launches=args.max_launches), False
        except LaunchCapReached as ex:
            res, capped = ex.result, True
        torch.cuda.synchronize(env.device)
        sec = time.perf_counter() - t0
        row = dict(res["summary"], launches=int(res["launches"]), launch_cap_reached=capped, seconds=sec, ms_per_real_launch=1e3 * sec / max(1, int(res["launches"])))
        row["decisions_per_episode"] = float(res["decisions"].sum(-1).mean())
        row.update(extra() if extra else {})
        out["policies"][name] = row
        print(name, json.dumps(row), flush=True)
        if args.out:                                           # kept row by row: a long comparison that is cut short leaves what it has
            with open(args.out, "w") as w:
                json.dump(out, w, indent=1)
        return row

    base = run("heuristic_min_charge", HeuristicPolicy(min_charge=args.min_charge))
    interval = base["lifetime_mean"] / max(1.0, base["decisions_per_episode"])
    out["heuristic_mean_request_interval_s"] = interval
    horizons = args.horizon or [interval, 3 * interval, 10 * interval]
    out["horizons_s"] = horizons
    for K in args.lookahead:
        sim = VecWRSN(scs * K, None, M, render=False, entities=True, step_budget=1250)
        for T in horizons:
            pol = LookaheadPolicy(sim, K=K, horizon=T, min_charge=args.min_charge, max_launches=args.sim_launches)
            cnt = torch.zeros(3, dtype=torch.int64, device=env.device)   # decisions, choice != 0 by survival, by return at equal survival

            def counting(e, ids, pol=pol, cnt=cnt):
                if args.label_yardstick:                       # wrsn_entity_heuristic_label on the same rows, for a kernel trace
                    e.entity_heuristic_label(ids, 1.0, args.min_charge, args.x_clip)
                act = pol(e, ids)
                rows = (ids >= 0) & (ids < M)
                c = pol.choice.long()
                sv = pol.look.survived
                better = sv.gather(0, c[None, :])[0] > sv[0]
                cnt.add_(torch.stack([rows.sum(), (rows & (c != 0) & better).sum(), (rows & (c != 0) & ~better).sum()]))
                return act

            def extra(pol=pol, cnt=cnt):
                d, a, b = (int(x) for x in cnt.cpu())
                return {"K": pol.K, "horizon_s": pol.horizon, "decisions": d, "share_choice_not_0": (a + b) / max(1, d), "decided_by_survival": a,
                        "decided_by_return": b, "sim_launches_per_real_launch": pol.sim_launches / max(1, pol.calls),
                        "wall_per_real_launch_over_heuristic": None}

            row = run("lookahead_K%d_T%g" % (K, T), counting, extra)
            row["wall_per_real_launch_over_heuristic"] = row["ms_per_real_launch"] / base["ms_per_real_launch"]
            row["lifetime_mean_over_heuristic"] = row["lifetime_mean"] / base["lifetime_mean"]
        sim.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", default="gaussian", choices=["gaussian", "pointer"], help="gaussian: the set policy (BatchedEntityIPPO, the default); "
                    "pointer: the node-pointer policy (BatchedEntityPointerIPPO, PointerPolicy)")
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--minibatch-size", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--max-launches", type=int, default=4000)
    ap.add_argument("--min-charge", type=float, default=0.02)
    ap.add_argument("--mask-claimed", action="store_true", help="pointer: every pointer row also with the candidate mask (masked_...)")
    for k in ("device-update", "joint-update", "fused-prepare"):
        ap.add_argument("--" + k, action="store_true", help="pointer: BatchedEntityPointerIPPO(%s=True)" % k.replace("-", "_"))
    ap.add_argument("--pretrain", type=int, default=0, help="pointer, with --device-update: iterations of imitation pretraining from the heuristic")
    ap.add_argument("--beta", type=float, default=1.0, help="pretraining: the share of decisions the expert executes in the first iteration")
    ap.add_argument("--beta-end", type=float, default=None, help="pretraining: the share in the last iteration (default: --beta)")
    ap.add_argument("--critic-iters", type=int, default=0, help="pretraining: critic-only iterations after it")
    ap.add_argument("--x-clip", type=float, default=4.0, help="pretraining: the clamp of the label's charge variable")
    ap.add_argument("--fused-policy", action="store_true", help="pointer: accepted for symmetry with bench_ippo.py; the tool always acts fused")
    ap.add_argument("--lookahead", type=int, action="append", default=None, help="K: compare LookaheadPolicy(K) with the heuristic (repeatable)")
    ap.add_argument("--horizon", type=float, action="append", default=None, help="lookahead: a horizon in simulated seconds (repeatable; default 1, 3, "
                    "10 times the heuristic's mean request interval)")
    ap.add_argument("--label-yardstick", action="store_true", help="lookahead: also run wrsn_entity_heuristic_label at every decision (kernel traces)")
    ap.add_argument("--sim-launches", type=int, default=64, help="lookahead: launches of the simulation batch per decision, at most")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--only", default=None, choices=[None, "fused", "torch"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.pretrain > 0 and not (args.policy == "pointer" and args.device_update):
        ap.error("--pretrain needs --policy pointer --device-update")
    out = bench(args) if args.bench else lookahead_compare(args) if args.lookahead else compare(args)
    path = args.out or os.path.join(ROOT, "profiles", "episodes_bench.json" if args.bench else "lookahead_eval.json" if args.lookahead else
                                    "entity_pointer_bc_eval.json" if args.policy == "pointer" and args.pretrain > 0 else
                                    "entity_pointer_mask_eval.json" if args.policy == "pointer" and args.mask_claimed else
                                    "entity_pointer_eval.json" if args.policy == "pointer" else "entity_eval.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as w:
        json.dump(out, w, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
