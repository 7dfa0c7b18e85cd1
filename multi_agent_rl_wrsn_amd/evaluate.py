"""Whole-episode evaluation on the device: `evaluate_policy` runs a policy for a fixed number of finished episodes per environment and
returns one entry per episode -- network lifetime, return and decisions per charger, why the episode ended -- from the episode ledger
(`wrsn_episodes_collect`).  The loop only enqueues: the ledger books every request, closes episodes (also the ones that outlive `max_time`
and would otherwise return at the same instant forever), parks an environment once it has its episodes and hands back the ids of the next
launch and the restart mask; the host reads one flag every `poll` launches.

Policies are callables `policy(env, ids) -> float64 [B, 3]` (rows with ids outside [0, M) are ignored by `env.step`):
`EntityPolicy` (the learned set policy through `wrsn_entity_act`, its mode or a sample), `PointerPolicy` (the learned node-pointer
policy through `wrsn_entity_pointer_act`, likewise), `HeuristicPolicy` (the deterministic baseline of
`wrsn_entity_heuristic_act`), `HeuristicLabelPolicy` (the same decision squashed the pointer's way, `wrsn_entity_heuristic_label`),
`LookaheadPolicy` (the heuristic's K best picks scored on clones in a second batch, `wrsn_lookahead_candidates` / `_collect` / `_pick`)
and `UniformPolicy` (`torch.rand`)."""
import numpy as np

from ._lib import ENDED_FELL_OFF, ENDED_TERMINAL, ENDED_TIME_LIMIT, POINTER_MASK_CLAIMED, POINTER_MASK_NONE

ENDED_NAMES = {ENDED_TERMINAL: "terminal", ENDED_TIME_LIMIT: "time_limit", ENDED_FELL_OFF: "fell_off"}


class EntityPolicy:
    """The actors `packed_actors` ([M, P], `EntityPPOLearner.packed_actors()`) through `VecWRSN.entity_act`: the mode of the Gaussian
    (`deterministic=True`, eps == NULL) or a sample with `torch.randn` draws of `generator` (on the environment's device; None: the
    default generator)."""

    def __init__(self, packed_actors, deterministic=True, generator=None):
        self.packed, self.deterministic, self.generator = packed_actors, bool(deterministic), generator

    def __call__(self, env, ids):
        eps = None
        if not self.deterministic:
            t = env.torch
            eps = t.randn((env.num_env, 3), dtype=t.float32, device=env.device, generator=self.generator)
        return env.entity_act(ids, self.packed, eps)[1]


class PointerPolicy:
    """The node-pointer actors `packed_actors` ([M, P], `EntityPointerPPOLearner.packed_actors()`) through `VecWRSN.entity_pointer_act`:
    the most probable node and the mode of the charge variable (`deterministic=True`), or a sample with Gumbel noise -log(-log(u)), u
    from `torch.rand`, and `torch.randn` draws of `generator`.  The third component of every action is at least `min_charge`: with
    min_charge > 0 every decision spends simulated time, so the policy cannot stand still.  mask_claimed: the candidate mask the actors
    act under (`VecWRSN.set_entity_pointer_mask`), set on the environment at every call -- True for actors trained with it, False (the
    default) for every alive node."""

    def __init__(self, packed_actors, deterministic=True, generator=None, min_charge=0.02, mask_claimed=False):
        self.packed, self.deterministic, self.generator, self.min_charge = packed_actors, bool(deterministic), generator, float(min_charge)
        self.mask_claimed = bool(mask_claimed)

    def __call__(self, env, ids):
        env._h.set_entity_pointer_mask(POINTER_MASK_CLAIMED if self.mask_claimed else POINTER_MASK_NONE)   # what `VecWRSN.set_entity_pointer_mask` calls
        g = eps = None
        if not self.deterministic:
            t = env.torch
            u = t.rand((env.num_env, env.n_node), dtype=t.float32, device=env.device, generator=self.generator)
            g = -t.log(-t.log(u))
            eps = t.randn((env.num_env,), dtype=t.float32, device=env.device, generator=self.generator)
        return env.entity_pointer_act(ids, self.packed, g, eps, self.min_charge)[1]


class HeuristicPolicy:
    """The most critical node no other charger is heading for (`VecWRSN.entity_heuristic_act`); the charging time is
    clip(charge_scale * (1 - the node's energy fraction), 0, 1) of `charging_time_max`.  min_charge > 0 raises that third component to
    at least min_charge (one elementwise clamp on the kernel's output): a charger that is sent to a node it already stands at, and
    that is full, then still spends simulated time, so the request cannot come back at the same instant forever.
    0 (the default) is the kernel's rule as it stands."""

    def __init__(self, charge_scale=1.0, min_charge=0.0):
        self.charge_scale, self.min_charge = float(charge_scale), float(min_charge)

    def __call__(self, env, ids):
        act = env.entity_heuristic_act(ids, self.charge_scale)[1]
        if self.min_charge > 0.0:
            act[:, 2].clamp_(min=self.min_charge)
        return act


class HeuristicLabelPolicy:
    """The heuristic's decision acted out the node-pointer policy's way (`VecWRSN.entity_heuristic_label`): the heuristic's node, and the
    charging time min_charge + (1 - min_charge) * sigmoid(x) of the label's x, x clamped to [-x_clip, x_clip].  What a pointer that
    reproduced its labels exactly would do: against `HeuristicPolicy` it shows what the clamp and the squashing alone cost.  The charging
    time is at least min_charge + (1 - min_charge) * sigmoid(-x_clip) > 0, so this policy cannot stand still either."""

    def __init__(self, charge_scale=1.0, min_charge=0.02, x_clip=4.0):
        self.charge_scale, self.min_charge, self.x_clip = float(charge_scale), float(min_charge), float(x_clip)

    def __call__(self, env, ids):
        t = env.torch
        stored, _, act = env.entity_heuristic_label(ids, self.charge_scale, self.min_charge, self.x_clip)
        act[:, 2] = self.min_charge + (1.0 - self.min_charge) * t.sigmoid(stored[:, 1].double())
        return act


class LookaheadPolicy:
    """One step of policy improvement over the heuristic: for every request the heuristic's K best nodes (`VecWRSN.lookahead_candidates`)
    are each tried on a clone of the environment in `sim_env` -- a `VecWRSN(entities=True, render=False, auto_reset=False)` of
    K * env.num_env environments of the same geometry, created on the same scenarios (tiled K times) so that the capacities agree --
    the clones run on under `HeuristicPolicy(charge_scale, min_charge)` for `horizon` simulated seconds, and the candidate whose clone
    survived longest, then collected the largest return, then has the lowest rank, is played (`VecWRSN.lookahead_pick`).  The real `env`
    is only read.  At most `max_launches` launches of `sim_env` per call; whether every slot has finished is read once every `poll`
    launches, the only host read.  Slots still open after the last launch are closed as they stand, so a step budget on `sim_env` works.
    K = 1 plays `HeuristicPolicy(charge_scale, min_charge)`'s bytes.  After a call: `choice` int32 [B] (the rank played), `stored`
    float32 [B, 2] (the played decision as the node-pointer policy stores one), `look` (the `Lookahead`) and `sim_launches`."""

    def __init__(self, sim_env, K=4, horizon=30.0, charge_scale=1.0, min_charge=0.02, x_clip=4.0, max_launches=64, poll=8):
        self.sim_env, self.K, self.horizon = sim_env, int(K), float(horizon)
        self.charge_scale, self.min_charge, self.x_clip = float(charge_scale), float(min_charge), float(x_clip)
        self.max_launches, self.poll = max(1, int(max_launches)), max(1, int(poll))
        self.rollout = HeuristicPolicy(charge_scale, min_charge)
        self.look = self.choice = self.stored = None
        self.sim_launches = self.calls = 0

    def __call__(self, env, ids):
        sim, K, B = self.sim_env, self.K, env.num_env
        if sim.num_env != K * B or sim.auto_reset or not sim.entities:
            raise ValueError("LookaheadPolicy needs sim_env = VecWRSN(entities=True, auto_reset=False) of K * env.num_env = %d environments" % (K * B))
        if self.look is None or self.look.B != B:
            self.look = env.new_lookahead(K)
            self._src, self._dst = np.tile(np.arange(B, dtype=np.int32), K), np.arange(K * B, dtype=np.int32)
        look = self.look
        look.clear()                                          # rows the candidates call skips: invalid and finished
        env.lookahead_candidates(look, ids, self.horizon, self.charge_scale, self.min_charge, self.x_clip)
        sim.clone_envs_from(env, self._src, self._dst)
        sim.step(look.sim_agent_id.view(-1), look.sim_action.view(-1, 3))
        launches = 1
        while True:
            nxt = sim.lookahead_collect(look)
            if launches % self.poll == 0 and bool(look.done.all()):   # the one host read, every `poll` launches
                break
            if launches >= self.max_launches:
                break
            sim.step(nxt, self.rollout(sim, nxt))
            launches += 1
        sim.lookahead_collect(look, close_all=True)
        self.choice, act, self.stored = env.lookahead_pick(look, ids)
        self.sim_launches += launches; self.calls += 1
        return act


class UniformPolicy:
    """Actions uniform in [0, 1)^3 (`torch.rand`, float64, with `generator` on the environment's device; None: the default generator)."""

    def __init__(self, generator=None):
        self.generator = generator

    def __call__(self, env, ids):
        t = env.torch
        return t.rand((env.num_env, 3), dtype=t.float64, device=env.device, generator=self.generator)


def summarize(result):
    """lifetime mean / std / min / median / max, the mean return per charger and the share of each `ended` code of a result."""
    life, ended = result["lifetime"], result["ended"]
    if "finished" in result:                                   # a partial result: only the slots that hold an episode
        stored = np.arange(life.shape[0])[:, None] < np.minimum(result["finished"], life.shape[0])[None, :]
        result = dict(result, ep_return=result["ep_return"][stored])
        life, ended = life[stored], ended[stored]
        if life.size == 0:
            return {"episodes": 0}
    s = {"episodes": int(life.size), "lifetime_mean": float(life.mean()), "lifetime_std": float(life.std()), "lifetime_min": float(life.min()),
         "lifetime_median": float(np.median(life)), "lifetime_max": float(life.max()),
         "return_per_charger": result["ep_return"].reshape(-1, result["ep_return"].shape[-1]).mean(0).tolist()}
    s["ended"] = {name: float((ended == code).mean()) for code, name in ENDED_NAMES.items()}
    return s


class LaunchCapReached(RuntimeError):
    """`evaluate_policy` used up `max_launches`.  `result` holds what the ledger has by then, in the layout of a full result plus
    `finished` [B] (episodes closed per environment: slots [finished[e]:, e] are empty), `running_return` / `running_decisions` [B, M] (the
    sums of the episodes in progress) and `standing` [B] (1: the environment's last
    two requests came at the same instant for the same charger -- a policy that repeats an action of zero duration)."""

    def __init__(self, msg, result):
        super().__init__(msg)
        self.result = result


def evaluate_policy(env, policy, episodes=1, time_limit=None, poll=8, max_launches=100000):
    """Run `policy` on `env` -- a `VecWRSN(entities=True, auto_reset=False)`; anything else: ValueError -- until every environment has
    finished `episodes` episodes.  An episode ends by a terminal return (network death), by a request at env.now >= time_limit
    (None: the smallest `max_time` of the environment's scenarios; 0: no limit) or by a step that falls off the end.  Finished
    environments restart in a record of the pool when one is set (`set_pool`), in their own scenario otherwise, and are parked once they
    have their episodes.  After `max_launches` launches: `LaunchCapReached`, a RuntimeError whose `result` is the partial log.

    Returns a dict of numpy arrays: `lifetime` [E, B], `ep_return` [E, B, M], `decisions` [E, B, M], `ended` [E, B] (1 terminal, 2 time
    limit, 3 fell off), `record` [E, B] (the pool record, -1: none), `launches`, and `summary` (`summarize`)."""
    if not getattr(env, "entities", False) or getattr(env, "auto_reset", True):
        raise ValueError("evaluate_policy needs a VecWRSN(entities=True, auto_reset=False)")
    episodes, poll, max_launches = int(episodes), max(1, int(poll)), int(max_launches)
    if time_limit is None:
        time_limit = min(float(s.max_time) for s in env.scenarios)
    pooled = getattr(env, "_pool", None) is not None
    log = env.new_episode_log(episodes, quota=episodes)
    log.clear()
    env.reset()
    ids, restart = env.episodes_collect(log, time_limit)
    launches = 0
    last_now = None
    while True:
        if launches + 1 >= max_launches:                      # the request in front of the last launch: what "standing" compares with
            last_now, last_ids = env._result()["now"].clone(), ids.clone()
        env.step(ids, policy(env, ids))
        ids, restart = env.episodes_collect(log, time_limit)
        env.pool_reset(mask=restart) if pooled else env.reset(mask=restart)   # an all-zero mask touches nothing
        ids, restart = env.episodes_collect(log, time_limit)                  # the restarted rows' requests
        launches += 1
        if launches % poll == 0 or launches >= max_launches:                  # the one host read, every `poll` launches
            if bool((log.finished >= episodes).all()):
                break
            if launches >= max_launches:
                part = _result(log, launches)
                part["finished"] = log.finished.cpu().numpy().copy()
                part["running_return"], part["running_decisions"] = log.run_return.cpu().numpy().copy(), log.run_decisions.cpu().numpy().copy()
                part["standing"] = ((ids >= 0) & (ids == last_ids) & (env._result()["now"] == last_now)).cpu().numpy().astype(np.uint8)
                part["summary"] = summarize(part)
                raise LaunchCapReached("evaluate_policy: %d launches and not every environment has finished %d episodes (fewest: %d, "
                                       "standing still: %d)" % (launches, episodes, int(part["finished"].min()), int(part["standing"].sum())), part)
    result = _result(log, launches)
    result["summary"] = summarize(result)
    return result


def _result(log, launches):
    result = {k: getattr(log, k).cpu().numpy().copy() for k in ("lifetime", "ep_return", "decisions", "ended", "record")}
    result["launches"] = np.array(launches)
    return result
