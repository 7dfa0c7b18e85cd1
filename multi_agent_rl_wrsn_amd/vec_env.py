"""VecWRSN -- B independent WRSN environments stepped by the gfx950 kernels (one wavefront per environment).

Batched counterpart of the reference's `rl_env.WRSN.WRSN` (rl_env/WRSN.py:21): the same asynchronous
multi-agent protocol -- `reset()` / `step(agent_ids, actions)` return, per environment, the id of the mobile
charger that needs an action, its reward, a 4 x G x G observation, the terminal flag and the simulated time
-- with every array living in HBM as a torch tensor.  torch is used for device memory and streams only; all
environment arithmetic happens in csrc/ (HIP) behind the C-ABI of include/wrsn_hip.h.
"""
import numpy as np

from . import _lib
from .scenario import DEFAULT_MC_SPEC, MC_SPEC_KEYS, Scenario, load_mc_yaml


def _mc_spec_dict(agent_type):
    if agent_type is None:
        return dict(DEFAULT_MC_SPEC)
    if isinstance(agent_type, str):
        return load_mc_yaml(agent_type)
    return {k: float(agent_type[k]) for k in MC_SPEC_KEYS}


def obs_torch_dtype(obs_dtype):
    """"float32" / "bfloat16" (or the torch dtypes) -> torch dtype of the observation tensors; anything else: ValueError."""
    import torch
    if obs_dtype in ("float32", torch.float32):
        return torch.float32
    if obs_dtype in ("bfloat16", torch.bfloat16):
        return torch.bfloat16
    raise ValueError("obs_dtype must be 'float32' or 'bfloat16' (or torch.float32 / torch.bfloat16), got %r" % (obs_dtype,))


class EpisodeLog:
    """The episode ledger of `wrsn_episodes_collect` for B environments x M chargers: the tensors under the field names of
    `wrsn_episode_log` (`run_return`, `run_decisions`, `finished`, `dropped`, `lifetime`, `ep_return`, `decisions`, `ended`, `record`),
    `episodes` stored per environment and the parking `quota`.  `clear()` zeroes everything (asynchronously); `clear(keep_running=True)`
    keeps the sums of the episodes in progress, for a log that is read and emptied while its environments go on."""

    def __init__(self, torch, device, B, M, episodes, quota=0):
        E, quota = int(episodes), int(quota)
        if E < 1 or not 0 <= quota <= E:
            raise ValueError("episodes must be >= 1 and quota in [0, episodes], got %d and %d" % (E, quota))
        self.episodes, self.quota = E, quota
        f64, i32 = torch.float64, torch.int32
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self.run_return, self.run_decisions = z((B, M), f64), z((B, M), i32)
        self.finished, self.dropped = z((B,), i32), z((B,), i32)
        self.lifetime, self.ep_return, self.decisions = z((E, B), f64), z((E, B, M), f64), z((E, B, M), i32)
        self.ended, self.record = z((E, B), i32), z((E, B), i32)
        self.raw = _lib.WrsnEpisodeLog(E, quota, *(getattr(self, k).data_ptr() for k in _lib.EPISODE_LOG_ARRAYS))

    def clear(self, keep_running=False):
        for k in _lib.EPISODE_LOG_ARRAYS:
            if not (keep_running and k in ("run_return", "run_decisions")):
                getattr(self, k).zero_()


class Lookahead:
    """The state of the lookahead calls for K candidates per row of a real batch of B environments (`wrsn_lookahead_state`: `t0`, `t_end`,
    `last_now`, `ret`, `survived` float64 and `done`, `died` uint8, all [K, B]), the k-major candidate tensors -- `node`, `sim_agent_id`
    int32 [K, B], `sim_action` float64 [K, B, 3], `cand_stored` float32 [K, B, 2]: the simulation batch's step inputs as they stand --
    `next_agent_id` int32 [K * B], and the choice per real row: `choice` int32 [B], `action_f64` [B, 3], `action` [B, 3], `stored` [B, 2].
    `clear()` marks every slot invalid and finished (asynchronously), which is what rows a candidates call skips must hold."""

    def __init__(self, torch, device, K, B):
        if not 1 <= K <= _lib.LOOKAHEAD_MAX_K:
            raise ValueError("K must lie in [1, %d], got %d" % (_lib.LOOKAHEAD_MAX_K, K))
        self.K, self.B = K, B
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        for k in _lib.LOOKAHEAD_F64:
            setattr(self, k, z((K, B), torch.float64))
        for k in _lib.LOOKAHEAD_U8:
            setattr(self, k, z((K, B), torch.uint8))
        self.node, self.sim_agent_id = z((K, B), torch.int32), z((K, B), torch.int32)
        self.sim_action, self.cand_stored = z((K, B, 3), torch.float64), z((K, B, 2), torch.float32)
        self.next_agent_id = z((K * B,), torch.int32)
        self.choice, self.action_f64, self.action, self.stored = z((B,), torch.int32), z((B, 3), torch.float64), z((B, 3), torch.float32), z((B, 2), torch.float32)
        self.raw = _lib.WrsnLookaheadState(K, B, *(getattr(self, k).data_ptr() for k in _lib.LOOKAHEAD_F64 + _lib.LOOKAHEAD_U8))
        self.clear()

    def clear(self):
        self.node.fill_(-1); self.sim_agent_id.fill_(-2); self.next_agent_id.fill_(-2); self.done.fill_(1)


class VecWRSN:
    """Batched WRSN environment on one MI355X.

    scenarios : list of `Scenario` (one per environment; the same object may repeat)
    agent_type: dict / YAML path of the charger parameters (mc_types/default.yaml), None = shipped defaults
    num_agent : number of mobile chargers per environment (`num_agent`, WRSN.py:26)
    auto_reset: an environment whose last return was terminal is reset by the next `step` (status 3)
    reuse_obs : False (default): every returned row of `state` is rendered in full and the caller may do with the tensor what it likes.
                True: the caller promises to treat `state` as READ-ONLY (clone before normalising / clipping in place) -- map 1 of a row,
                the node map, which depends on node state only, is then not re-rendered by a step that returns at the instant it was
                called (`wrsn_set_obs_reuse`, ~40 % of the random-policy benchmark's returns); bit-identical results when the promise is
                kept, stale / corrupted map 1 when it is not.  bench.py, bench_ippo.py and the diagnostics opt in.
    step_budget: 0 = every `step` runs each WRSN.step to its end (the reference's blocking call).  > 0 bounds the work
                of one launch per environment (units of ~400 cycles counted per simulated second / service / exact second): an
                environment whose step is still in flight reports status 4 / agent_id -1 and simply goes on in the
                next `step` (its agent_id / action row is ignored).  Requests are identical either way; only the
                launch they appear in differs, so a batch no longer waits for its slowest environment.
    step_deadline_us: > 0 = time-sliced launches (`wrsn_set_step_deadline`): every launch lasts about that long; the waves walk the
                environments in a cyclic order, an environment whose step is not finished (or not even begun: its action then waits in a
                latch inside the library) reports status 4 / agent_id -1 and goes on in the following launches.  Same requests; which
                launch reports one depends on timing.  May be combined with a step budget (a cap per visit).
    obs_dtype : "float32" (default) or "bfloat16" (also torch.float32 / torch.bfloat16): the dtype of `state` and of what `render_state`
                returns, fixed for the life of the object (`wrsn_set_obs_format`).  A bfloat16 cell is the float32 cell rounded to nearest
                even by the render kernel itself: half the bytes written per step and kept per stored observation.
    entities  : True = the entity observation (`wrsn_set_entity_out`): every call that renders also writes, for the rows it renders, the
                numbers `state` is a picture of -- `nodes` [B,N,8], `chargers` [B,M,12] and `env_feat` [B,8], float32, slots named by
                `ENT_NODE` / `ENT_MC` / `ENT_ENV` -- and the returned dict holds them.  Legal with `render=False` (no image at all: the
                observation for MLP, set and graph policies) and with every launch option.  Rows a call does not render keep their bytes.
    """

    def __init__(self, scenarios, agent_type=None, num_agent=3, map_size=100, warm_up_time=100, device="cuda:0",
                 auto_reset=False, render=True, max_degree=0, max_cover=0, step_budget=0, reuse_obs=False, step_deadline_us=0,
                 obs_dtype="float32", entities=False):
        import torch
        self.obs_dtype = obs_torch_dtype(obs_dtype)            # ValueError before anything is created
        if not torch.cuda.is_available():
            raise RuntimeError("VecWRSN needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("VecWRSN runs on HIP devices only")
        scenarios = list(scenarios)
        if not scenarios or not all(isinstance(s, Scenario) for s in scenarios):
            raise TypeError("scenarios must be a non-empty list of Scenario")
        self.scenarios = scenarios
        self.mc_spec = _mc_spec_dict(agent_type)
        self.num_env = len(scenarios)
        self.num_agent = int(num_agent)
        self.map_size = int(map_size)
        self.warm_up_time = float(warm_up_time)
        self.auto_reset = bool(auto_reset)
        self.render = bool(render)
        self.n_node, self.n_target = self._sizes(scenarios)
        lib = _lib.load()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev_index):
            self._h = _lib.RawHandle(lib, self.num_env, self.n_node, self.n_target, self.num_agent, self.map_size,
                                     self.warm_up_time, dev_index, max_degree, max_cover)
            self._h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
            if self.obs_dtype == torch.bfloat16:
                self._h.set_obs_format(_lib.OBS_BF16)
            if reuse_obs and self.render:
                self._h.set_obs_reuse(True)
            self.step_budget = int(step_budget)
            if self.step_budget:
                self._h.set_step_budget(self.step_budget)
            self.step_deadline_us = int(step_deadline_us)
            if self.step_deadline_us:
                self._h.set_step_deadline(self.step_deadline_us)
            # topology build + warm-up + snapshot happen on the device inside set_scenario
            self._h.set_scenarios(scenarios, self.mc_spec)
            B, G = self.num_env, self.map_size
            self.agent_id = torch.full((B,), -1, dtype=torch.int32, device=self.device)
            self.reward = torch.zeros(B, dtype=torch.float64, device=self.device)
            self.terminal = torch.zeros(B, dtype=torch.uint8, device=self.device)
            self.now = torch.zeros(B, dtype=torch.float64, device=self.device)
            self.status = torch.zeros(B, dtype=torch.int32, device=self.device)
            self.state = torch.zeros((B, 4, G, G), dtype=self.obs_dtype, device=self.device) if self.render else None
            self._in_agent = torch.zeros(B, dtype=torch.int32, device=self.device)
            self._in_action = torch.zeros((B, 3), dtype=torch.float64, device=self.device)
            self.entities = bool(entities)
            self.nodes_feat = self.chargers_feat = self.env_feat = None
            if self.entities:
                self.nodes_feat, self.chargers_feat, self.env_feat = self._entity_tensors()
                self._h.set_entity_out(self.nodes_feat.data_ptr(), self.chargers_feat.data_ptr(), self.env_feat.data_ptr())
            self._pool = None                                 # the records of set_pool, alive as long as the handle reads them

    def _sizes(self, scenarios):
        """Node and target count the handle is created for."""
        return max(s.n_node for s in scenarios), max(s.n_target for s in scenarios)

    # -- plumbing -----------------------------------------------------------------------------------------
    def _out_ptrs(self):
        return dict(agent_id=self.agent_id.data_ptr(), reward=self.reward.data_ptr(), terminal=self.terminal.data_ptr(),
                    now=self.now.data_ptr(), status=self.status.data_ptr(),
                    obs=(self.state.data_ptr() if self.state is not None else 0))

    def _result(self):
        r = {"agent_id": self.agent_id, "reward": self.reward, "terminal": self.terminal, "now": self.now,
             "status": self.status, "state": self.state}
        if self.entities:
            r.update(nodes=self.nodes_feat, chargers=self.chargers_feat, env_feat=self.env_feat)
        return r

    def _entity_tensors(self):
        t = self.torch
        return (t.zeros((self.num_env, self.n_node, _lib.ENT_NODE_F), dtype=t.float32, device=self.device),
                t.zeros((self.num_env, self.num_agent, _lib.ENT_MC_F), dtype=t.float32, device=self.device),
                t.zeros((self.num_env, _lib.ENT_ENV_F), dtype=t.float32, device=self.device))

    def _bind_stream(self):
        self._h.set_stream(self.torch.cuda.current_stream(self.device).cuda_stream)

    # -- API ----------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        """WRSN.reset (WRSN.py:41-83) for all environments, or those with mask != 0.  Returns the request
        tensors (views on internal buffers: agent_id, reward, terminal, now, status, state)."""
        self._bind_stream()
        mptr = 0
        if mask is not None:
            self._mask = mask.to(device=self.device, dtype=self.torch.uint8).contiguous()
            mptr = self._mask.data_ptr()
        self._h.reset(mptr, **self._out_ptrs())
        return self._result()

    def step(self, agent_ids, actions):
        """WRSN.step (WRSN.py:289-330) for every environment.

        agent_ids: int tensor [B]; >= 0 gives `actions[b]` to that charger, -1 means "just run" (agent_id=None in
                   the reference), -2 leaves the environment untouched.
        actions  : float tensor [B,3] in [0,1] (clipped inside, WRSN.py:299); density_map=False path."""
        t = self.torch
        self._bind_stream()
        # Arrays that already are what the C-ABI takes (int32 / float64, contiguous, on this device) go in as they are -- including this
        # object's own `agent_id` output tensor: a launch reads row e of the inputs and writes row e of the outputs from the one block
        # that owns environment e.  Anything else is converted into the staging buffers (two small copy kernels per call).
        a = agent_ids
        if not (a.dtype == t.int32 and a.device == self.device and a.is_contiguous() and a.numel() == self.num_env):
            self._in_agent.copy_(a.to(device=self.device, dtype=t.int32).reshape(-1)); a = self._in_agent
        x = actions
        if not (x.dtype == t.float64 and x.device == self.device and x.is_contiguous() and x.numel() == 3 * self.num_env):
            self._in_action.copy_(x.to(device=self.device, dtype=t.float64).reshape(-1, 3)); x = self._in_action
        if self._pool is not None and self.auto_reset:
            # rows whose last return was terminal restart in a drawn pool record, on the device: wrsn_pool_reset marks them -2 in a copy
            # of the ids (never the caller's tensor, never this object's `agent_id` output), the step then leaves them alone and their
            # rows carry the status-3 request of the new network out of this call
            if a is not self._in_agent:
                self._in_agent.copy_(a); a = self._in_agent
            self._h.pool_reset(0, 0, a.data_ptr(), **self._out_ptrs())
        self._keep_in = (a, x)                                # alive until the launch has run
        self._h.step(a.data_ptr(), x.data_ptr(), self.auto_reset, **self._out_ptrs())
        return self._result()

    def render_state(self, agent_ids, out=None):
        """get_state(agent) (WRSN.py:130-186) for arbitrary agents; rows with agent < 0 are left untouched.  `out`, when given, is a
        contiguous [B,4,G,G] tensor of this object's `obs_dtype` on its device."""
        t = self.torch
        self._bind_stream()
        a = agent_ids.to(device=self.device, dtype=t.int32).contiguous()
        if out is None:
            out = t.zeros((self.num_env, 4, self.map_size, self.map_size), dtype=self.obs_dtype, device=self.device)
        elif out.dtype != self.obs_dtype or out.device != self.device or not out.is_contiguous() or \
                out.numel() != self.num_env * 4 * self.map_size * self.map_size:
            raise ValueError("out must be a contiguous %s tensor [%d,4,%d,%d] on %s" %
                             (self.obs_dtype, self.num_env, self.map_size, self.map_size, self.device))
        self._h.render(a.data_ptr(), out.data_ptr())
        return out

    def entity_state(self, agent_ids, out=None):
        """The entity observation of arbitrary agents (`wrsn_entities`; works with or without `entities=True`): a dict of `nodes`
        [B,N,8], `chargers` [B,M,12] and `env_feat` [B,8]; rows with agent < 0 are left untouched.  `out`, when given, is such a dict of
        contiguous float32 tensors on this device."""
        t = self.torch
        self._bind_stream()
        a = agent_ids.to(device=self.device, dtype=t.int32).contiguous()
        if out is None:
            out = dict(zip(("nodes", "chargers", "env_feat"), self._entity_tensors()))
        else:
            want = {"nodes": (self.num_env, self.n_node, _lib.ENT_NODE_F), "chargers": (self.num_env, self.num_agent, _lib.ENT_MC_F),
                    "env_feat": (self.num_env, _lib.ENT_ENV_F)}
            for k, shape in want.items():
                x = out[k]
                if x.dtype != t.float32 or x.device != self.device or not x.is_contiguous() or tuple(x.shape) != shape:
                    raise ValueError("out[%r] must be a contiguous float32 tensor %s on %s" % (k, list(shape), self.device))
        self._h.entities(a.data_ptr(), out["nodes"].data_ptr(), out["chargers"].data_ptr(), out["env_feat"].data_ptr())
        return out

    def entity_act(self, agent_ids, packed, eps=None):
        """`wrsn_entity_act` on the entity rows this object holds (`entities=True`): the chargers `agent_ids` [B] (< 0: row skipped) act with
        the packed actors `packed` [M, P] (`EntityPPOLearner.packed_actors`) and the standard-normal draws `eps` [B, 3] (None: the mode).
        Returns (action float32 [B,3], action_f64 float64 [B,3] -- what `step` takes --, logp float32 [B]): tensors this object owns and
        writes again at the next call; skipped rows keep what they held."""
        t = self.torch
        if not self.entities:
            raise ValueError("entity_act needs a VecWRSN with the entity observation (entities=True)")
        self._bind_stream()
        a = agent_ids
        if not (a.dtype == t.int32 and a.device == self.device and a.is_contiguous() and a.numel() == self.num_env):
            a = a.to(device=self.device, dtype=t.int32).reshape(-1).contiguous()
        P = self._h.lib.wrsn_entity_actor_floats()
        w = packed
        if not (w.dtype == t.float32 and w.device == self.device and w.is_contiguous()):
            w = w.to(device=self.device, dtype=t.float32).contiguous()
        if tuple(w.shape) != (self.num_agent, P):
            raise ValueError("packed actors must be [%d, %d], not %s" % (self.num_agent, P, list(w.shape)))
        e = None
        if eps is not None:
            e = eps.to(device=self.device, dtype=t.float32).contiguous()
            if e.numel() != 3 * self.num_env:
                raise ValueError("eps must be [%d, 3]" % self.num_env)
        if getattr(self, "_act", None) is None:
            B = self.num_env
            self._act = (t.zeros((B, 3), dtype=t.float32, device=self.device), t.zeros((B, 3), dtype=t.float64, device=self.device),
                         t.zeros((B,), dtype=t.float32, device=self.device))
        self._keep_act = (a, w, e)                            # alive until the launch has run
        act, act64, logp = self._act
        self._h.entity_act(w.data_ptr(), a.data_ptr(), e.data_ptr() if e is not None else 0, None,
                           action=act.data_ptr(), action_f64=act64.data_ptr(), logp=logp.data_ptr())
        return act, act64, logp

    def set_entity_pointer_mask(self, mode):
        """`wrsn_set_entity_pointer_mask`: the candidate mask of the node-pointer calls that follow on this object -- `entity_pointer_act`,
        `entity_pointer_eval`, `entity_pointer_ppo_grad`, `entity_pointer_ppo_grad_multi`, `entity_pointer_ppo_update` and the
        behaviour-cloning calls `entity_pointer_bc_grad`, `entity_pointer_bc_grad_multi`, `entity_pointer_bc_update`.
        `_lib.POINTER_MASK_NONE` (0, the default): every alive node is a candidate.  `_lib.POINTER_MASK_CLAIMED` (1, or True): not the
        alive nodes inside the charging disc around another live charger's destination, unless that leaves none.  Launches already
        enqueued keep the mode they were enqueued under."""
        self._h.set_entity_pointer_mask(int(mode))

    def entity_pointer_act(self, agent_ids, packed, gumbel=None, eps=None, min_charge=0.0):
        """`wrsn_entity_pointer_act` on the entity rows this object holds (`entities=True`): the chargers `agent_ids` [B] (< 0: row skipped)
        act with the packed node-pointer actors `packed` [M, P] (`EntityPointerPPOLearner.packed_actors`), the Gumbel draws `gumbel` [B, N]
        (None: the most probable node) and the standard-normal draws `eps` [B] (None: the mode of the charge variable); the third
        component of every action is at least `min_charge`.  Returns (stored float32 [B,2] -- (node, x), what the buffers keep --,
        action_f64 float64 [B,3] -- what `step` takes --, logp float32 [B], node int32 [B], -1: no alive node): tensors this object owns
        and writes again at the next call; skipped rows keep what they held."""
        t = self.torch
        if not self.entities:
            raise ValueError("entity_pointer_act needs a VecWRSN with the entity observation (entities=True)")
        self._bind_stream()
        a = agent_ids
        if not (a.dtype == t.int32 and a.device == self.device and a.is_contiguous() and a.numel() == self.num_env):
            a = a.to(device=self.device, dtype=t.int32).reshape(-1).contiguous()
        P = self._h.lib.wrsn_entity_pointer_floats()
        w = packed
        if not (w.dtype == t.float32 and w.device == self.device and w.is_contiguous()):
            w = w.to(device=self.device, dtype=t.float32).contiguous()
        if tuple(w.shape) != (self.num_agent, P):
            raise ValueError("packed pointer actors must be [%d, %d], not %s" % (self.num_agent, P, list(w.shape)))
        g = e = None
        if gumbel is not None:
            g = gumbel.to(device=self.device, dtype=t.float32).contiguous()
            if g.numel() != self.n_node * self.num_env:
                raise ValueError("gumbel must be [%d, %d]" % (self.num_env, self.n_node))
        if eps is not None:
            e = eps.to(device=self.device, dtype=t.float32).contiguous()
            if e.numel() != self.num_env:
                raise ValueError("eps must be [%d]" % self.num_env)
        if getattr(self, "_ptr_act", None) is None:
            B = self.num_env
            z = lambda shape, dt: t.zeros(shape, dtype=dt, device=self.device)
            self._ptr_act = (z((B, 2), t.float32), z((B, 3), t.float32), z((B, 3), t.float64), z((B,), t.float32), z((B,), t.int32))
        self._keep_ptr_act = (a, w, g, e)                     # alive until the launch has run
        stored, act, act64, logp, node = self._ptr_act
        self._h.entity_pointer_act(w.data_ptr(), a.data_ptr(), g.data_ptr() if g is not None else 0, e.data_ptr() if e is not None else 0,
                                   min_charge, None, node=node.data_ptr(), stored=stored.data_ptr(), action=act.data_ptr(),
                                   action_f64=act64.data_ptr(), logp=logp.data_ptr())
        return stored, act64, logp, node

    def entity_heuristic_act(self, agent_ids, charge_scale=1.0):
        """`wrsn_entity_heuristic_act` on the entity rows this object holds (`entities=True`): for the chargers `agent_ids` [B] (outside
        [0, M): row skipped) the most critical node no other charger is heading for.  Returns (action float32 [B,3], action_f64 float64
        [B,3] -- what `step` takes): tensors this object owns and writes again at the next call; skipped rows keep what they held."""
        t = self.torch
        if not self.entities:
            raise ValueError("entity_heuristic_act needs a VecWRSN with the entity observation (entities=True)")
        self._bind_stream()
        a = agent_ids
        if not (a.dtype == t.int32 and a.device == self.device and a.is_contiguous() and a.numel() == self.num_env):
            a = a.to(device=self.device, dtype=t.int32).reshape(-1).contiguous()
        if getattr(self, "_heur", None) is None:
            B = self.num_env
            self._heur = (t.zeros((B, 3), dtype=t.float32, device=self.device), t.zeros((B, 3), dtype=t.float64, device=self.device))
        self._keep_heur = a                                   # alive until the launch has run
        act, act64 = self._heur
        self._h.entity_heuristic_act(a.data_ptr(), None, charge_scale, action=act.data_ptr(), action_f64=act64.data_ptr())
        return act, act64

    def entity_heuristic_label(self, agent_ids, charge_scale=1.0, min_charge=0.0, x_clip=4.0):
        """`wrsn_entity_heuristic_label` on the entity rows this object holds (`entities=True`): the heuristic's decision for the chargers
        `agent_ids` [B] as the node-pointer policy stores a decision.  Returns (stored float32 [B,2] = ((float) node, x), action float32
        [B,3], action_f64 float64 [B,3] -- `entity_heuristic_act`'s bytes): tensors this object owns and writes again at the next call;
        skipped rows keep what they held."""
        t = self.torch
        if not self.entities:
            raise ValueError("entity_heuristic_label needs a VecWRSN with the entity observation (entities=True)")
        self._bind_stream()
        a = agent_ids
        if not (a.dtype == t.int32 and a.device == self.device and a.is_contiguous() and a.numel() == self.num_env):
            a = a.to(device=self.device, dtype=t.int32).reshape(-1).contiguous()
        if getattr(self, "_label", None) is None:
            B = self.num_env
            self._label = (t.zeros((B, 2), dtype=t.float32, device=self.device), t.zeros((B, 3), dtype=t.float32, device=self.device),
                           t.zeros((B, 3), dtype=t.float64, device=self.device))
        self._keep_label = a                                  # alive until the launch has run
        stored, act, act64 = self._label
        self._h.entity_heuristic_label(a.data_ptr(), None, charge_scale, min_charge, x_clip, stored=stored.data_ptr(), action=act.data_ptr(),
                                       action_f64=act64.data_ptr())
        return stored, act, act64

    def new_episode_log(self, episodes, quota=0):
        """An `EpisodeLog` for this batch: `episodes` finished episodes stored per environment; quota 0 = never park, else an environment
        is parked (left alone, not restarted) once it has finished `quota` episodes."""
        return EpisodeLog(self.torch, self.device, self.num_env, self.num_agent, episodes, quota)

    def episodes_collect(self, log, time_limit=0.0, consume=True):
        """`wrsn_episodes_collect` after a `reset`, `step` or `pool_reset` of this object: books the requests of that call into `log` and
        returns (next_agent_id int32 [B], restart uint8 [B]) -- the ids for the next `step` (-2: leave the row alone, -1: step in flight)
        and the mask of the rows whose episode this call closed, for `reset(mask=...)` / `pool_reset(mask=...)`.  Tensors this object owns.
        time_limit > 0 closes an episode whose request comes at env.now >= time_limit; consume=False leaves the requests to a
        following `TransitionBuffers.collect`."""
        t = self.torch
        self._bind_stream()
        if getattr(self, "_ledger_out", None) is None:
            self._ledger_out = (t.full((self.num_env,), -2, dtype=t.int32, device=self.device), t.zeros(self.num_env, dtype=t.uint8, device=self.device))
        nxt, restart = self._ledger_out
        p = self._out_ptrs(); p.pop("obs", None)
        self._h.episodes_collect(log.raw, time_limit, nxt.data_ptr(), restart.data_ptr(), consume, **p)
        return nxt, restart

    def set_step_budget(self, work_units):
        self.step_budget = int(work_units)
        self._h.set_step_budget(self.step_budget)

    def density_to_action(self, agent_ids, dmaps, out=None):
        """WRSN.density_map_to_action (WRSN.py:229-287, with the exp-normalisation of WRSN.py:293-296) on the device:
        dmaps [B, G, G] -> actions [B, 3] float64 for `step`.  Rows with agent < 0 are left untouched."""
        t = self.torch
        self._bind_stream()
        a = agent_ids.to(device=self.device, dtype=t.int32).contiguous()
        m = dmaps.to(device=self.device, dtype=t.float64).contiguous()
        if out is None:
            out = t.zeros((self.num_env, 3), dtype=t.float64, device=self.device)
        self._h.density_action(a.data_ptr(), m.data_ptr(), out.data_ptr())
        return out

    def rollout_table(self, zero_after=False, out=None):
        """[B, M + 3] float64 device tensor accumulated inside the step kernel: sum of rewards per charger, finished
        episodes, sum of lifetimes (env.now at terminal), completed WRSN.step calls -- the layout of
        `sharding.RolloutStats` (pass it to `RolloutStats.gather_table`)."""
        t = self.torch
        self._bind_stream()
        if out is None:
            out = t.empty((self.num_env, self.num_agent + 3), dtype=t.float64, device=self.device)
        self._h.rollout_table(out.data_ptr(), zero_after)
        return out

    # -- environment records: save, load and clone running environments (wrsn_save_envs / wrsn_load_envs / wrsn_clone_envs) -------------
    @staticmethod
    def _env_list(envs, n):
        return np.arange(n, dtype=np.int32) if envs is None else np.asarray(envs, dtype=np.int64).reshape(-1).astype(np.int32)

    def record_bytes(self):
        """Bytes of one environment record of this batch."""
        return self._h.env_record_bytes()

    def save_envs(self, envs=None):
        """Records of environments `envs` (default: all) with their pending requests: a device uint8 tensor [n, record_bytes()].
        Asynchronous; `.cpu()` / `torch.save` it for a checkpoint."""
        t = self.torch
        self._bind_stream()
        idx = self._env_list(envs, self.num_env)
        rec = t.empty((len(idx), self._h.env_record_bytes()), dtype=t.uint8, device=self.device)
        p = self._out_ptrs(); p.pop("obs")
        self._h.save_envs(idx, rec.data_ptr(), **p)
        return rec

    def load_envs(self, records, envs=None):
        """Replace environments `envs` (default: 0 .. n-1) by `records` ([n, record_bytes] uint8, host or device, from any batch of the same
        geometry) and return the request tensors, whose restored rows now hold the saved requests (state rendered for agent_id >= 0)."""
        t = self.torch
        self._bind_stream()
        if records.dim() != 2 or records.dtype != t.uint8:
            raise ValueError("records must be a uint8 tensor [n, record_bytes]")
        rec = records.to(device=self.device).contiguous()
        idx = self._env_list(envs, rec.shape[0])
        if len(idx) != rec.shape[0]:
            raise ValueError("%d records for %d environments" % (rec.shape[0], len(idx)))
        self._h.load_envs(idx, rec.data_ptr(), **self._out_ptrs())
        return self._result()

    def clone_envs(self, src, dst):
        """Environment dst[i] becomes a copy of src[i] (device to device, asynchronous); its request row follows.  Returns the request
        tensors."""
        self._bind_stream()
        s = np.asarray(src, dtype=np.int64).reshape(-1).astype(np.int32)
        d = np.asarray(dst, dtype=np.int64).reshape(-1).astype(np.int32)
        self._h.clone_envs(s, d, **self._out_ptrs())
        return self._result()

    def clone_envs_from(self, src_env, src, dst):
        """Environment dst[i] of THIS batch becomes a copy of environment src[i] of `src_env`, another batch of the same geometry on the
        same device and stream (`wrsn_clone_envs_from`; device to device, asynchronous, no host read); `src` may repeat.  `src_env` is
        only read.  Its request rows follow into this batch's rows.  Returns this batch's request tensors."""
        self._bind_stream(); src_env._bind_stream()
        s = np.asarray(src, dtype=np.int64).reshape(-1).astype(np.int32)
        d = np.asarray(dst, dtype=np.int64).reshape(-1).astype(np.int32)
        q = dict(src_env._out_ptrs()); q.pop("obs", None)
        self._h.clone_envs_from(src_env._h, s, d, q, **self._out_ptrs())
        return self._result()

    # -- one-step lookahead over the heuristic's K best picks (wrsn_lookahead_candidates / _collect / _pick) --------------------------
    def new_lookahead(self, K):
        """The state and the k-major tensors of a lookahead over K candidates per row of THIS (the real) batch: a `Lookahead`."""
        return Lookahead(self.torch, self.device, int(K), self.num_env)

    def lookahead_candidates(self, look, agent_ids, horizon, charge_scale=1.0, min_charge=0.0, x_clip=4.0):
        """`wrsn_lookahead_candidates` on the entity rows this object holds (`entities=True`) for the chargers `agent_ids` [B]: the
        heuristic's K best nodes per row into `look.node`, `look.sim_agent_id`, `look.sim_action`, `look.cand_stored`, and the slots of
        `look` initialised at this batch's `now`.  Rows outside [0, M) are skipped and keep what they held.  Returns `look`."""
        t = self.torch
        if not self.entities:
            raise ValueError("lookahead_candidates needs a VecWRSN with the entity observation (entities=True)")
        self._bind_stream()
        a = agent_ids
        if not (a.dtype == t.int32 and a.device == self.device and a.is_contiguous() and a.numel() == self.num_env):
            a = a.to(device=self.device, dtype=t.int32).reshape(-1).contiguous()
        look._keep = a                                        # alive until the launch has run
        self._h.lookahead_candidates(a.data_ptr(), self._out_ptrs()["now"], look.raw, horizon, charge_scale, min_charge, x_clip, None,
                                     node=look.node.data_ptr(), sim_agent_id=look.sim_agent_id.data_ptr(), sim_action=look.sim_action.data_ptr(),
                                     stored=look.cand_stored.data_ptr())
        return look

    def lookahead_collect(self, look, close_all=False):
        """`wrsn_lookahead_collect` after a `step` of THIS (the simulation) batch of K * B environments: books its requests into `look`
        and returns `look.next_agent_id` [K * B], the ids of the next `step` (-2: slot closed, -1: step in flight)."""
        self._bind_stream()
        p = self._out_ptrs(); p.pop("obs", None)
        self._h.lookahead_collect(look.raw, look.next_agent_id.data_ptr(), close_all, **p)
        return look.next_agent_id

    def lookahead_pick(self, look, agent_ids):
        """`wrsn_lookahead_pick` on THIS (the real) batch: per row the finished slot with the longest survival, then the largest return,
        then the lowest k.  Returns (choice int32 [B], action_f64 float64 [B,3], stored float32 [B,2]): tensors of `look`."""
        t = self.torch
        self._bind_stream()
        a = agent_ids
        if not (a.dtype == t.int32 and a.device == self.device and a.is_contiguous() and a.numel() == self.num_env):
            a = a.to(device=self.device, dtype=t.int32).reshape(-1).contiguous()
        look._keep = a
        self._h.lookahead_pick(a.data_ptr(), look.raw, look.sim_agent_id.data_ptr(), look.sim_action.data_ptr(), look.cand_stored.data_ptr(),
                               choice=look.choice.data_ptr(), action_f64=look.action_f64.data_ptr(), action=look.action.data_ptr(),
                               stored=look.stored.data_ptr())
        return look.choice, look.action_f64, look.stored

    # -- scenario pools: finished episodes restart in another network, on the device (wrsn_pool_set / wrsn_pool_reset) ----------------
    def set_pool(self, records, seed=0):
        """Register `records` ([P, record_bytes()] uint8, e.g. from `build_scenario_pool`; None clears) as this batch's scenario pool.
        With `auto_reset=True` every `step` from now on restarts the environments whose last return was terminal in a pool record
        drawn on the device (`pool_draw(seed, env, swaps so far, P)`) instead of their own scenario: the same protocol, a status-3 row
        with the reset request, of a new network."""
        t = self.torch
        self._bind_stream()
        if records is None:
            self._h.pool_set(0, 0, 0)
            self._pool = None
            return
        if records.dim() != 2 or records.dtype != t.uint8:
            raise ValueError("records must be a uint8 tensor [P, record_bytes]")
        rec = records.to(device=self.device).contiguous()
        if rec.shape[1] != self._h.env_record_bytes():
            raise ValueError("records of %d bytes, this batch's are %d" % (rec.shape[1], self._h.env_record_bytes()))
        self._h.pool_set(rec.data_ptr(), rec.shape[0], seed)
        self._pool = rec

    def pool_reset(self, mask=None, index=None):
        """Replace the environments with mask != 0 (None: those whose last return was terminal) by the pool records `index` (int tensor
        [B], read for the selected rows; None: drawn on the device).  Asynchronous, no host round trip.  Returns the request tensors:
        replaced rows hold their record's reset request (status 0 with a mask, 3 without), every other row is untouched."""
        t = self.torch
        self._bind_stream()
        mptr = iptr = 0
        if mask is not None:
            self._mask = mask.to(device=self.device, dtype=t.uint8).contiguous(); mptr = self._mask.data_ptr()
        if index is not None:
            self._pool_index = index.to(device=self.device, dtype=t.int32).contiguous(); iptr = self._pool_index.data_ptr()
        self._h.pool_reset(mptr, iptr, 0, **self._out_ptrs())
        return self._result()

    def pool_info(self):
        """Per environment: the pool record it runs (-1: its own scenario or a loaded record) and its swaps since `set_pool` (host copies)."""
        return self._h.pool_info()

    # -- the PPO update of the entity policy (wrsn_entity_eval / wrsn_entity_ppo_grad / wrsn_entity_adam): thin wrappers that bind the stream
    def _entity_rows(self, rows, index):
        t = self.torch
        if not (rows.dtype == t.float32 and rows.is_contiguous() and rows.dim() == 2):
            raise ValueError("rows must be a contiguous float32 tensor [*, R]")
        M = self.num_agent
        N = (rows.shape[1] - 12 * M - 8) // 8
        if N < 1 or 8 * N + 12 * M + 8 != rows.shape[1]:
            raise ValueError("rows of %d floats are no packed entity rows of %d chargers" % (rows.shape[1], M))
        if index is not None and not (index.dtype == t.int32 and index.is_contiguous()):
            raise ValueError("index must be a contiguous int32 tensor")
        n = rows.shape[0] if index is None else index.numel()
        return rows.data_ptr(), (0 if index is None else index.data_ptr()), n, N, M

    def entity_eval(self, rows, actor=None, critic=None, index=None):
        """`wrsn_entity_eval`: the packed actor and / or critic block on packed entity rows [*, R] (row index[i] for minibatch row i;
        None: all rows in order).  Returns (mean [n,3], log_std [n,3], value [n]) as new float32 tensors, None for a net that is not given."""
        t = self.torch
        self._bind_stream()
        rp, ip, n, N, M = self._entity_rows(rows, index)
        new = lambda *sh: t.empty(sh, dtype=t.float32, device=rows.device)
        mean, log_std = (new(n, 3), new(n, 3)) if actor is not None else (None, None)
        value = new(n) if critic is not None else None
        ptr = lambda x: 0 if x is None else x.data_ptr()
        self._h.entity_eval(ptr(actor), ptr(critic), rp, ip, n, N, M, ptr(mean), ptr(log_std), ptr(value))
        return mean, log_std, value

    def _ppo_grad(self, pointer, actor, critic, rows, index, batch, hyper, grad, stats):
        self._bind_stream()
        rp, ip, n, N, M = self._entity_rows(rows, index)
        call, Pa = (self._h.entity_pointer_ppo_grad, self._h.lib.wrsn_entity_pointer_floats()) if pointer else \
                   (self._h.entity_ppo_grad, self._h.lib.wrsn_entity_actor_floats())
        call(actor.data_ptr(), critic.data_ptr(), rp, ip, n, N, M, batch["actions"].data_ptr(), batch["log_probs"].data_ptr(),
             batch["advantages"].data_ptr(), batch["returns"].data_ptr(), batch["values"].data_ptr(), hyper["clip"], hyper["ent_coef"],
             hyper["vf_coef"], hyper["norm_adv"], hyper["clip_vloss"], grad.data_ptr(), grad.data_ptr() + 4 * Pa, stats.data_ptr())

    def entity_ppo_grad(self, actor, critic, rows, index, batch, hyper, grad, stats):
        """`wrsn_entity_ppo_grad`: loss and gradient of one minibatch.  batch: float32 tensors `actions` [*,3], `log_probs`, `advantages`,
        `returns`, `values`, indexed like the rows; hyper: clip, ent_coef, vf_coef, norm_adv, clip_vloss; grad: ONE contiguous float32
        tensor [P_actor + P_critic] (overwritten), stats: float32 [8] (loss, pg, v_loss, entropy, approx_kl, clipfrac, 0, 0)."""
        VecWRSN._ppo_grad(self, False, actor, critic, rows, index, batch, hyper, grad, stats)

    def entity_pointer_eval(self, rows, stored=None, actor=None, critic=None, index=None, node_logp=False):
        """`wrsn_entity_pointer_eval`: the packed node-pointer actor and / or critic block on packed entity rows [*, R] and the stored
        decisions `stored` [*, 2] = (node, x), indexed like the rows (row index[i] for minibatch row i; None: all rows in order).  Returns
        a dict of new float32 tensors: logp [n], entropy [n], mean [n], log_std [n] (and node_logp [n, N] when asked) with an actor,
        value [n] with a critic."""
        t = self.torch
        self._bind_stream()
        rp, ip, n, N, M = self._entity_rows(rows, index)
        new = lambda *sh: t.empty(sh, dtype=t.float32, device=rows.device)
        o = {}
        if actor is not None:
            if stored is None or not (stored.dtype == t.float32 and stored.is_contiguous()):
                raise ValueError("stored must be a contiguous float32 tensor [*, 2]")
            o.update(logp=new(n), entropy=new(n), mean=new(n), log_std=new(n))
            if node_logp:
                o["node_logp"] = new(n, N)
        if critic is not None:
            o["value"] = new(n)
        ptr = lambda x: 0 if x is None else x.data_ptr()
        self._h.entity_pointer_eval(ptr(actor), ptr(critic), rp, ip, n, N, M, ptr(stored) if actor is not None else 0, ptr(o.get("logp")),
                                    ptr(o.get("entropy")), ptr(o.get("node_logp")), ptr(o.get("mean")), ptr(o.get("log_std")), ptr(o.get("value")))
        return o

    def entity_pointer_ppo_grad(self, actor, critic, rows, index, batch, hyper, grad, stats):
        """`wrsn_entity_pointer_ppo_grad`: `entity_ppo_grad` for the node-pointer actor; batch["actions"] is the stored decisions [*, 2] and
        grad ONE contiguous float32 tensor [wrsn_entity_pointer_floats() + wrsn_entity_critic_floats()] (overwritten)."""
        VecWRSN._ppo_grad(self, True, actor, critic, rows, index, batch, hyper, grad, stats)

    def entity_adam(self, param, grad, m, v, step, lr, max_norm, beta1=0.9, beta2=0.999, eps=1e-8, norm_out=None):
        """`wrsn_entity_adam`: clip_grad_norm_(max_norm) and one Adam step in place on the block `param` with moments m, v."""
        self._bind_stream()
        self._h.entity_adam(param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), param.numel(), step, lr, beta1, beta2, eps, max_norm,
                            0 if norm_out is None else norm_out.data_ptr())

    # -- the same for several independent learners at once (wrsn_entity_ppo_grad_multi / wrsn_entity_adam_multi / wrsn_entity_ppo_update)
    def _entity_groups(self, groups, need_batch, pointer=False, critic=True):
        """Raw groups (dicts of addresses) from groups of tensors: `actor`, `critic`, `grad` (ONE contiguous float32 tensor [P_actor +
        P_critic]), `m_a`, `v_a`, `m_c`, `v_c`, `step`, and with need_batch `rows` [*, R] and `batch` (the tensors `entity_ppo_grad` takes).
        pointer: the actors are node-pointer blocks (P_actor = wrsn_entity_pointer_floats()) and `actions` the [*, 2] stored pairs.
        critic=False, the cloning calls: no critic is named, only the first P_actor floats of `grad` receive a gradient, and the stored
        pairs are the group's `stored` [rows, 2] in place of a batch.  Returns (raw groups, N, M)."""
        t = self.torch
        Pa = self._h.lib.wrsn_entity_pointer_floats() if pointer else self._h.lib.wrsn_entity_actor_floats()
        raw, N = [], 0
        for g in groups:
            q = dict(actor=g["actor"].data_ptr(), grad_actor=g["grad"].data_ptr(), adam_step=int(g.get("step", 0)))
            if critic:
                q.update(critic=g["critic"].data_ptr(), grad_critic=g["grad"].data_ptr() + 4 * Pa)
            for k, name in (("m_a", "m_actor"), ("v_a", "v_actor")) + ((("m_c", "m_critic"), ("v_c", "v_critic")) if critic else ()):
                if g.get(k) is not None:
                    q[name] = g[k].data_ptr()
            if need_batch:
                q["rows"], _, _, n_node, _ = self._entity_rows(g["rows"], None)
                if N and n_node != N:
                    raise ValueError("the groups' rows must hold the same number of nodes")
                N = n_node
                if critic:
                    b = g["batch"]
                    q.update(action=b["actions"].data_ptr(), logp_old=b["log_probs"].data_ptr(), advantage=b["advantages"].data_ptr(),
                             ret=b["returns"].data_ptr(), value_old=b["values"].data_ptr())
                else:
                    st = g["stored"]
                    if not (st.dtype == t.float32 and st.is_contiguous() and st.dim() == 2 and st.shape[1] == 2 and st.shape[0] == g["rows"].shape[0]):
                        raise ValueError("stored must be a contiguous float32 tensor [rows, 2]")
                    q["action"] = st.data_ptr()
            raw.append(q)
        return raw, N, self.num_agent

    def _entity_index(self, index, shape):
        t = self.torch
        if not (index.dtype == t.int32 and index.is_contiguous() and tuple(index.shape) == tuple(shape)):
            raise ValueError("index must be a contiguous int32 tensor %s" % (tuple(shape),))
        return index.data_ptr()

    # One implementation per shape of call.  `call`: the RawHandle method; `what`: the hyper dict or the cloning calls' ent_coef; `kind`: the
    # (pointer, critic) switches of `_entity_groups`.  The public wrappers reach them through the class, so that an object that borrows
    # single public methods of VecWRSN (the emulator adapters of tests/) needs none of them.
    def _grad_multi(self, call, groups, index, what, stats, *kind):
        self._bind_stream()
        raw, N, M = self._entity_groups(groups, True, *kind)
        n = groups[0]["rows"].shape[0] if index is None else index.shape[1]
        ip = 0 if index is None else self._entity_index(index, (len(groups), n))
        call(raw, n, N, M, ip, what, stats.data_ptr())

    def _adam_multi(self, call, groups, adam, *kind):
        self._bind_stream()
        raw, _, _ = self._entity_groups(groups, False, *kind)
        call(raw, adam)

    def _update(self, call, groups, index, minibatch, what, stats, adam, *kind):
        self._bind_stream()
        raw, N, M = self._entity_groups(groups, True, *kind)
        ip = self._entity_index(index, (len(groups),) + tuple(index.shape[1:3]))
        epochs, batch_size = int(index.shape[1]), int(index.shape[2])
        call(raw, N, M, ip, batch_size, minibatch, epochs, what, adam, stats.data_ptr())

    def entity_ppo_grad_multi(self, groups, index, hyper, stats):
        """`wrsn_entity_ppo_grad_multi`: loss and gradient of one minibatch for every group (see `_entity_groups`) in six launches.  index:
        int32 [G, n] (row index[g, i] of group g's rows) or None: all rows of every group; stats: float32 [G, 8]."""
        VecWRSN._grad_multi(self, self._h.entity_ppo_grad_multi, groups, index, hyper, stats)

    def entity_adam_multi(self, groups, lr, max_norm, beta1=0.9, beta2=0.999, eps=1e-8):
        """`wrsn_entity_adam_multi`: clip_grad_norm_(max_norm) and one Adam step on both blocks of every group, group g at `step` + 1."""
        VecWRSN._adam_multi(self, self._h.entity_adam_multi, groups, dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm))

    def entity_ppo_update(self, groups, index, minibatch, hyper, stats, lr, max_norm, beta1=0.9, beta2=0.999, eps=1e-8):
        """`wrsn_entity_ppo_update`: every epoch and minibatch of `PPOLearner.update` for every group behind one call.  index: int32
        [G, epochs, batch_size], the shuffles; stats: float32 [G, epochs * ceil(batch_size / minibatch), 8].  Only enqueues; the caller
        advances its step counts by stats.shape[1]."""
        VecWRSN._update(self, self._h.entity_ppo_update, groups, index, minibatch, hyper, stats,
                        dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm))

    # -- and for node-pointer actors (wrsn_entity_pointer_ppo_grad_multi / wrsn_entity_pointer_adam_multi / wrsn_entity_pointer_ppo_update)
    def entity_pointer_ppo_grad_multi(self, groups, index, hyper, stats):
        """`wrsn_entity_pointer_ppo_grad_multi`: `entity_ppo_grad_multi` for node-pointer actors, ten launches.  The groups' `actor` holds
        wrsn_entity_pointer_floats() floats, `grad` is [P_pointer + P_critic] and the batch's `actions` the [*, 2] stored pairs."""
        VecWRSN._grad_multi(self, self._h.entity_pointer_ppo_grad_multi, groups, index, hyper, stats, True)

    def entity_pointer_adam_multi(self, groups, lr, max_norm, beta1=0.9, beta2=0.999, eps=1e-8):
        """`wrsn_entity_pointer_adam_multi`: `entity_adam_multi` on pointer blocks, group g at `step` + 1."""
        VecWRSN._adam_multi(self, self._h.entity_pointer_adam_multi, groups, dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm), True)

    def entity_pointer_ppo_update(self, groups, index, minibatch, hyper, stats, lr, max_norm, beta1=0.9, beta2=0.999, eps=1e-8):
        """`wrsn_entity_pointer_ppo_update`: `entity_ppo_update` for node-pointer actors.  index: int32 [G, epochs, batch_size]; stats:
        float32 [G, epochs * ceil(batch_size / minibatch), 8].  Only enqueues; the caller advances its step counts by stats.shape[1]."""
        VecWRSN._update(self, self._h.entity_pointer_ppo_update, groups, index, minibatch, hyper, stats,
                        dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm), True)

    # -- behaviour cloning of node-pointer actors (wrsn_entity_pointer_bc_grad / _bc_grad_multi / _bc_update): the actor's side alone
    def entity_pointer_bc_grad(self, actor, rows, stored, index, ent_coef, grad, stats):
        """`wrsn_entity_pointer_bc_grad`: -mean(logp) - ent_coef * mean(H) of the stored pairs `stored` [*, 2] (indexed like the rows) under
        the packed node-pointer actor, its gradient into the first wrsn_entity_pointer_floats() floats of `grad` and the statistics
        (loss, -mean logp, node part, charge part, mean H, top-1, share of rows with a live stored node, 0) into stats, float32 [8]."""
        self._bind_stream()
        rp, ip, n, N, M = self._entity_rows(rows, index)
        self._h.entity_pointer_bc_grad(actor.data_ptr(), rp, ip, n, N, M, stored.data_ptr(), ent_coef, grad.data_ptr(), stats.data_ptr())

    def entity_pointer_bc_grad_multi(self, groups, index, ent_coef, stats):
        """`wrsn_entity_pointer_bc_grad_multi`: `entity_pointer_bc_grad` for every group (see `_entity_groups`, critic=False).  index: int32
        [G, n] or None: all rows of every group; stats: float32 [G, 8]."""
        VecWRSN._grad_multi(self, self._h.entity_pointer_bc_grad_multi, groups, index, ent_coef, stats, True, False)

    def entity_pointer_bc_update(self, groups, index, minibatch, ent_coef, stats, lr, max_norm, beta1=0.9, beta2=0.999, eps=1e-8):
        """`wrsn_entity_pointer_bc_update`: every epoch and minibatch of a behaviour-cloning update for every group behind one call, Adam on
        the actor blocks alone (group g from `step` + 1 on).  index: int32 [G, epochs, batch_size], the shuffles; stats: float32
        [G, epochs * ceil(batch_size / minibatch), 8].  Only enqueues; the caller advances its step counts by stats.shape[1]."""
        VecWRSN._update(self, self._h.entity_pointer_bc_update, groups, index, minibatch, ent_coef, stats,
                        dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm), True, False)

    def entity_prepare(self, groups, index, gamma, gae_lambda):
        """`wrsn_entity_prepare`: the PPO batch of every group -- the critic's values, `PPOLearner.cal_rt_adv` (gae=True) and the gathers --
        in three launches.  groups: dicts of contiguous float32 tensors under the field names of `wrsn_prepare_group`: `critic`, `state` and
        `next_state` [*, R], `reward` [*], `value`, `advantage`, `ret` [n]; optional (absent or None: NULL) `terminal` [*], `action` [*, 3],
        `logp` [*], `out_state`, `out_next_state` [n, R], `out_action` [n, 3], `out_logp`, `out_reward` [n].  index: int32 [G, n] (position i
        of group g takes row index[g, i] of ITS arrays) or None: rows 0 .. n - 1 (n = the length of `value`).  Only enqueues."""
        t = self.torch
        self._bind_stream()
        n = int(groups[0]["value"].numel()) if index is None else int(index.shape[1])
        ip = 0 if index is None else self._entity_index(index, (len(groups), n))
        raw, N = [], 0
        for g in groups:
            for k in ("state", "next_state"):
                _, _, _, n_node, _ = self._entity_rows(g[k], None)
                if N and n_node != N:
                    raise ValueError("the groups' rows must hold the same number of nodes")
                N = n_node
            q = {}
            for k, v in g.items():
                if v is None:
                    continue
                if not (v.dtype == t.float32 and v.is_contiguous()):
                    raise ValueError("%s must be a contiguous float32 tensor" % k)
                q[k] = v.data_ptr()
            raw.append(q)
        self._h.entity_prepare(raw, n, N, self.num_agent, ip, gamma, gae_lambda)

    def synchronize(self):
        self._h.sync()

    # -- read-only views for tests / logging (host copies) --------------------------------------------------
    def nodes(self):
        return self._h.nodes()

    def topology(self):
        return self._h.topology()

    def targets_active(self):
        """Network.targets_active (Network.py:9, 45-55) per environment: int32 [B, T]."""
        return self._h.targets_active()

    def mcs(self):
        return self._h.mcs()

    def env_info(self):
        return self._h.env_info()

    def counters(self):
        return self._h.counters()

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._h.close()
            self._h = None


def build_scenario_pool(scenarios, agent_type=None, num_agent=3, map_size=100, warm_up_time=100, device="cuda:0", n_node=None, n_target=None,
                        chunk=256, **capacities):
    """Records of `scenarios` right after `reset()`: a uint8 device tensor [P, record_bytes] for `VecWRSN.set_pool` of a batch with the
    same geometry (num_agent, the node / target classes of n_node / n_target, max_degree / max_cover in `capacities`).  The scenarios
    are run `chunk` at a time through a temporary VecWRSN created for n_node nodes and n_target targets (default: the largest of
    `scenarios`), so scenarios of different sizes share one pool as long as they fit."""
    import torch
    scenarios = list(scenarios)
    if not scenarios:
        raise ValueError("no scenarios")
    n_node = int(n_node) if n_node else max(s.n_node for s in scenarios)
    n_target = int(n_target) if n_target else max(s.n_target for s in scenarios)
    chunk = max(1, min(int(chunk), len(scenarios)))
    env = _PoolBuilder(scenarios[:chunk], n_node, n_target, agent_type=agent_type, num_agent=num_agent, map_size=map_size,
                       warm_up_time=warm_up_time, device=device, render=False, **capacities)
    parts = []
    try:
        for i0 in range(0, len(scenarios), chunk):
            part = scenarios[i0:i0 + chunk]
            if i0:
                env._h.set_scenarios(part, env.mc_spec)
            env.reset()
            parts.append(env.save_envs(range(len(part))))
        env.synchronize()
    finally:
        env.close()
    return torch.cat(parts, 0) if len(parts) > 1 else parts[0]


class _PoolBuilder(VecWRSN):
    """A VecWRSN whose handle is created for a stated node / target count rather than the largest of its scenarios."""

    def __init__(self, scenarios, n_node, n_target, **kw):
        self._geometry = (n_node, n_target)
        super().__init__(scenarios, **kw)

    def _sizes(self, scenarios):
        return self._geometry
