"""TEST INFRASTRUCTURE -- the two backends behind one driver, and the helpers every test module shares.

EmuSide runs the CPU-emulated build of the product kernels (tests/emu/libwrsn_emu.so) through the same C-ABI binding the product uses,
with numpy arrays standing in for device memory; VecSide runs VecWRSN on the device.  Both take VecWRSN's constructor keywords and hand
back plain numpy, so one body holds both to the same assertions.  The body lives in the family's CPU module and takes the side; the test
of that module runs it on EmuSide and the test of the `_gpu` module (marked gpu) on VecSide, each under the name it has always had:

    def x_matches(Side, ...): side = Side(scenarios, mc, M, ...); side.reset(); side.step(ids, actions); side.decision(0) ...
    def test_emulated_x(...): x_matches(EmuSide, ...)          # tests/test_x.py
    def test_x(...): body.x_matches(VecSide, ...)              # tests/test_x_gpu.py

What a side offers: reset / step / view / decision / rows / density_action / render_state / save_envs / load_envs / clone_envs /
set_pool / pool_reset / pool_info / out_ptrs / entity_buffers / set_entity_out / entities / handle / close.  EmuVec puts the part of VecWRSN's
interface that the trainers of ippo.py use on top of an EmuSide."""
import glob
import os
import random

import numpy as np

from conftest import load_golden

FIELDS = ("agent_id", "reward", "terminal", "now", "status")
PGP_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prob_gp")
PGP_NAMES = sorted(os.path.splitext(os.path.basename(f))[0] for f in glob.glob(os.path.join(PGP_DIR, "*.npz")))


def need_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_MT = {}


def python_mt_state(seed, n):
    """The 625 words of random.getstate()[1] after random.seed(seed) and n draws of random.random(), as uint32.  The generator of a seed
    is kept, so asking for growing n (after every decision of a replay) draws every number once."""
    r, taken = _MT.get(seed, (None, n + 1))
    if taken > n:
        r, taken = random.Random(seed), 0
    for _ in range(n - taken):
        r.random()
    _MT[seed] = (r, n)
    return np.array(r.getstate()[1], dtype=np.uint32)


def scenario_from_prob_gp(z, seed=None, stochastic=True, prob_gp=None):
    """(Scenario, charger spec) of a fixture whose packets are (or, with stochastic=True, are treated as) drawn: seed64 of the fixture,
    else its seed, unless `seed` is given; `prob_gp` replaces the fixture's."""
    from multi_agent_rl_wrsn_amd.scenario import MC_SPEC_KEYS, NODE_SPEC_KEYS, Scenario
    ns = {k: float(v) for k, v in zip(NODE_SPEC_KEYS, z["node_spec"])}
    if prob_gp is not None:
        ns["prob_gp"] = prob_gp
    mc = {k: float(v) for k, v in zip(MC_SPEC_KEYS, z["mc_spec"])}
    if seed is None:
        seed = int(z["seed64"]) if "seed64" in z.files else int(z["seed"])
    return Scenario(z["node_xy"], z["target_xy"], z["bs_xy"], ns, float(z["max_time"]), seed, stochastic_packets=stochastic), mc


def load_fixture(name):
    """(npz, Scenario, charger spec) of tests/golden/<name>.npz, or of tests/golden/prob_gp/<rest>.npz for "prob_gp/<rest>"."""
    if name.startswith("prob_gp/"):
        z = np.load(os.path.join(PGP_DIR, name.split("/", 1)[1] + ".npz"))
        return (z,) + scenario_from_prob_gp(z)
    from multi_agent_rl_wrsn_amd.scenario import scenario_from_golden
    z = load_golden(name)
    return (z,) + scenario_from_golden(z)


def aligned(shape):
    """A zeroed uint8 array whose first byte is 16-byte aligned (device records are)."""
    n = int(np.prod(shape))
    buf = np.zeros(n + 16, dtype=np.uint8)
    off = (-buf.ctypes.data) % 16
    return buf[off:off + n].reshape(shape)


def decision_dict(req, obs, h, e=0, sc=None, with_nodes=True):
    """The dict parity.check_decision takes for the request of environment e: `req` holds the request rows (arrays or tensors by
    field), `obs` the float64 observation of the row (or None), `h` is the RawHandle (synchronised); node and target arrays are cut to
    scenario `sc` when given."""
    g = {"agent_id": int(req["agent_id"][e]), "now": float(req["now"][e]), "reward": float(req["reward"][e]), "terminal": bool(req["terminal"][e]),
         "obs": obs}
    if with_nodes:
        n, t = (sc.n_node, sc.n_target) if sc is not None else (None, None)
        nd = h.nodes(); m = h.mcs()
        g.update(node_energy=nd["energy"][e][:n], node_cs=nd["cs"][e][:n], node_status=nd["status"][e][:n],
                 mc_energy=m["energy"][e], mc_loc=np.stack([m["loc_x"][e], m["loc_y"][e]], 1), mc_status=m["status"][e],
                 mc_charging=m["type_charging"][e], mc_nconn=m["n_conn"][e], excl=m["excl"][e], prev_minfit=m["prev_minfit"][e],
                 min_fitness=float(h.env_info()["min_fitness"][e]), targets_active=h.targets_active()[e][:t])
    return g


class _Side:
    """What both backends answer from the request rows (`_host()`: numpy copies of FIELDS), `obs_row(e)` and the handle's peek views."""

    def view(self):
        h = self.handle
        v = self._host()
        v.update(nodes=h.nodes(), mcs=h.mcs(), env_info=h.env_info(), obs=(self.obs_row if self.render else None))
        return v

    def rows(self):
        """The request rows: one tuple (agent, now, reward, terminal, status) per environment."""
        r = self._host()
        return [(int(r["agent_id"][e]), float(r["now"][e]), float(r["reward"][e]), int(r["terminal"][e]), int(r["status"][e])) for e in range(self.B)]

    def decision(self, e=0, sc=None, with_nodes=True):
        """decision_dict of environment e; node and target arrays cut to scenario `sc` (default: the one the side was built with -- pass
        the record's after a load or a pool swap)."""
        return decision_dict(self._host(), self.obs_row(e) if self.render else None, self.handle, e, sc or self.scenarios[e], with_nodes)

    def nodes(self): return self.handle.nodes()
    def topology(self): return self.handle.topology()
    def targets_active(self): return self.handle.targets_active()
    def mcs(self): return self.handle.mcs()
    def env_info(self): return self.handle.env_info()
    def pool_info(self): return self.handle.pool_info()

    def entity_buffers(self):
        """Guarded, pattern-filled entity buffers (entity_ref.EntBuf) in this side's memory."""
        from entity_ref import EntBuf
        return EntBuf(self.B, self.N, self.M, device=self.device)

    def set_entity_out(self, buf=None):
        """Register the buffers of an EntBuf on the handle; None drops them."""
        self.handle.set_entity_out(*(buf.ptrs() if buf is not None else ()))


class EmuSide(_Side):
    """B environments on the emulated library: what VecWRSN does with torch tensors, on numpy arrays (`agent_id`, `reward`, `terminal`,
    `now`, `status`, `obs` are the arrays the library writes).  Keywords as VecWRSN's, except that observation reuse is on by default --
    the same obs array is passed call after call and never modified -- and that `n_node` / `n_target` may state the handle's geometry
    (default: the largest scenario's, as VecWRSN).  `reset` and `step` take `with_obs` / `auto_reset` to depart from the constructor's
    render / auto_reset for one call."""
    name, device = "emu", None

    def __init__(self, scenarios, mc_spec, num_agent, map_size=100, warm_up_time=100.0, auto_reset=False, render=True, step_budget=0,
                 step_deadline_us=0, reuse_obs=True, obs_dtype="float32", entities=False, max_degree=0, max_cover=0, n_node=None, n_target=None):
        from emu_env import emu_lib
        from multi_agent_rl_wrsn_amd import _lib
        self.scenarios = list(scenarios)
        self.B = len(scenarios)
        self.N = n_node or max(s.n_node for s in scenarios); self.T = n_target or max(s.n_target for s in scenarios)
        self.M, self.G = num_agent, map_size
        self.auto_reset, self.render = bool(auto_reset), bool(render)
        self.h = self.handle = _lib.RawHandle(emu_lib(), self.B, self.N, self.T, num_agent, map_size, warm_up_time, 0, max_degree, max_cover)
        bf16 = {"float32": False, "bfloat16": True}[obs_dtype]
        if bf16: self.h.set_obs_format(_lib.OBS_BF16)
        if reuse_obs and self.render: self.h.set_obs_reuse(True)
        if step_budget: self.h.set_step_budget(step_budget)
        if step_deadline_us: self.h.set_step_deadline(step_deadline_us)
        self.h.set_scenarios(scenarios, mc_spec)
        B, G = self.B, self.G
        self.agent_id = np.full(B, -1, dtype=np.int32); self.reward = np.zeros(B); self.terminal = np.zeros(B, dtype=np.uint8)
        self.now = np.zeros(B); self.status = np.zeros(B, dtype=np.int32)
        self.obs = np.zeros((B, 4, G, G), dtype=np.uint16 if bf16 else np.float32)
        self.ent = None
        if entities:
            self.ent = self.entity_buffers(); self.set_entity_out(self.ent)

    def _ptrs(self, with_obs=None):
        with_obs = self.render if with_obs is None else with_obs
        return dict(agent_id=self.agent_id.ctypes.data, reward=self.reward.ctypes.data, terminal=self.terminal.ctypes.data,
                    now=self.now.ctypes.data, status=self.status.ctypes.data, obs=(self.obs.ctypes.data if with_obs else 0))

    def _host(self):
        return {k: getattr(self, k).copy() for k in FIELDS}

    def out_ptrs(self):
        """Addresses of the request rows by field, and obs = 0: what the raw handle's calls take as their `out`."""
        return self._ptrs(False)

    def obs_row(self, e):
        o = self.obs[e]
        if o.dtype == np.uint16:
            o = (o.astype(np.uint32) << 16).view(np.float32)
        return o.astype(np.float64)

    def reset(self, mask=None, with_obs=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self.h.reset(0 if m is None else m.ctypes.data, **self._ptrs(with_obs))

    def step(self, agent_ids, actions, with_obs=None, auto_reset=None):
        a = np.ascontiguousarray(agent_ids, dtype=np.int32); act = np.ascontiguousarray(actions, dtype=np.float64).reshape(self.B, 3)
        if self._pool is not None and self.auto_reset:        # as VecWRSN.step: terminal rows restart in a drawn record and are marked -2
            a = a.copy()
            self.h.pool_reset(0, 0, a.ctypes.data, **self._ptrs(with_obs))
        self.h.step(a.ctypes.data, act.ctypes.data, self.auto_reset if auto_reset is None else auto_reset, **self._ptrs(with_obs))

    def density_action(self, agent_ids, maps):
        a = np.ascontiguousarray(agent_ids, dtype=np.int32); m = np.ascontiguousarray(maps, dtype=np.float64); out = np.zeros((self.B, 3))
        self.h.density_action(a.ctypes.data, m.ctypes.data, out.ctypes.data)
        return out

    def render_state(self, agent_ids):
        a = np.ascontiguousarray(agent_ids, dtype=np.int32); out = np.zeros_like(self.obs)
        self.h.render(a.ctypes.data, out.ctypes.data)
        return out

    def save_envs(self, envs=None):
        idx = np.arange(self.B, dtype=np.int32) if envs is None else np.asarray(envs, dtype=np.int32)
        rec = aligned((len(idx), self.h.env_record_bytes()))
        p = self._ptrs(False); p.pop("obs")
        self.h.save_envs(idx, rec.ctypes.data, **p)
        return rec

    def load_envs(self, records, envs=None, with_obs=None):
        idx = np.arange(len(records), dtype=np.int32) if envs is None else np.asarray(envs, dtype=np.int32)
        self.h.load_envs(idx, records.ctypes.data, **self._ptrs(with_obs))

    def clone_envs(self, src, dst, with_obs=None):
        self.h.clone_envs(src, dst, **self._ptrs(with_obs))

    _pool = None

    def set_pool(self, records, seed=0):
        self._pool = records                                  # kept alive and unchanged while the handle reads it
        self.h.pool_set(0 if records is None else records.ctypes.data, 0 if records is None else len(records), seed)

    def pool_reset(self, mask=None, index=None, with_obs=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        self.h.pool_reset(0 if m is None else m.ctypes.data, 0 if i is None else i.ctypes.data, 0, **self._ptrs(with_obs))

    def entities(self, agent_ids, buf):
        """wrsn_entities for `agent_ids` into the EntBuf `buf`."""
        a = np.ascontiguousarray(agent_ids, dtype=np.int32)
        self.h.entities(a.ctypes.data, *buf.ptrs())

    def close(self):
        self.h.close()


class EmuVec:
    """What the batched trainers and the transition buffers use of a VecWRSN, on an EmuSide that renders (float32), has entities, or
    both: CPU tensors that share the memory the emulated library writes."""

    def __init__(self, side):
        import torch
        from entity_ref import GUARD
        self.torch, self.device, self.side = torch, torch.device("cpu"), side
        self.num_env, self.num_agent, self.n_node, self.map_size = side.B, side.M, side.N, side.G
        self.entities, self.auto_reset, self._h = side.ent is not None, side.auto_reset, side.handle
        self.state = torch.from_numpy(side.obs) if side.render else None
        self._t = {k: torch.from_numpy(getattr(side, k)) for k in FIELDS}
        self.nodes_feat = self.chargers_feat = self.env_feat = None
        if self.entities:
            raw, shp = side.ent.raw, side.ent.shapes
            self.nodes_feat, self.chargers_feat, self.env_feat = (
                torch.from_numpy(raw[k][GUARD:-GUARD].view(np.float32).reshape(shp[k])) for k in ("node", "mc", "env"))
        self._act = None

    def _bind_stream(self):
        pass

    def _out_ptrs(self):
        return self.side._ptrs()

    def _result(self):
        r = dict(self._t); r.update(state=self.state, nodes=self.nodes_feat, chargers=self.chargers_feat, env_feat=self.env_feat)
        return r

    def reset(self):
        self.side.reset(); return self._result()

    def step(self, ids, actions):
        self.side.step(ids.numpy(), actions.numpy()); return self._result()

    def density_to_action(self, ids, dmaps):
        return self.torch.from_numpy(self.side.density_action(ids.numpy(), dmaps.numpy()))

    def entity_act(self, ids, packed, eps=None):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN.entity_act(self, ids, packed, eps)


class VecSide(_Side):
    """VecWRSN (the device) behind the same interface: the Python layer stays under test, and every call synchronises before anything
    is read."""
    name = "gpu"

    def __init__(self, scenarios, mc_spec, num_agent, **kw):
        self.torch = need_gpu()
        from multi_agent_rl_wrsn_amd import VecWRSN
        self.env = env = VecWRSN(scenarios, mc_spec, num_agent, **kw)
        self.scenarios = env.scenarios
        self.B, self.N, self.T, self.M, self.G = env.num_env, env.n_node, env.n_target, env.num_agent, env.map_size
        self.render, self.device, self.handle = env.render, env.device, env._h

    def _t(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))

    def _host(self):
        self.env.synchronize()
        return {k: getattr(self.env, k).cpu().numpy() for k in FIELDS}

    def obs_row(self, e):
        return self.env.state[e].double().cpu().numpy()

    def out_ptrs(self):
        return dict(self.env._out_ptrs(), obs=0)

    def reset(self, mask=None):
        self.env.reset(None if mask is None else self._t(mask, np.uint8)); self.env.synchronize()

    def step(self, agent_ids, actions):
        self.env.step(self._t(agent_ids, np.int32), self._t(actions, np.float64).reshape(self.B, 3)); self.env.synchronize()

    def density_action(self, agent_ids, maps):
        out = self.env.density_to_action(self._t(agent_ids, np.int32), self._t(maps, np.float64)); self.env.synchronize()
        return out.cpu().numpy()

    def render_state(self, agent_ids):
        out = self.env.render_state(self._t(agent_ids, np.int32)); self.env.synchronize()
        return out.view(self.torch.int16).cpu().numpy().view(np.uint16) if out.dtype == self.torch.bfloat16 else out.cpu().numpy()

    def save_envs(self, envs=None):
        return self.env.save_envs(envs)

    def load_envs(self, records, envs=None):
        self.env.load_envs(records, envs); self.env.synchronize()

    def clone_envs(self, src, dst):
        self.env.clone_envs(src, dst); self.env.synchronize()

    def set_pool(self, records, seed=0):
        self.env.set_pool(records, seed)

    def pool_reset(self, mask=None, index=None):
        self.env.pool_reset(None if mask is None else self._t(mask, np.uint8), None if index is None else self._t(index, np.int32))
        self.env.synchronize()

    def entities(self, agent_ids, buf):
        a = self._t(agent_ids, np.int32).to(self.device)
        self.handle.entities(a.data_ptr(), *buf.ptrs()); self.env.synchronize()

    def close(self):
        self.env.close()

