"""Shared helpers of the entity-policy tests (tests/test_entity_act.py on the emulator, tests/test_entity_act_gpu.py on the device):
memory for both sides, synthetic entity rows, actors with weights that show errors, and the reference evaluation.

Reference and tolerance.  The reference is the module itself (`build_entity_networks`) in float64 on the CPU.  No fixed number bounds the
kernel: `Ref.err32[k]` is the largest deviation of the module's own float32 CPU forward from the float64 one over the rows of the test,
per output k, and the kernel may deviate by at most 4 * err32[k] + 1e-6 -- the factor covers a different but equally long summation order
and fmaf contraction; a kernel that loses more has dropped a term.  The log-probability is held, in addition, to 1e-4 against the float64
log-density at the kernel's own action (the bound tests/test_entity_policy.py uses for the log-ratio).  That bound is tightest where
log_std sits at its lower clamp: with sigma = exp(-4) an error d of the mean enters the log-density as |eps| d / sigma, about 160 d, so
the actors of `make_actors` keep |mean| near 1 (a float32 error of a few 1e-7), not near 5."""
import copy
import math

import numpy as np

from entity_ref import GUARD, PATTERN, EntBuf

OUTS = ("action", "action_f64", "logp", "mean", "log_std")
LOG_2PI_15 = 1.5 * math.log(2.0 * math.pi)


def to_side(side, a):
    """A host array in the side's memory (kept alive by the caller)."""
    a = np.ascontiguousarray(a)
    if side.device is None:
        return a
    import torch
    return torch.from_numpy(a).to(side.device)


def addr(x):
    if x is None:
        return 0
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def sync(side):
    if side.device is not None:
        side.env.synchronize()


class OutBuf:
    """The five outputs of wrsn_entity_act for B rows, each between GUARD pattern bytes and pattern-filled, in the side's memory."""

    def __init__(self, side, B):
        self.side, self.B = side, B
        self.spec = {"action": ((B, 3), np.float32), "action_f64": ((B, 3), np.float64), "logp": ((B,), np.float32),
                     "mean": ((B, 3), np.float32), "log_std": ((B, 3), np.float32)}
        self.raw = {}
        for k, (sh, dt) in self.spec.items():
            n = int(np.prod(sh)) * np.dtype(dt).itemsize + 2 * GUARD
            if side.device is None:
                buf = np.empty(n + 16, dtype=np.uint8); off = (-buf.ctypes.data) % 16
            else:
                import torch
                buf = torch.empty(n + 16, dtype=torch.uint8, device=side.device); off = (-buf.data_ptr()) % 16
            self.raw[k] = buf[off:off + n]
        self.fill()

    def fill(self):
        for r in self.raw.values():
            r[:] = PATTERN

    def ptr(self, k):
        return addr(self.raw[k]) + GUARD

    def ptrs(self, **override):
        p = {k: self.ptr(k) for k in OUTS}; p.update(override)
        return p

    def snap(self):
        return {k: (r.copy() if isinstance(r, np.ndarray) else r.cpu().numpy()) for k, r in self.raw.items()}

    def arrays(self, snap=None):
        snap = snap or self.snap()
        return {k: snap[k][GUARD:-GUARD].view(dt).reshape(sh) for k, (sh, dt) in self.spec.items()}

    def guards_intact(self, snap):
        return all((s[:GUARD] == PATTERN).all() and (s[-GUARD:] == PATTERN).all() for s in snap.values())

    def row_untouched(self, snap, e):
        return all((snap[k][GUARD:-GUARD].reshape(self.B, -1)[e] == PATTERN).all() for k in OUTS)


def fill_entities(buf, node, mc, env):
    """Host arrays (node [B,N,8], mc [B,M,12], env [B,8], float32) into the EntBuf `buf`."""
    for k, a in (("node", node), ("mc", mc), ("env", env)):
        b = np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint8)
        r = buf.raw[k]
        if isinstance(r, np.ndarray):
            r[GUARD:-GUARD] = b
        else:
            import torch
            r[GUARD:-GUARD] = torch.from_numpy(b.copy()).to(r.device)


def synth_rows(seed, B, N, M, ids, p_alive=0.8):
    """Entity rows as the simulator lays them out, drawn from a seeded generator: node [B,N,8] (a dead node keeps u, v and is 0 elsewhere),
    mc [B,M,12] with is_self on charger ids[e], env [B,8]."""
    g = np.random.default_rng(seed)
    node = g.random((B, N, 8)).astype(np.float32)
    node[..., 2] *= 2.0
    node[..., 6] = g.integers(0, 6, (B, N))
    alive = g.random((B, N)) < p_alive
    node[..., 7] = alive
    node[..., 2:7] *= alive[..., None]
    mc = g.random((B, M, 12)).astype(np.float32)
    mc[..., 3] = 0.0
    for e in range(B):
        mc[e, max(int(ids[e]), 0) % M, 3] = 1.0
    mc[..., 4] = g.random((B, M)) < 0.8
    mc[..., 5] = g.random((B, M)) < 0.3
    mc[..., 10:] = 0.0
    env = np.zeros((B, 8), np.float32)
    env[:, :4] = 0.05 + 0.3 * g.random((B, 4))
    env[:, 4] = np.maximum(ids, 0); env[:, 5] = N
    return node, mc, env


def pack_rows(node, mc, env):
    B = node.shape[0]
    return np.concatenate([node.reshape(B, -1), mc.reshape(B, -1), env.reshape(B, -1)], 1).astype(np.float32)


_ACTORS = {}


def make_actors(M, seed=7):
    """M EntityActor modules (float32, CPU) whose parameters are re-drawn from a seeded generator: He-scaled hidden layers, a mean of
    O(1) (largest values near 1) and a log_std wide enough to leave [-4, 1] on both sides.  (The stock 0.01 last-layer init would hide errors.)"""
    key = (M, seed)
    if key not in _ACTORS:
        import torch
        from multi_agent_rl_wrsn_amd import build_entity_networks
        Actor, _ = build_entity_networks(M)
        g = torch.Generator().manual_seed(seed)
        actors = []
        for _ in range(M):
            a = Actor()
            with torch.no_grad():
                for name, lay in list(a.trunk.named_children()) + [("mean", a.mean), ("log_std", a.log_std)]:
                    k = lay.weight.shape[1]
                    scale = {"mean": 0.25, "log_std": 3.0}.get(name, math.sqrt(2.0))
                    lay.weight.copy_(torch.randn(lay.weight.shape, generator=g) * (scale / math.sqrt(k)))
                    lay.bias.copy_(torch.randn(lay.bias.shape, generator=g) * 0.1 + (-1.5 if name == "log_std" else 0.0))
            actors.append(a)
        _ACTORS[key] = actors
    return _ACTORS[key]


_PACKED = {}


def packed(M, seed=7):
    """pack_entity_actor of make_actors(M, seed): float32 [M, P] on the host."""
    key = (M, seed)
    if key not in _PACKED:
        import torch
        from multi_agent_rl_wrsn_amd import pack_entity_actor
        _PACKED[key] = torch.stack([pack_entity_actor(a) for a in make_actors(M, seed)]).numpy().copy()
    return _PACKED[key]


class Ref:
    """The module's float64 and float32 CPU forwards on packed rows [B,R] for the chargers ids [B] (rows with ids < 0 are left out) and
    draws eps [B,3] (None: zeros): `f64` / `f32` hold action, logp, mean, log_std; `err32` their largest difference per output."""

    def __init__(self, actors, rows, ids, eps=None):
        import torch
        self.rows_in = [e for e in range(len(ids)) if ids[e] >= 0]
        B = len(ids)
        eps = np.zeros((B, 3), np.float32) if eps is None else np.asarray(eps, np.float32)
        self.f64, self.f32 = self._run(actors, rows, ids, eps, torch.float64), self._run(actors, rows, ids, eps, torch.float32)
        r = self.rows_in
        self.err32 = {k: float(np.abs(self.f32[k][r] - self.f64[k][r]).max()) for k in self.f64}
        self.actors64 = None

    @staticmethod
    def _run(actors, rows, ids, eps, dtype):
        import torch
        B = len(ids)
        out = {"action": np.zeros((B, 3)), "logp": np.zeros(B), "mean": np.zeros((B, 3)), "log_std": np.zeros((B, 3))}
        with torch.no_grad():
            for a, actor in enumerate(actors):
                idx = [e for e in range(B) if ids[e] == a]
                if not idx:
                    continue
                net = copy.deepcopy(actor).to(dtype)
                mean, ls = net(torch.from_numpy(rows[idx]).to(dtype))
                ep = torch.from_numpy(eps[idx]).to(dtype)
                act = mean + ls.exp() * ep
                lp = (-0.5 * ep * ep - ls).sum(1) - torch.tensor(LOG_2PI_15, dtype=dtype)
                for k, v in (("action", act), ("logp", lp), ("mean", mean), ("log_std", ls)):
                    out[k][idx] = v.double().numpy()
        return out

    def logp64_at(self, action):
        """float64 log-density of the float64 policy at `action` [B,3]."""
        mu, ls = self.f64["mean"], self.f64["log_std"]
        z = (np.asarray(action, np.float64) - mu) / np.exp(ls)
        return (-0.5 * z * z - ls).sum(1) - LOG_2PI_15

    def check(self, got, tag="", rows=None):
        """got: arrays of OutBuf.arrays().  Every row of `rows` (default: every row that asked) in every output; returns the ratios
        deviation / err32."""
        r = self.rows_in if rows is None else rows
        ratios = {}
        for k in ("action", "logp", "mean", "log_std"):
            dev = float(np.abs(got[k][r].astype(np.float64) - self.f64[k][r]).max())
            bound = 4.0 * self.err32[k] + 1e-6
            ratios[k] = dev / max(self.err32[k], 1e-30)
            print("%s %s: deviation %.3g, err32 %.3g, ratio %.2f" % (tag, k, dev, self.err32[k], ratios[k]))
            assert dev <= bound, (tag, k, dev, self.err32[k])
        assert np.array_equal(got["action_f64"][r], got["action"][r].astype(np.float64)), (tag, "action_f64")
        d = float(np.abs(got["logp"][r] - self.logp64_at(got["action"])[r]).max())
        print("%s logp at the kernel's own action: %.3g" % (tag, d))
        assert d <= 1e-4, (tag, "logp", d)
        return ratios


class Call:
    """One wrsn_entity_act call on a side: the packed actors, ids, eps and entity rows in the side's memory, an OutBuf for the results."""

    def __init__(self, side, M, node, mc, env, ids, eps, seed=7):
        self.side, self.M = side, M
        B, N = node.shape[0], node.shape[1]
        self.B = B
        self.ent = EntBuf(B, N, M, device=side.device)
        fill_entities(self.ent, node, mc, env)
        self.actors = to_side(side, packed(M, seed))
        self.ids = to_side(side, np.asarray(ids, np.int32))
        self.eps = None if eps is None else to_side(side, np.asarray(eps, np.float32))
        self.out = OutBuf(side, B)

    def run(self, ent="own", **override):
        """ent: "own" = this call's buffers, None = the registered ones, else (node, mc, env) addresses; override: argument -> address."""
        p = dict(actors_ptr=addr(self.actors), agent_ptr=addr(self.ids), eps_ptr=addr(self.eps),
                 ent_ptrs=self.ent.ptrs() if isinstance(ent, str) else ent)
        o = self.out.ptrs()
        for k, v in override.items():
            (p if k in p else o)[k] = v
        self.side.handle.entity_act(p["actors_ptr"], p["agent_ptr"], p["eps_ptr"], p["ent_ptrs"], **o)
        sync(self.side)
        return self.out.arrays()
