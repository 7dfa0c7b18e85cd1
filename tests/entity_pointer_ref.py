"""Shared helpers of the node-pointer policy tests (tests/test_entity_pointer.py on the emulator, tests/test_entity_pointer_gpu.py on the
device): actors with weights that show errors, the reference evaluation, guarded outputs and the call on a side.

Reference and tolerance, as tests/entity_act_ref.py: the reference is the module itself (`build_entity_pointer_networks`) in float64 on
the CPU; `Ref.err32[k]` is the largest deviation of the module's own float32 CPU forward from the float64 one over the rows of the test,
both evaluated at the float64 choice of node, and the kernel may deviate by b[k] = 4 * err32[k] + 1e-6."""
import copy
import math

import numpy as np

import entity_act_ref as R
from entity_ref import GUARD, PATTERN, EntBuf

KEYS = ("node_logp", "mean", "log_std", "logp", "x", "action")
MIN_CHARGE = 0.02

_ACTORS, _PACKED = {}, {}


def make_actors(M, seed=7):
    """M EntityPointerActor modules (float32, CPU), parameters re-drawn from a seeded generator: He-scaled hidden layers, a query wide
    enough for logits that spread by several units, a charge head whose log_std leaves [-4, 1] on both sides."""
    key = (M, seed)
    if key not in _ACTORS:
        import torch
        from multi_agent_rl_wrsn_amd import build_entity_pointer_networks
        Actor, _ = build_entity_pointer_networks(M)
        g = torch.Generator().manual_seed(seed)
        actors = []
        for _ in range(M):
            a = Actor()
            with torch.no_grad():
                for name, lay in list(a.trunk.named_children()) + [("query", a.query), ("charge", a.charge)]:
                    k = lay.weight.shape[1]
                    scale = {"query": 2.0, "charge": 1.0}.get(name, math.sqrt(2.0))
                    lay.weight.copy_(torch.randn(lay.weight.shape, generator=g) * (scale / math.sqrt(k)))
                    lay.bias.copy_(torch.randn(lay.bias.shape, generator=g) * 0.1)
                a.charge.weight[0] *= 0.25                     # the mean stays O(1), as tests/entity_act_ref.py argues
                a.charge.weight[1] *= 5.0; a.charge.bias[1] -= 1.0
            actors.append(a)
        _ACTORS[key] = actors
    return _ACTORS[key]


def packed(M, seed=7):
    key = (M, seed)
    if key not in _PACKED:
        import torch
        from multi_agent_rl_wrsn_amd import pack_entity_pointer_actor
        _PACKED[key] = torch.stack([pack_entity_pointer_actor(a) for a in make_actors(M, seed)]).numpy().copy()
    return _PACKED[key]


class Ref:
    """The module's float64 and float32 CPU evaluation on packed rows [B,R] for the chargers ids [B] (rows with ids outside [0, M) are left
    out), Gumbel noise g [B,N] and draws eps [B] (None: the mode of that part).  `f64` holds node, node_logp, logits, mean, log_std, logp,
    x, action at the float64 choice; `at(node)` evaluates the float64 module at given nodes."""

    def __init__(self, actors, rows, ids, gumbel=None, eps=None, min_charge=MIN_CHARGE):
        self.actors, self.rows, self.ids, self.gumbel, self.eps, self.min_charge = actors, rows, np.asarray(ids), gumbel, eps, min_charge
        self.M = len(actors)
        self.rows_in = [e for e in range(len(ids)) if 0 <= ids[e] < self.M]
        import torch
        self.f64 = self._run(torch.float64, None)
        self.f32 = self._run(torch.float32, self.f64["node"])
        r = self.rows_in
        self.err32 = {}
        for k in KEYS + ("logits",):
            a, b = self.f32[k][r], self.f64[k][r]
            fin = np.isfinite(b)
            assert np.array_equal(fin, np.isfinite(a)), k
            self.err32[k] = float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
        self.b = {k: 4.0 * v + 1e-6 for k, v in self.err32.items()}

    def _run(self, dtype, nodes):
        import torch
        B, N = self.rows.shape[0], (self.rows.shape[1] - 12 * self.M - 8) // 8
        out = {"node": np.full(B, -2, np.int64), "node_logp": np.zeros((B, N)), "logits": np.zeros((B, N)), "mean": np.zeros(B), "log_std": np.zeros(B),
               "logp": np.zeros(B), "x": np.zeros(B), "action": np.zeros((B, 3))}
        with torch.no_grad():
            for a, actor in enumerate(self.actors):
                idx = [e for e in range(B) if self.ids[e] == a]
                if not idx:
                    continue
                net = copy.deepcopy(actor).to(dtype)
                rows = torch.from_numpy(self.rows[idx]).to(dtype)
                g = None if self.gumbel is None else torch.from_numpy(self.gumbel[idx]).to(dtype)
                ep = torch.zeros(len(idx), dtype=dtype) if self.eps is None else torch.from_numpy(self.eps[idx]).to(dtype)
                z, l, nlp, alive, nd, mcs, env = net.scores(rows)
                k = net.choose(l, alive, g) if nodes is None else torch.from_numpy(np.asarray(nodes)[idx]).long()
                mu, ls, _ = net.charge_head(z, nd, k)
                x = mu + ls.exp() * ep
                c = self.min_charge + (1.0 - self.min_charge) * torch.sigmoid(x)
                lp = net._node_term(nlp, k) + (-0.5 * ep * ep - ls - 0.5 * math.log(2.0 * math.pi))
                act = torch.cat([net.destination(nd, mcs, env, k), c.unsqueeze(1)], 1)
                for key, v in (("node", k), ("node_logp", nlp), ("logits", l), ("mean", mu), ("log_std", ls), ("logp", lp), ("x", x), ("action", act)):
                    out[key][idx] = v.double().numpy() if key != "node" else v.numpy()
        return out

    def at(self, nodes):
        import torch
        return self._run(torch.float64, nodes)

    def perturbed(self):
        """float64 l + g [B,N] (-inf for nodes that are not alive)."""
        return self.f64["logits"] + (0.0 if self.gumbel is None else self.gumbel.astype(np.float64))

    def check_scores(self, got, tag=""):
        """Test 1 on the arrays of OutBuf.arrays(): everything within b of the reference evaluated at the kernel's own node."""
        r = self.rows_in
        at = self.at(np.where(got["node"] < -1, -1, got["node"]))
        ninf = np.isneginf(self.f64["node_logp"][r])
        assert np.array_equal(np.isneginf(got["node_logp"][r]), ninf), (tag, "node_logp -inf")
        want = {"node_logp": at["node_logp"], "mean": at["mean"], "log_std": at["log_std"], "logp": at["logp"], "x": at["x"], "action": at["action"]}
        have = {"node_logp": got["node_logp"], "mean": got["charge_mean"], "log_std": got["charge_log_std"], "logp": got["logp"],
                "x": got["stored"][:, 1], "action": got["action"]}
        for k in KEYS:
            a, b = have[k][r].astype(np.float64), want[k][r]
            fin = np.isfinite(b)
            dev = float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
            print("%s %s: deviation %.3g, err32 %.3g, bound %.3g" % (tag, k, dev, self.err32[k], self.b[k]))
            assert np.isfinite(a[fin]).all() and dev <= self.b[k], (tag, k, dev, self.err32[k])
        assert np.array_equal(got["action_f64"][r], got["action"][r].astype(np.float64)), (tag, "action_f64")
        assert np.array_equal(got["stored"][r, 0], got["node"][r].astype(np.float32)), (tag, "stored[:, 0]")

    def check_choice(self, got, tag=""):
        """Test 2: the chosen node is alive and its float64 perturbed score is within 2 b of the maximum; on rows whose float64 gap
        between best and runner-up exceeds 2 b the node is the reference's.  Returns the share of such rows."""
        r = np.array(self.rows_in)
        sc = self.perturbed()[r]
        node = got["node"][r]
        has = np.isfinite(sc).any(1)
        assert (node[~has] == -1).all() and (node[has] >= 0).all(), tag
        tol = 2.0 * self.b["logits"]
        top2 = -np.sort(-sc, axis=1)[:, :2]
        with np.errstate(invalid="ignore"):                   # a row with one alive node: -inf as runner-up; with none: -inf - -inf
            clear = has & ((top2[:, 0] - top2[:, 1]) > tol)
        for j in np.nonzero(has)[0]:
            assert np.isfinite(sc[j, node[j]]), (tag, "dead node chosen", r[j])
            assert sc[j, node[j]] >= top2[j, 0] - tol, (tag, r[j], sc[j, node[j]], top2[j, 0])
        assert np.array_equal(node[clear], self.f64["node"][r][clear]), tag
        return float(clear.mean())


OUT_SPEC = lambda B, N: {"node": ((B,), np.int32), "stored": ((B, 2), np.float32), "action": ((B, 3), np.float32), "action_f64": ((B, 3), np.float64),
                         "logp": ((B,), np.float32), "node_logp": ((B, N), np.float32), "charge_mean": ((B,), np.float32),
                         "charge_log_std": ((B,), np.float32)}
OUTS = ("node", "stored", "action", "action_f64", "logp", "node_logp", "charge_mean", "charge_log_std")


class OutBuf(R.OutBuf):
    """The eight outputs of wrsn_entity_pointer_act for B rows of N nodes, each between GUARD pattern bytes and pattern-filled."""

    def __init__(self, side, B, N):
        self.side, self.B = side, B
        self.spec = OUT_SPEC(B, N)
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

    def ptrs(self, **override):
        p = {k: self.ptr(k) for k in OUTS}; p.update(override)
        return p

    def row_untouched(self, snap, e):
        return all((snap[k][GUARD:-GUARD].reshape(self.B, -1)[e] == PATTERN).all() for k in OUTS)


class Call:
    """One wrsn_entity_pointer_act call on a side: packed actors, ids, noise and entity rows in the side's memory, an OutBuf."""

    def __init__(self, side, M, node, mc, env, ids, gumbel, eps, seed=7):
        self.side, self.M = side, M
        B, N = node.shape[0], node.shape[1]
        self.B = B
        self.ent = EntBuf(B, N, M, device=side.device)
        R.fill_entities(self.ent, node, mc, env)
        self.actors = R.to_side(side, packed(M, seed))
        self.ids = R.to_side(side, np.asarray(ids, np.int32))
        self.gumbel = None if gumbel is None else R.to_side(side, np.asarray(gumbel, np.float32))
        self.eps = None if eps is None else R.to_side(side, np.asarray(eps, np.float32))
        self.out = OutBuf(side, B, N)

    def run(self, ent="own", min_charge=MIN_CHARGE, **override):
        p = dict(actors_ptr=R.addr(self.actors), agent_ptr=R.addr(self.ids), gumbel_ptr=R.addr(self.gumbel), eps_ptr=R.addr(self.eps),
                 ent_ptrs=self.ent.ptrs() if isinstance(ent, str) else ent, min_charge=min_charge)
        o = self.out.ptrs()
        for k, v in override.items():
            (p if k in p else o)[k] = v
        self.side.handle.entity_pointer_act(p["actors_ptr"], p["agent_ptr"], p["gumbel_ptr"], p["eps_ptr"], p["min_charge"], p["ent_ptrs"], **o)
        R.sync(self.side)
        return self.out.arrays()


def gumbel_noise(seed, B, N):
    u = np.random.default_rng(seed).random((B, N))
    return (-np.log(-np.log(np.clip(u, 1e-12, 1.0 - 1e-12)))).astype(np.float32)


def emu_pointer_vec(side):
    """tests/episode_ref.py's adapter plus `entity_pointer_act`, as VecWRSN offers it: what BatchedEntityPointerIPPO and PointerPolicy use."""
    import episode_ref as E
    from multi_agent_rl_wrsn_amd import VecWRSN
    base = type(E.emu_eval_vec(side))

    class EmuPointerVec(base):
        def entity_pointer_act(self, *a, **kw): return VecWRSN.entity_pointer_act(self, *a, **kw)

    return EmuPointerVec(side)
