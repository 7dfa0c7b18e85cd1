"""Shared helpers of the entity-update tests (tests/test_entity_update.py on the emulator, tests/test_entity_update_gpu.py on the device):
nets with weights that show errors, guarded memory and the three calls on a side, the reference, the kink margins, and the adapter that
lets the trainer reach the new calls on the emulator.

Reference and tolerance (as tests/entity_act_ref.py).  The reference is the product's own module and `PPOLearner.minibatch_loss` on float64
copies on the CPU; `err32[k]` is the largest deviation of the same computation in float32 on the CPU, per output tensor k.  Forward outputs
and statistics may deviate by 4 * err32[k] + 1e-6, a gradient tensor by 4 * err32[k] + 1e-6 * max|g64[k]|.

Kinks.  A pre-activation near 0 or a maximum near its runner-up flips a derivative from 0 to 1, and float64, float32 and the kernel may
then differ by whole terms.  `Ref.margins` holds, per kind of kink, (smallest float64 margin, err32 of that quantity); `assert_margins`
demands margin > 8 * err32 + 2e-6 -- twice the forward allowance -- before a gradient is compared.  The seeds of GRAD_CASES were chosen on
the CPU (`find_seed`) so that it holds."""
import copy
import math

import numpy as np

import entity_act_ref as R
from entity_ref import GUARD, PATTERN

STATS = ("loss", "pg", "v_loss", "entropy", "approx_kl", "clipfrac")
HYPER = dict(clip=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=True, clip_vloss=True)
P_ACTOR, P_CRITIC = 49224, 48580

_NETS = {}


def make_nets(M, seed=11):
    """(EntityActor, EntityCritic) for M chargers, float32 on the CPU: the actor is make_actors' first (He-scaled hidden layers, mean of
    O(1), log_std leaving [-4, 1] on both sides), the critic re-drawn the same way with a `value` layer of O(1)."""
    key = (M, seed)
    if key not in _NETS:
        import torch
        from multi_agent_rl_wrsn_amd import build_entity_networks
        actor = R.make_actors(M)[0]
        _, Critic = build_entity_networks(M)
        g = torch.Generator().manual_seed(seed)
        c = Critic()
        with torch.no_grad():
            for name, lay in list(c.trunk.named_children()) + [("value", c.value)]:
                k = lay.weight.shape[1]
                scale = 1.0 if name == "value" else math.sqrt(2.0)
                lay.weight.copy_(torch.randn(lay.weight.shape, generator=g) * (scale / math.sqrt(k)))
                lay.bias.copy_(torch.randn(lay.bias.shape, generator=g) * 0.1)
        _NETS[key] = (actor, c)
    return _NETS[key]


def named_layers(net):
    t = net.trunk
    tail = [("value", net.value)] if hasattr(net, "value") else [("mean", net.mean), ("log_std", net.log_std)]
    return [(k, getattr(t, k)) for k in ("node1", "node2", "mc1", "mc2", "head1", "head2")] + tail


def block_slices(net):
    """name -> slice of the packed block for every weight ("node1.w") and bias ("node1.b"), in block order."""
    out, o = {}, 0
    for name, lay in named_layers(net):
        out[name + ".w"] = slice(o, o + lay.weight.numel()); o += lay.weight.numel()
        out[name + ".b"] = slice(o, o + lay.bias.numel()); o += lay.bias.numel()
    return out


def grad_block(net, floats):
    """The gradients of `net`'s parameters in the layout of its packed block (float64 numpy, padding zero)."""
    g, o = np.zeros(floats), 0
    for _, lay in named_layers(net):
        for p, tr in ((lay.weight, True), (lay.bias, False)):
            gr = p.grad if p.grad is not None else p.new_zeros(p.shape)
            g[o:o + p.numel()] = (gr.t() if tr else gr).reshape(-1).double().numpy(); o += p.numel()
    return g


def pack(net):
    from multi_agent_rl_wrsn_amd import pack_entity_actor, pack_entity_critic
    return (pack_entity_critic if hasattr(net, "value") else pack_entity_actor)(net).numpy().copy()


def make_rows(seed, n, N, M, p_alive=0.8):
    ids = np.zeros(n, np.int32)
    return R.pack_rows(*R.synth_rows(seed, n, N, M, ids, p_alive))


def make_batch(seed, rows, actor, critic):
    """Batch arrays for `rows`: actions drawn from the policy, stored log-probabilities that put the ratio below, inside and above the
    clip range, advantages of both signs, returns and old values on both sides of the new value by less and by more than clip."""
    import torch
    n = rows.shape[0]
    g = np.random.default_rng(seed)
    with torch.no_grad():
        r64 = torch.from_numpy(rows).double()
        mean, ls = copy.deepcopy(actor).double()(r64)
        v = copy.deepcopy(critic).double()(r64).sum(1).numpy()
    mean, ls = mean.numpy(), ls.numpy()
    action = mean + np.exp(ls) * g.standard_normal(mean.shape)
    z = (action - mean) / np.exp(ls)
    logp = (-0.5 * z * z - ls).sum(1) - R.LOG_2PI_15
    shift = np.resize(np.array([-0.5, 0.3, -0.05, 0.04, 0.5, -0.3, 0.0, 0.1]), n) + 0.01 * g.standard_normal(n)
    adv = np.resize(np.array([1.0, -1.0, 1.0, 1.0, -1.0, -1.0]), n) * (0.3 + g.random(n) * 2.0)
    ret = v + g.choice([-1.0, 1.0], n) * (0.05 + g.random(n))
    vold = v + np.resize(np.array([0.07, -0.5, 0.9, -0.1]), n) * (0.8 + 0.4 * g.random(n))
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(action=f(action), logp_old=f(logp - shift), advantage=f(adv), ret=f(ret), value_old=f(vold))


class _Learner:
    """What PPOLearner.minibatch_loss needs of `self`, around one actor and one critic."""

    def __init__(self, actor, critic, hyper):
        import torch
        from multi_agent_rl_wrsn_amd.ippo import EntityPPOLearner
        self.torch, self.actors, self.critics, self._cls = torch, [actor], [critic], EntityPPOLearner
        self._logp_dims = EntityPPOLearner._logp_dims
        for k, v in hyper.items():
            setattr(self, k, v)

    def _forward(self, net, x, inference=False): return net(x)
    def evaluate(self, *a): return self._cls.evaluate(self, *a)
    def get_value(self, *a): return self._cls.get_value(self, *a)
    def minibatch_loss(self, *a): return self._cls.minibatch_loss(self, *a)


def trace(net, rows, M):
    """Every quantity of `net` on `rows` that sits at a kink, computed with the statements of build_entity_networks._Trunk.forward:
    pre-activations p1, p2 (nodes), q1, q2 (chargers), z1, z2 (head), the two largest values of every pooled unit, the raw last layer."""
    import torch
    import torch.nn.functional as F
    from multi_agent_rl_wrsn_amd import _lib
    from multi_agent_rl_wrsn_amd.ippo import EntityTransitionBuffers
    t = net.trunk
    lin = lambda layer, x: torch.bmm(x, layer.weight.t().unsqueeze(0).expand(x.shape[0], -1, -1)) + layer.bias
    with torch.no_grad():
        nodes, mcs, env = EntityTransitionBuffers.split(rows, M)
        alive = nodes[..., _lib.ENT_NODE["alive"]] == 1
        x = torch.where(alive.unsqueeze(-1), nodes, torch.zeros_like(nodes))
        p1 = lin(t.node1, x); p2 = lin(t.node2, F.relu(p1)); h = F.relu(p2)
        w = alive.unsqueeze(-1).to(h.dtype); cnt = w.sum(1)
        mean = (h * w).sum(1) / cnt.clamp(min=1.0)
        hm = h.masked_fill(~alive.unsqueeze(-1), float("-inf"))
        top = hm.topk(2, 1).values                            # [n, 2, 64]
        mx = torch.where(cnt > 0, top[:, 0], torch.zeros_like(top[:, 0]))
        q1 = lin(t.mc1, mcs); q2 = lin(t.mc2, F.relu(q1)); g = F.relu(q2)
        cw = (mcs[..., _lib.ENT_MC["alive"]] == 1).unsqueeze(-1).to(g.dtype)
        cmean = (g * cw).sum(1) / cw.sum(1).clamp(min=1.0)
        own = (g * (mcs[..., _lib.ENT_MC["is_self"]] == 1).unsqueeze(-1).to(g.dtype)).sum(1)
        scale = torch.ones(_lib.ENT_ENV_F, dtype=env.dtype)
        scale[_lib.ENT_ENV["agent"]] = 1.0 / M; scale[_lib.ENT_ENV["n_node"]] = 1.0 / max(1, nodes.shape[1])
        feat = torch.cat([mean, mx, cmean, own, env * scale], 1).unsqueeze(1)
        z1 = lin(t.head1, feat); z2 = lin(t.head2, F.relu(z1))
        out = dict(p1=p1[alive], p2=p2[alive], q1=q1, q2=q2, z1=z1, z2=z2, top=top)
        if hasattr(net, "log_std"):
            out["raw_ls"] = lin(net.log_std, F.relu(z2))
    return {k: v.double().numpy() for k, v in out.items()}


class Ref:
    """float64 and float32 CPU evaluations of (actor, critic) on `rows` [n, R] (the minibatch, in order) with `batch` [n] under `hyper`:
    forward outputs, statistics, gradients in block layout, err32 per tensor, and the kink margins.  batch None: forward only."""

    def __init__(self, actor, critic, rows, batch, hyper, M):
        import torch
        self.M, self.hyper = M, dict(hyper)
        out, stats, grad, tr = {}, {}, {}, {}
        for dt in (torch.float64, torch.float32):
            a, c = copy.deepcopy(actor).to(dt), copy.deepcopy(critic).to(dt)
            r = torch.from_numpy(rows).to(dt)
            mean, ls = a(r); v = c(r).sum(1)
            out[dt] = dict(mean=mean.detach().double().numpy(), log_std=ls.detach().double().numpy(), value=v.detach().double().numpy())
            if batch is None:
                continue
            b = dict(states=r, actions=torch.from_numpy(batch["action"]).to(dt), log_probs=torch.from_numpy(batch["logp_old"]).to(dt),
                     advantages=torch.from_numpy(batch["advantage"]).to(dt), returns=torch.from_numpy(batch["ret"]).to(dt),
                     values=torch.from_numpy(batch["value_old"]).to(dt))
            res = _Learner(a, c, hyper).minibatch_loss(0, b, torch.arange(rows.shape[0]))
            stats[dt] = np.array([float(x.detach()) if hasattr(x, "detach") else float(x) for x in res])
            res[0].backward()
            grad[dt] = (grad_block(a, P_ACTOR), grad_block(c, P_CRITIC))
            q = {"a." + k: x for k, x in trace(a, r, M).items()}
            q.update({"c." + k: x for k, x in trace(c, r, M).items()})
            with torch.no_grad():
                z = (b["actions"] - mean) / ls.exp()
                q["ratio"] = (((-0.5 * z * z - ls).sum(1) - R.LOG_2PI_15) - b["log_probs"]).exp().double().numpy()
                dv = v - b["values"]
                q["dv"] = dv.double().numpy()
                q["v_diff"] = ((v - b["returns"]) ** 2 - (b["values"] + dv.clamp(-hyper["clip"], hyper["clip"]) - b["returns"]) ** 2).double().numpy()
            tr[dt] = q
        f64, f32 = torch.float64, torch.float32
        self.f64, self.f32 = out[f64], out[f32]
        self.err32 = {k: float(np.abs(self.f32[k] - self.f64[k]).max()) for k in self.f64}
        if batch is not None:
            self.stats64, self.stats32 = stats[f64], stats[f32]
            self.err32_stats = np.abs(self.stats32 - self.stats64)
            self.g64, self.g32 = grad[f64], grad[f32]
            self.q64, self.q32 = tr[f64], tr[f32]
            self.margins = self._margins()

    def _margins(self):
        a, b, clip = self.q64, self.q32, self.hyper["clip"]
        m = {}
        err = lambda k: float(np.abs(a[k] - b[k]).max())
        for tag in ("a.", "c."):
            for k in ("p1", "p2", "q1", "q2", "z1", "z2"):
                m[tag + k] = (float(np.abs(a[tag + k]).min()), err(tag + k))
            top, top32 = a[tag + "top"], b[tag + "top"]
            pos = top[:, 0] > 0                               # pooled units with a maximum > 0: the gap to the runner-up (ReLU outputs, >= 0; -inf: dead)
            gap, gap32 = (top[:, 0] - np.maximum(top[:, 1], 0.0))[pos], (top32[:, 0] - np.maximum(top32[:, 1], 0.0))[pos]
            if gap.size:
                m[tag + "max"] = (float(gap.min()), float(np.abs(gap - gap32).max()))
        r = a["ratio"]
        m["ratio"] = (float(np.minimum(np.abs(r - (1 - clip)), np.abs(r - (1 + clip))).min()), err("ratio"))
        m["log_std"] = (float(np.minimum(np.abs(a["a.raw_ls"] + 4.0), np.abs(a["a.raw_ls"] - 1.0)).min()), err("a.raw_ls"))
        if self.hyper["clip_vloss"]:
            m["dv"] = (float(np.abs(np.abs(a["dv"]) - clip).min()), err("dv"))
            differ = np.abs(a["dv"]) > clip                   # where the two value terms differ as functions
            if differ.any():
                m["v_terms"] = (float(np.abs(a["v_diff"][differ]).min()), float(np.abs(a["v_diff"] - b["v_diff"])[differ].max()))
        return m

    def margins_clear(self):
        return all(mg > 8.0 * e + 2e-6 for mg, e in self.margins.values())

    def assert_margins(self, tag=""):
        for k, (mg, e) in self.margins.items():
            print("%s margin %-9s %.3g  (err32 %.3g)" % (tag, k, mg, e))
            assert mg > 8.0 * e + 2e-6, (tag, k, mg, e)

    def check_forward(self, got, tag="", keys=("mean", "log_std", "value")):
        for k in keys:
            dev = float(np.abs(got[k].astype(np.float64) - self.f64[k]).max())
            print("%s %s: deviation %.3g, err32 %.3g" % (tag, k, dev, self.err32[k]))
            assert dev <= 4.0 * self.err32[k] + 1e-6, (tag, k, dev, self.err32[k])

    def check_stats(self, stats, tag=""):
        e = float(self.err32_stats.max())                     # `stats` is one output tensor: err32 is the largest deviation over its entries
        for i, k in enumerate(STATS):
            dev = abs(float(stats[i]) - self.stats64[i])
            print("%s %s: %.9g (float64 %.9g) deviation %.3g, its own err32 %.3g, err32 of stats %.3g" % (tag, k, stats[i], self.stats64[i], dev, self.err32_stats[i], e))
        for i, k in enumerate(STATS):
            dev = abs(float(stats[i]) - self.stats64[i])
            assert dev <= 4.0 * e + 1e-6, (tag, k, dev, e)
        assert np.float32(stats[5]) == np.float32(self.stats64[5]), (tag, "clipfrac", stats[5], self.stats64[5])
        assert stats[6] == 0 and stats[7] == 0

    def check_grads(self, ga, gc, nets, tag=""):
        for which, got, net in ((0, ga, nets[0]), (1, gc, nets[1])):
            g64, g32 = self.g64[which], self.g32[which]
            sl_all = block_slices(net)
            for name, sl in sl_all.items():
                e = float(np.abs(g32[sl] - g64[sl]).max()); mx = float(np.abs(g64[sl]).max())
                dev = float(np.abs(got[sl].astype(np.float64) - g64[sl]).max())
                print("%s %s %-9s deviation %.3g, err32 %.3g, max|g| %.3g" % (tag, ("actor", "critic")[which], name, dev, e, mx))
                assert dev <= 4.0 * e + 1e-6 * mx, (tag, which, name, dev, e, mx)
            assert (got[max(s.stop for s in sl_all.values()):] == 0).all(), (tag, "padding")


def find_seed(n, N, M, hyper=HYPER, tries=40, first=0):
    """The first seed >= first whose rows and batch clear the kink margins for make_nets(M) (CPU only)."""
    actor, critic = make_nets(M)
    for seed in range(first, first + tries):
        rows = make_rows(seed, n, N, M)
        if Ref(actor, critic, rows, make_batch(seed, rows, actor, critic), hyper, M).margins_clear():
            return seed
    return None


# ------------------------------------------------------------------------------------------------ memory and calls on a side
class Guarded:
    """A buffer of `shape` / `dtype` between GUARD pattern bytes, 16-byte aligned, pattern-filled, in the side's memory."""

    def __init__(self, side, shape, dtype=np.float32, data=None, shift=0):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        n = self.nbytes + 2 * GUARD
        if side.device is None:
            buf = np.empty(n + 32, dtype=np.uint8); off = (-buf.ctypes.data) % 16 + shift
        else:
            import torch
            buf = torch.empty(n + 32, dtype=torch.uint8, device=side.device); off = (-buf.data_ptr()) % 16 + shift
        self.raw = buf[off:off + n]
        self.fill()
        if data is not None:
            self.set(data)

    def fill(self):
        self.raw[:] = PATTERN

    def set(self, data):
        b = np.ascontiguousarray(data, dtype=self.dtype).reshape(-1).view(np.uint8)
        assert b.size == self.nbytes
        if isinstance(self.raw, np.ndarray):
            self.raw[GUARD:GUARD + self.nbytes] = b
        else:
            import torch
            self.raw[GUARD:GUARD + self.nbytes] = torch.from_numpy(b.copy()).to(self.raw.device)

    @property
    def ptr(self):
        return R.addr(self.raw) + GUARD

    def snap(self):
        return self.raw.copy() if isinstance(self.raw, np.ndarray) else self.raw.cpu().numpy()

    def get(self):
        return self.snap()[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape).copy()

    def guards_intact(self):
        s = self.snap()
        return bool((s[:GUARD] == PATTERN).all() and (s[GUARD + self.nbytes:] == PATTERN).all())

    def untouched(self):
        return bool((self.snap() == PATTERN).all())


class Job:
    """Blocks, rows, batch and outputs of one minibatch in the side's memory, and the three calls on them."""

    def __init__(self, side, nets, rows, batch, N, M, index=None, hyper=HYPER):
        self.side, self.N, self.M, self.hyper = side, N, M, dict(hyper)
        self.n = rows.shape[0] if index is None else len(index)
        self.n_all = rows.shape[0]
        self.actor = Guarded(side, (P_ACTOR,), data=pack(nets[0]))
        self.critic = Guarded(side, (P_CRITIC,), data=pack(nets[1]))
        self.rows = Guarded(side, rows.shape, data=rows)
        self.index = None if index is None else Guarded(side, (len(index),), np.int32, data=np.asarray(index, np.int32))
        self.batch = None if batch is None else {k: Guarded(side, v.shape, data=v) for k, v in batch.items()}
        self.mean, self.log_std, self.value = Guarded(side, (self.n, 3)), Guarded(side, (self.n, 3)), Guarded(side, (self.n,))
        self.ga, self.gc, self.stats = Guarded(side, (P_ACTOR,)), Guarded(side, (P_CRITIC,)), Guarded(side, (8,))
        self.outs = (self.mean, self.log_std, self.value, self.ga, self.gc, self.stats)

    def fill(self):
        for o in self.outs:
            o.fill()

    def eval(self, actor=True, critic=True, **over):
        p = dict(actor_ptr=self.actor.ptr if actor else 0, critic_ptr=self.critic.ptr if critic else 0, rows_ptr=self.rows.ptr,
                 index_ptr=self.index.ptr if self.index is not None else 0, n=self.n, n_node=self.N, n_mc=self.M,
                 mean=self.mean.ptr if actor else 0, log_std=self.log_std.ptr if actor else 0, value=self.value.ptr if critic else 0)
        p.update(over)
        self.side.handle.entity_eval(**p)
        R.sync(self.side)
        return dict(mean=self.mean.get(), log_std=self.log_std.get(), value=self.value.get())

    def grad(self, **over):
        p = dict(actor_ptr=self.actor.ptr, critic_ptr=self.critic.ptr, rows_ptr=self.rows.ptr,
                 index_ptr=self.index.ptr if self.index is not None else 0, n=self.n, n_node=self.N, n_mc=self.M,
                 grad_actor=self.ga.ptr, grad_critic=self.gc.ptr, stats=self.stats.ptr)
        p.update({k: b.ptr for k, b in self.batch.items()})
        p.update(self.hyper)
        p.update(over)
        self.side.handle.entity_ppo_grad(**p)
        R.sync(self.side)
        return self.ga.get(), self.gc.get(), self.stats.get()


# ------------------------------------------------------------------------------------------------ the trainer on the emulator
class EmuTrainVec:
    """tests/sides.py's EmuVec plus the three update calls, as VecWRSN offers them: what BatchedEntityIPPO(fused_update=True) uses."""

    def __init__(self, side):
        from sides import EmuVec
        self._v = EmuVec(side)

    def __getattr__(self, k):
        return getattr(self._v, k)

    def _entity_rows(self, *a):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN._entity_rows(self, *a)

    def entity_eval(self, *a, **kw):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN.entity_eval(self, *a, **kw)

    def entity_ppo_grad(self, *a, **kw):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN.entity_ppo_grad(self, *a, **kw)

    def entity_adam(self, *a, **kw):
        from multi_agent_rl_wrsn_amd import VecWRSN
        return VecWRSN.entity_adam(self, *a, **kw)
