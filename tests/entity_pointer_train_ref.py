"""Shared helpers of the node-pointer update tests (tests/test_entity_pointer_update.py on the emulator,
tests/test_entity_pointer_update_gpu.py on the device): nets, stored decisions and batches that show errors, the calls on a side, the
reference and the kink margins.

Reference and tolerance are those of tests/entity_train_ref.py.  The reference is `EntityPointerActor.forward`, `EntityCritic.forward` and
`PPOLearner.minibatch_loss` on float64 copies on the CPU; `err32[k]` is the largest deviation of the same computation in float32 on the CPU,
per output tensor k.  Forward outputs and statistics may deviate by 4 * err32[k] + 1e-6, a gradient tensor by 4 * err32[k] + 1e-6 *
max|g64[k]|.  A gradient is compared only when every kink's float64 margin exceeds 8 * err32 + 2e-6 (`assert_margins`): the ReLU
pre-activations of alive nodes and of the two head layers, the pooled maximum against its runner-up, the ratio against 1 +- clip, the
value terms, and s_raw (the charge head's log_std before the clamp) against -4 and 1.  The seeds of the cases were chosen on the CPU
(`find_seed`) so that the reference alone meets them."""
import copy

import numpy as np

import entity_act_ref as R
import entity_pointer_ref as P
import entity_train_ref as T
from entity_train_ref import Guarded, HYPER, STATS, P_CRITIC

P_ACTOR = 56980
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)
_NETS = {}


def make_nets(M, seed=23):
    """(EntityPointerActor, EntityCritic), float32 on the CPU: the trunk of tests/entity_pointer_ref.py's first actor, `query` and `charge`
    re-drawn with a standard deviation of 0.3 (not the initial 0.01: the softmax is far from uniform); the critic of
    tests/entity_train_ref.py.  One bias serves every row of a call, so s_raw is moved beyond the clamp row by row through the input the
    charge head alone sees (`clamp_rows`)."""
    key = (M, seed)
    if key not in _NETS:
        import torch
        a = copy.deepcopy(P.make_actors(M)[0])
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for lay in (a.query, a.charge):
                lay.weight.copy_(torch.randn(lay.weight.shape, generator=g) * 0.3)
                lay.bias.copy_(torch.randn(lay.bias.shape, generator=g) * 0.1)
        _NETS[key] = (a, T.make_nets(M)[1])
    return _NETS[key]


S_LOW, S_HIGH = -5.5, 2.5                                     # where the shifted rows put s_raw: 1.5 beyond either end of the clamp [-4, 1]


def clamp_rows(rows, actor, N, M):
    """A per-row shift of the charge head's bias.  Row 0 (and row 1 when there are at least four rows) gets node 0 dead and stored: a dead
    node's features reach nothing but x_k, the charge head's own input, so its first seven floats are set along charge.weight[1, 128:135]
    to whatever puts s_raw at S_LOW (row 0) or S_HIGH (row 1).  Returns (rows, {row: 0})."""
    import torch
    rows = rows.copy()
    n = rows.shape[0]
    targets = {0: S_LOW, 1: S_HIGH} if n >= 4 else {0: S_HIGH}
    for r in targets:
        rows[r, 0:8] = 0.0                                    # node 0: dead, features zero
    a = copy.deepcopy(actor).double()
    with torch.no_grad():
        z = a.scores(torch.from_numpy(rows).double())[0].squeeze(1)
        s0 = (z @ a.charge.weight[1, :128] + a.charge.bias[1]).numpy()     # s_raw with x_k = 0
        w = a.charge.weight[1, 128:135].numpy()
    for r, target in targets.items():
        rows[r, 0:7] = ((target - s0[r]) * w / (w * w).sum()).astype(np.float32)
    return rows, {r: 0 for r in targets}


def named_layers(net):
    t = net.trunk
    tail = [("value", net.value)] if hasattr(net, "value") else [("query", net.query), ("charge", net.charge)]
    return [(k, getattr(t, k)) for k in ("node1", "node2", "mc1", "mc2", "head1", "head2")] + tail


def block_slices(net):
    out, o = {}, 0
    for name, lay in named_layers(net):
        out[name + ".w"] = slice(o, o + lay.weight.numel()); o += lay.weight.numel()
        out[name + ".b"] = slice(o, o + lay.bias.numel()); o += lay.bias.numel()
    return out


def grad_block(net, floats):
    g, o = np.zeros(floats), 0
    for _, lay in named_layers(net):
        for p, tr in ((lay.weight, True), (lay.bias, False)):
            gr = p.grad if p.grad is not None else p.new_zeros(p.shape)
            g[o:o + p.numel()] = (gr.t() if tr else gr).reshape(-1).double().numpy(); o += p.numel()
    return g


def pack(net):
    from multi_agent_rl_wrsn_amd import pack_entity_critic, pack_entity_pointer_actor
    return (pack_entity_critic if hasattr(net, "value") else pack_entity_pointer_actor)(net).numpy().copy()


make_rows = T.make_rows


def clean_node(stored, N):
    """The node the kernel and the module see for stored[:, 0]: NaN, infinities and indices outside [0, N) are -1."""
    kf = stored[:, 0].astype(np.float64)
    ok = np.isfinite(kf)
    k = np.where(ok, np.trunc(np.where(ok, kf, 0.0)), -1).astype(np.int64)
    return np.where((k >= 0) & (k < N), k, -1)


def make_stored(seed, rows, actor, M, force=None):
    """Decisions for `rows` [n, R]: a node sampled from the policy (so alive, -1 where no node is alive; `force` {row: node} overrides it)
    and x = mu + exp(s) eps at that node."""
    import torch
    n = rows.shape[0]
    N = (rows.shape[1] - 12 * M - 8) // 8
    g = np.random.default_rng(seed + 1000)
    a = copy.deepcopy(actor).double()
    with torch.no_grad():
        r64 = torch.from_numpy(rows).double()
        z, l, _, alive, nodes, _, _ = a.scores(r64)
        k = a.choose(l, alive, torch.from_numpy(P.gumbel_noise(seed, n, N)).double())
        for r, node in (force or {}).items():
            k[r] = node
        mu, ls, _ = a.charge_head(z, nodes, k)
        x = mu + ls.exp() * torch.from_numpy(g.standard_normal(n))
    return np.ascontiguousarray(np.stack([k.numpy().astype(np.float64), x.numpy()], 1), np.float32)


def make_batch(seed, rows, stored, actor, critic, M):
    """As tests/entity_train_ref.py's: stored log-probabilities that put the ratio below, inside and above the clip range, advantages of
    both signs, returns and old values on both sides of the new value by less and by more than clip."""
    import torch
    n = rows.shape[0]
    N = (rows.shape[1] - 12 * M - 8) // 8
    g = np.random.default_rng(seed)
    with torch.no_grad():
        r64 = torch.from_numpy(rows).double()
        logp, _ = copy.deepcopy(actor).double()(r64, torch.from_numpy(clean_node(stored, N)), torch.from_numpy(stored[:, 1]).double())
        v = copy.deepcopy(critic).double()(r64).sum(1).numpy()
    shift = np.resize(np.array([-0.5, 0.3, -0.05, 0.04, 0.5, -0.3, 0.0, 0.1]), n) + 0.01 * g.standard_normal(n)
    adv = np.resize(np.array([1.0, -1.0, 1.0, 1.0, -1.0, -1.0]), n) * (0.3 + g.random(n) * 2.0)
    ret = v + g.choice([-1.0, 1.0], n) * (0.05 + g.random(n))
    vold = v + np.resize(np.array([0.07, -0.5, 0.9, -0.1]), n) * (0.8 + 0.4 * g.random(n))
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(stored=f(stored), logp_old=f(logp.numpy() - shift), advantage=f(adv), ret=f(ret), value_old=f(vold))


class _Learner(T._Learner):
    def __init__(self, actor, critic, hyper):
        super().__init__(actor, critic, hyper)
        from multi_agent_rl_wrsn_amd.ippo import EntityPointerPPOLearner
        self._cls = EntityPointerPPOLearner


class Ref:
    """float64 and float32 CPU evaluations of (actor, critic) on `rows` [n, R] (the minibatch, in order) with the decisions `stored` [n, 2]
    and `batch` under `hyper`: forward outputs, statistics, gradients in block layout, err32 per tensor, the kink margins.  batch None:
    forward only."""

    def __init__(self, actor, critic, rows, stored, batch, hyper, M):
        import torch
        self.M, self.hyper = M, dict(hyper)
        N = (rows.shape[1] - 12 * M - 8) // 8
        node = torch.from_numpy(clean_node(stored, N))
        out, stats, grad, tr = {}, {}, {}, {}
        for dt in (torch.float64, torch.float32):
            a, c = copy.deepcopy(actor).to(dt), copy.deepcopy(critic).to(dt)
            r = torch.from_numpy(rows).to(dt)
            x = torch.from_numpy(stored[:, 1]).to(dt)
            logp, ent = a(r, node, x)
            z, _, nlp, alive, nodes, _, _ = a.scores(r)
            mu, ls, xk = a.charge_head(z, nodes, node)
            s_raw = (torch.cat([z, xk.unsqueeze(1)], 2).squeeze(1) @ a.charge.weight.t() + a.charge.bias)[:, 1]
            v = c(r).sum(1)
            nl = torch.where(alive, nlp, torch.zeros_like(nlp))       # compared on the alive nodes; the others are -inf by a select
            out[dt] = {k: t.detach().double().numpy() for k, t in dict(logp=logp, entropy=ent, mean=mu, log_std=ls, value=v, node_logp=nl).items()}
            self.alive = alive.numpy()
            if batch is None:
                continue
            st = torch.stack([node.to(dt), x], 1)
            b = dict(states=r, actions=st, log_probs=torch.from_numpy(batch["logp_old"]).to(dt),
                     advantages=torch.from_numpy(batch["advantage"]).to(dt), returns=torch.from_numpy(batch["ret"]).to(dt),
                     values=torch.from_numpy(batch["value_old"]).to(dt))
            res = _Learner(a, c, hyper).minibatch_loss(0, b, torch.arange(rows.shape[0]))
            stats[dt] = np.array([float(y.detach()) if hasattr(y, "detach") else float(y) for y in res])
            res[0].backward()
            grad[dt] = (grad_block(a, P_ACTOR), grad_block(c, P_CRITIC))
            q = {"a." + k: y for k, y in T.trace(a, r, M).items()}
            q.update({"c." + k: y for k, y in T.trace(c, r, M).items()})
            with torch.no_grad():
                q["ratio"] = (logp - b["log_probs"]).exp().double().numpy()
                dv = v - b["values"]
                q["dv"] = dv.double().numpy()
                q["v_diff"] = ((v - b["returns"]) ** 2 - (b["values"] + dv.clamp(-hyper["clip"], hyper["clip"]) - b["returns"]) ** 2).double().numpy()
                q["s_raw"] = s_raw.double().numpy()
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
            pos = top[:, 0] > 0
            gap, gap32 = (top[:, 0] - np.maximum(top[:, 1], 0.0))[pos], (top32[:, 0] - np.maximum(top32[:, 1], 0.0))[pos]
            if gap.size:
                m[tag + "max"] = (float(gap.min()), float(np.abs(gap - gap32).max()))
        r = a["ratio"]
        m["ratio"] = (float(np.minimum(np.abs(r - (1 - clip)), np.abs(r - (1 + clip))).min()), err("ratio"))
        m["s_raw"] = (float(np.minimum(np.abs(a["s_raw"] + 4.0), np.abs(a["s_raw"] - 1.0)).min()), err("s_raw"))
        if self.hyper["clip_vloss"]:
            m["dv"] = (float(np.abs(np.abs(a["dv"]) - clip).min()), err("dv"))
            differ = np.abs(a["dv"]) > clip
            if differ.any():
                m["v_terms"] = (float(np.abs(a["v_diff"][differ]).min()), float(np.abs(a["v_diff"] - b["v_diff"])[differ].max()))
        return m

    margins_clear = T.Ref.margins_clear
    assert_margins = T.Ref.assert_margins
    check_stats = T.Ref.check_stats

    def check_forward(self, got, tag="", keys=("logp", "entropy", "mean", "log_std", "value")):
        for k in keys:
            dev = float(np.abs(got[k].astype(np.float64) - self.f64[k]).max())
            print("%s %s: deviation %.3g, err32 %.3g" % (tag, k, dev, self.err32[k]))
            assert dev <= 4.0 * self.err32[k] + 1e-6, (tag, k, dev, self.err32[k])

    def check_grads(self, ga, gc, nets, tag=""):
        """Every tensor of both blocks; all are printed before the first failure is raised, so the `query`, `charge` and trunk slices each
        show on their own."""
        bad = []
        for which, got, net in ((0, ga, nets[0]), (1, gc, nets[1])):
            g64, g32 = self.g64[which], self.g32[which]
            sl_all = block_slices(net)
            for name, sl in sl_all.items():
                e = float(np.abs(g32[sl] - g64[sl]).max()); mx = float(np.abs(g64[sl]).max())
                dev = float(np.abs(got[sl].astype(np.float64) - g64[sl]).max())
                print("%s %s %-9s deviation %.3g, err32 %.3g, max|g| %.3g, fraction of the bound %.2f" %
                      (tag, ("actor", "critic")[which], name, dev, e, mx, dev / (4.0 * e + 1e-6 * mx) if mx > 0 else 0.0))
                if not dev <= 4.0 * e + 1e-6 * mx:
                    bad.append((tag, ("actor", "critic")[which], name, dev, e, mx))
            assert (got[max(s.stop for s in sl_all.values()):] == 0).all(), (tag, "padding")
        assert not bad, bad


def case(seed, n, N, M, hyper=HYPER):
    nets = make_nets(M)
    rows, force = clamp_rows(make_rows(seed, n, N, M), nets[0], N, M)
    stored = make_stored(seed, rows, nets[0], M, force)
    batch = make_batch(seed, rows, stored, nets[0], nets[1], M)
    return nets, rows, batch, Ref(nets[0], nets[1], rows, stored, batch, hyper, M)


def find_seed(n, N, M, hyper=HYPER, tries=60, first=0):
    """The first seed >= first whose case clears the kink margins one and a half times over (CPU only): err32 is a float32 run of the
    host's own kernels and moves a little from host to host, and the tests assert the margins themselves."""
    for seed in range(first, first + tries):
        if all(mg > 1.5 * (8.0 * e + 2e-6) for mg, e in case(seed, n, N, M, hyper)[3].margins.values()):
            return seed
    return None


class Job:
    """Blocks, rows, decisions, batch and outputs of one minibatch in the side's memory, and the two calls on them."""

    def __init__(self, side, nets, rows, batch, N, M, index=None, hyper=HYPER, stored=None):
        self.side, self.N, self.M, self.hyper = side, N, M, dict(hyper)
        self.n = rows.shape[0] if index is None else len(index)
        self.actor = Guarded(side, (P_ACTOR,), data=pack(nets[0]))
        self.critic = Guarded(side, (P_CRITIC,), data=pack(nets[1]))
        self.rows = Guarded(side, rows.shape, data=rows)
        self.index = None if index is None else Guarded(side, (len(index),), np.int32, data=np.asarray(index, np.int32))
        self.batch = None if batch is None else {k: Guarded(side, v.shape, data=v) for k, v in batch.items()}
        self.stored = self.batch["stored"] if batch is not None else Guarded(side, stored.shape, data=stored)
        n = self.n
        self.fwd = dict(logp=Guarded(side, (n,)), entropy=Guarded(side, (n,)), node_logp=Guarded(side, (n, N)), charge_mean=Guarded(side, (n,)),
                        charge_log_std=Guarded(side, (n,)), value=Guarded(side, (n,)))
        self.ga, self.gc, self.stats = Guarded(side, (P_ACTOR,)), Guarded(side, (P_CRITIC,)), Guarded(side, (8,))
        self.outs = tuple(self.fwd.values()) + (self.ga, self.gc, self.stats)
        self.inputs = (self.actor, self.critic, self.rows, self.stored) + (() if batch is None else tuple(self.batch.values()))

    def fill(self):
        for o in self.outs:
            o.fill()

    def eval(self, actor=True, critic=True, **over):
        p = dict(actor_ptr=self.actor.ptr if actor else 0, critic_ptr=self.critic.ptr if critic else 0, rows_ptr=self.rows.ptr,
                 index_ptr=self.index.ptr if self.index is not None else 0, n=self.n, n_node=self.N, n_mc=self.M,
                 stored=self.stored.ptr if actor else 0, value=self.fwd["value"].ptr if critic else 0)
        p.update({k: (b.ptr if actor else 0) for k, b in self.fwd.items() if k != "value"})
        p.update(over)
        self.side.handle.entity_pointer_eval(**p)
        R.sync(self.side)
        g = {k: b.get() for k, b in self.fwd.items()}
        g["mean"], g["log_std"] = g["charge_mean"], g["charge_log_std"]
        return g

    def grad(self, **over):
        p = dict(actor_ptr=self.actor.ptr, critic_ptr=self.critic.ptr, rows_ptr=self.rows.ptr,
                 index_ptr=self.index.ptr if self.index is not None else 0, n=self.n, n_node=self.N, n_mc=self.M,
                 grad_actor=self.ga.ptr, grad_critic=self.gc.ptr, stats=self.stats.ptr)
        p.update({k: b.ptr for k, b in self.batch.items()})
        p.update(self.hyper)
        p.update(over)
        self.side.handle.entity_pointer_ppo_grad(**p)
        R.sync(self.side)
        return self.ga.get(), self.gc.get(), self.stats.get()


def emu_update_vec(side):
    """tests/entity_pointer_ref.py's adapter plus the update calls, as VecWRSN offers them: what
    BatchedEntityPointerIPPO(device_update=True) uses on the emulator."""
    from multi_agent_rl_wrsn_amd import VecWRSN
    base = type(P.emu_pointer_vec(side))

    class EmuPointerUpdateVec(base):
        def _entity_rows(self, *a): return VecWRSN._entity_rows(self, *a)
        def entity_eval(self, *a, **kw): return VecWRSN.entity_eval(self, *a, **kw)
        def entity_pointer_eval(self, *a, **kw): return VecWRSN.entity_pointer_eval(self, *a, **kw)
        def entity_pointer_ppo_grad(self, *a, **kw): return VecWRSN.entity_pointer_ppo_grad(self, *a, **kw)
        def entity_adam(self, *a, **kw): return VecWRSN.entity_adam(self, *a, **kw)

    return EmuPointerUpdateVec(side)
