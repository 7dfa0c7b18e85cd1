"""Batched independent-PPO roll-out and training on top of `VecWRSN` (f2 roll-out glue, f4 data-parallel
training).  Counterpart of the reference's `controller/ippo/IPPO.py` for B environments per GPU instead of one:

  reference (one environment, Python lists)                       here (B environments, device buffers)
  ------------------------------------------------------------    ------------------------------------------------------
  roll_out bookkeeping            IPPO.py:119-156                  `TransitionBuffers` + HIP kernels behind the C-ABI
                                                                   (`wrsn_rollout_record` / `wrsn_rollout_collect`)
  first transition dropped        IPPO.py:146-147                  a charger without a pending action appends nothing
  cal_rt_adv                      IPPO.py:71-93                    `BatchedIPPO.cal_rt_adv` (stored terminals are all False,
                                                                   so returns == rewards, advantages = r - V(s))
  outlier batch selection         IPPO.py:193-209                  `select_batch` (same index arithmetic, same numpy calls)
  UNet actor / CNN critic         controller/ppo/actor/UnetActor.py:61-80, critic/CNNCritic.py:7-49   `UNet`, `CNNCritic`
                                                                   (same parameter names and shapes: reference
                                                                   checkpoints load with load_state_dict)
  PPO update                      IPPO.py:225-271                  `BatchedIPPO.update` (+ one all-reduce of the flattened
                                                                   actor/critic gradients per minibatch when data-parallel)

torch is used for the policy networks and for device memory; everything that touches environment state goes through
the C-ABI.  What differs from the reference by construction: actions are sampled for all environments of a launch that
carry a request for that charger in one forward pass, so BatchNorm statistics are taken over that batch (the reference
runs the actor on batches of one, in training mode); logging goes to CSV (tensorboard is not a dependency).
"""
import math
import os
import time
import warnings

import numpy as np

from . import _lib


def _torch():
    import torch
    return torch


# ------------------------------------------------------------------------------------------------------------------
# policy networks (PyTorch): same architecture, parameter names and initialisation as the reference's
# ------------------------------------------------------------------------------------------------------------------
def _ortho(layer, std=math.sqrt(2.0), bias=0.0):
    """utils.py:19-22 layer_init: orthogonal weights, constant bias."""
    torch = _torch()
    torch.nn.init.orthogonal_(layer.weight, std)
    torch.nn.init.constant_(layer.bias, bias)
    return layer


def build_networks(map_size=100):
    """Returns (UNet, CNNCritic) classes bound to `map_size` (the reference hard-codes 100 x 100)."""
    torch = _torch()
    nn = torch.nn
    F = torch.nn.functional

    class _Block(nn.Module):                                 # conv 3x3 + BatchNorm + ReLU   (UnetActor.py:6-17)
        def __init__(self, cin, cout):
            super().__init__()
            self.conv = _ortho(nn.Conv2d(cin, cout, kernel_size=3, padding=1))
            self.bn = nn.BatchNorm2d(cout)

        def forward(self, x):
            return F.relu(self.bn(self.conv(x)), inplace=True)

    class _Down(nn.Module):                                  # max-pool 2 then block          (UnetActor.py:19-30)
        def __init__(self, cin, cout):
            super().__init__()
            self.conv_block = _Block(cin, cout)

        def forward(self, x):
            return self.conv_block(F.max_pool2d(x, 2))

    class _Up(nn.Module):                                    # bilinear x2, pad to the skip, concat, block   (UnetActor.py:33-47)
        def __init__(self, cin, cout):
            super().__init__()
            self.conv_block = _Block(cin, cout)

        def forward(self, low, skip):
            low = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=True)
            dy, dx = skip.shape[2] - low.shape[2], skip.shape[3] - low.shape[3]
            low = F.pad(low, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
            return self.conv_block(torch.cat([skip, low], dim=1))

    class _Out(nn.Module):                                   # conv 3x3, small init            (UnetActor.py:50-58)
        def __init__(self, cin, cout):
            super().__init__()
            self.conv = _ortho(nn.Conv2d(cin, cout, kernel_size=3, padding=1), std=0.1)

        def forward(self, x):
            return self.conv(x)

    class UNet(nn.Module):
        """Actor: 4 x G x G observation -> per-cell mean of a G x G density map + a learned log-std map (UnetActor.py:61-80)."""

        def __init__(self):
            super().__init__()
            self.inc = _Block(4, 64)
            self.down1 = _Down(64, 128)
            self.down2 = _Down(128, 256)
            self.up1 = _Up(384, 128)
            self.up2 = _Up(192, 64)
            self.out_mean = _Out(64, 1)
            self.log_std = nn.Parameter(torch.zeros((1, 1, map_size, map_size)))

        def forward(self, x):
            x1 = self.inc(x); x2 = self.down1(x1); x3 = self.down2(x2)
            mean = self.out_mean(self.up2(self.up1(x3, x2), x1))
            return mean[:, 0], self.log_std.expand_as(mean)[:, 0]      # [n, G, G] each (the reference squeezes: same for n > 1)

    class CNNCritic(nn.Module):
        """Critic: three 5x5 stride-2 convolutions, two linear layers (CNNCritic.py:7-49)."""

        def __init__(self):
            super().__init__()
            self.conv1 = _ortho(nn.Conv2d(4, 16, kernel_size=5, stride=2, padding=2))
            self.conv2 = _ortho(nn.Conv2d(16, 32, kernel_size=5, stride=2, padding=2))
            self.conv3 = _ortho(nn.Conv2d(32, 64, kernel_size=5, stride=2, padding=2))
            n = map_size
            for _ in range(3):
                n = (n - 1) // 2 + 1
            self.fc1 = _ortho(nn.Linear(64 * n * n, 100))                # 10816 inputs at G = 100
            self.fc2 = _ortho(nn.Linear(100, 1), std=1.0)

        def forward(self, x):
            x = F.relu(self.conv1(x)); x = F.relu(self.conv2(x)); x = F.relu(self.conv3(x))
            return self.fc2(F.relu(self.fc1(x.flatten(1))))

    return UNet, CNNCritic


# ------------------------------------------------------------------------------------------------------------------
# device-side transition buffers
# ------------------------------------------------------------------------------------------------------------------
class _TransitionBuffers:
    """What the two kinds of transition buffers share: the twelve tensors of `wrsn_transition_buffers`, the ctypes struct over them and
    the calls that do not depend on what a stored state row is.  A subclass states the shape and dtype of a state row and which
    `_lib.RawHandle` calls `record` and `collect` go to."""

    def __init__(self, env, capacity, action_elems, row_shape, row_dtype):
        torch = env.torch
        self.env = env
        B, M, C, A = env.num_env, env.num_agent, int(capacity), int(action_elems)
        self.capacity, self.action_elems = C, A
        dev = env.device
        f32 = dict(dtype=torch.float32, device=dev)
        row = dict(dtype=row_dtype, device=dev)
        self.pend_state = torch.zeros((B, M) + row_shape, **row)
        self.pend_action = torch.zeros((B, M, A), **f32)
        self.pend_logp = torch.zeros((B, M), **f32)
        self.pend_valid = torch.zeros((B, M), dtype=torch.uint8, device=dev)
        self.state = torch.zeros((M, C) + row_shape, **row)
        self.action = torch.zeros((M, C, A), **f32)
        self.next_state = torch.zeros((M, C) + row_shape, **row)
        self.reward = torch.zeros((M, C), **f32)
        self.logp = torch.zeros((M, C), **f32)
        self.now = torch.zeros((M, C), dtype=torch.float64, device=dev)
        self.env_index = torch.zeros((M, C), dtype=torch.int32, device=dev)
        self.count = torch.zeros((M,), dtype=torch.int32, device=dev)
        self._c = _lib.WrsnTransitionBuffers(C, A, *[t.data_ptr() for t in (
            self.pend_state, self.pend_action, self.pend_logp, self.pend_valid, self.state, self.action, self.next_state,
            self.reward, self.logp, self.now, self.env_index, self.count)])

    def clear(self, keep_pending=False):
        self.count.zero_()
        if not keep_pending:
            self.pend_valid.zero_()

    def _record(self, call, agent_ids, actions, logp, *rows):
        """`call(self._c, agent_ids, actions, logp, *rows)` on the addresses of the arguments in the types the kernels read."""
        env, t = self.env, self.env.torch
        env._bind_stream()
        a = agent_ids.to(device=env.device, dtype=t.int32).contiguous()
        x = actions.to(device=env.device, dtype=t.float32).reshape(env.num_env, self.action_elems).contiguous()
        lp = logp.to(device=env.device, dtype=t.float32).reshape(env.num_env).contiguous()
        self._keep = (a, x, lp) + rows                        # alive until the kernel has run
        call(self._c, *[v.data_ptr() for v in self._keep])

    def _collect(self, call, *args):
        env = self.env
        env._bind_stream()
        call(self._c, *args, **env._out_ptrs())

    def counts(self):
        """Transitions appended per charger so far (host list; synchronises)."""
        return [int(v) for v in self.count.cpu()]

    def stored(self):
        return [min(c, self.capacity) for c in self.counts()]


class TransitionBuffers(_TransitionBuffers):
    """Per-charger transition lists of a batched roll-out, filled by the HIP kernels of csrc/wrsn_rollout.h.

    env          : VecWRSN (rendering on); `pend_state`, `state` and `next_state` take the dtype of its `state` (float32 or bfloat16:
                   the copy kernels move rows in the environment's observation format)
    capacity     : transitions kept per charger (further ones are counted in `count` and dropped)
    action_elems : size of the policy's raw output per decision: 3, or map_size**2 for density-map policies"""

    def __init__(self, env, capacity, action_elems):
        if env.state is None:
            raise ValueError("TransitionBuffers needs a rendering VecWRSN (render=True)")
        super().__init__(env, capacity, action_elems, (4, env.map_size, env.map_size), env.state.dtype)

    def record(self, agent_ids, actions, logp, states=None):
        """The chargers `agent_ids` [B] (< 0: none) are about to receive `actions` [B, action_elems] (IPPO.py:141-142)."""
        env = self.env
        st = (env.state if states is None else states.to(device=env.device, dtype=env.state.dtype)).contiguous()
        self._record(env._h.rollout_record, agent_ids, actions, logp, st)

    def collect(self):
        """Append the transitions the request just returned by `env.step` completes (IPPO.py:144-155)."""
        self._collect(self.env._h.rollout_collect)


def select_batch(rewards, batch_size, rng=np.random):
    """The reference's batch selection (IPPO.py:193-200), index for index: the `batch_size // 2` rewards furthest from
    the mean, plus `batch_size - batch_size // 2` indices drawn without replacement from range(len - batch_size // 2)."""
    rewards = np.asarray(rewards)
    mean = np.mean(rewards)
    abs_diff = np.abs(rewards - mean)
    indices = np.argsort(abs_diff)
    selected_num = int(batch_size / 2.0)
    random_num = batch_size - selected_num
    return np.concatenate((indices[-selected_num:], rng.choice(len(rewards) - selected_num, size=random_num, replace=False)))


# ------------------------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------------------------
DEFAULT_ARGS = dict(seed=0, lr=3.0e-4, gamma=0.99, clip=0.2, batch_size=512, n_updates_per_iteration=5, save_freq=5, gae=True,
                    norm_adv=True, minibatch_size=64, ent_coef=0.0, vf_coef=0.5, gae_lambda=0.95, max_grad_norm=0.5,
                    clip_vloss=True)                          # alg_args/ippo.yaml:4-18


class PPOLearner:
    """Networks, optimisers and the PPO arithmetic of the reference's IPPO (IPPO.py:17-117, 225-271) for `num_agent`
    chargers; knows nothing about environments.

    process_group : data-parallel training -- the flattened actor + critic gradients of the charger being updated are averaged
                  over the ranks with ONE all-reduce per minibatch (RCCL over xGMI with backend "nccl"; gloo in the CPU tests).
                  Parameters and BatchNorm buffers are broadcast from rank 0 at construction."""

    def __init__(self, args, num_agent, map_size, device, model_path=None, infer_chunk=1024, process_group=None, inference_dtype=None, min_bucket=16):
        torch = _torch()
        self.torch = torch
        self.num_agent = int(num_agent)
        self.map_size = int(map_size)
        self.device = torch.device(device)
        a = dict(DEFAULT_ARGS); a.update(args or {})
        self.args = a
        for k in ("gamma", "clip", "batch_size", "minibatch_size", "n_updates_per_iteration", "save_freq", "gae", "clip_vloss", "ent_coef",
                  "vf_coef", "gae_lambda", "norm_adv", "max_grad_norm"):
            setattr(self, k, a[k])
        self.actors, self.critics = self._build_networks()
        # optional reduced-precision INFERENCE (roll-out actions and values only; the update stays float32): "bf16" doubles the
        # forward throughput again but the roll-out log-probabilities then differ from the float32 ones the update recomputes
        self.inference_dtype = {None: None, "bf16": torch.bfloat16, "fp16": torch.float16}[inference_dtype]
        self.loggers = [{"i_so_far": 0, "t_so_far": 0, "ep_lifetime": [], "losses": [], "rewards": []} for _ in range(self.num_agent)]
        if model_path is not None:                            # IPPO.py:49-64
            for agent_folder in os.listdir(model_path):
                i = int(agent_folder); p = os.path.join(model_path, agent_folder)
                self.critics[i].load_state_dict(torch.load(os.path.join(p, "critic.pth"), map_location=self.device, weights_only=True))
                self.actors[i].load_state_dict(torch.load(os.path.join(p, "actor.pth"), map_location=self.device, weights_only=True))
        self.group = process_group
        dist = torch.distributed
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        if self.world > 1:
            for net in self.actors + self.critics:
                for p in list(net.parameters()) + list(net.buffers()):
                    dist.broadcast(p.data, src=0, group=process_group)
        self.optimizers = [torch.optim.Adam(list(self.actors[i].parameters()) + list(self.critics[i].parameters()), lr=a["lr"])
                           for i in range(self.num_agent)]
        self.infer_chunk = int(infer_chunk)
        self.min_bucket = max(1, int(min_bucket))

    # -- what a subclass with other networks replaces: construction, `_forward`, and the axes a decision's action spans
    _logp_dims = (1, 2)                                        # log-prob / entropy are summed over these axes of the action (G x G map)

    def _build_networks(self):
        """(actors, critics): one network of each kind per charger, on `self.device`."""
        torch = self.torch
        UNet, CNNCritic = build_networks(self.map_size)
        # channels-last weights and activations: the same float32 arithmetic, 3.6 x the NCHW convolution throughput of MIOpen on
        # MI355X (tools/diag_policy.py: 71 vs 20 TFLOP/s for the UNet forward); state_dict keys and shapes are unaffected
        self._cl = self.device.type == "cuda"
        mf = dict(memory_format=torch.channels_last) if self._cl else {}
        actors = [UNet().to(self.device).to(**mf) for _ in range(self.num_agent)]
        critics = [CNNCritic().to(self.device).to(**mf) for _ in range(self.num_agent)]
        return actors, critics

    # -- policy ------------------------------------------------------------------------------------------------------
    def _bucket(self, r):
        """Rows a short inference chunk is padded to: `min_bucket` (16) doubled until it fits, at most `infer_chunk`.  MIOpen searches /
        compiles its convolution kernels per input shape (seconds for each new one), so the forward passes of a roll-out may only
        ever see this small set of batch shapes; padding to the power of two instead of the full chunk keeps a 20-row request
        from paying for (and taking its BatchNorm statistics from) hundreds of copies of itself."""
        b = self.min_bucket
        while b < r:
            b <<= 1
        return min(b, self.infer_chunk)

    _pad_on_cpu = False                                        # short chunks are padded to their bucket on the device only

    def _actor_chunks(self, agent_id, states):
        """The actor over `states` in the batch composition of the roll-out: chunks of `infer_chunk` rows, a short chunk filled up to its
        bucket by repeating its own rows, whose outputs are dropped.  Yields (mean, log_std) in float32 per chunk."""
        torch = self.torch
        for s in states.split(self.infer_chunk):
            r = s.shape[0]
            nb = self._bucket(r) if self._pad_on_cpu or self.device.type == "cuda" else r
            if r < nb:
                s = s.index_select(0, torch.arange(nb, device=s.device) % r)
            mean, log_std = self._forward(self.actors[agent_id], s, inference=True)
            yield mean[:r].float(), log_std[:r].float()

    def get_action(self, agent_id, states):
        """IPPO.py:95-105 for a batch: states [n,4,G,G] -> (action maps [n,G,G], summed log-prob [n]).

        The actor runs in training mode like the reference's (IPPO.py never calls `.eval()`), so BatchNorm normalises with the
        statistics of the rows in THIS forward pass: the sampled means and the stored log-probabilities depend on the batch
        composition (rows of the chunk + its padding), exactly as the reference's depend on its batch of one."""
        torch = self.torch
        outs, lps = [], []
        with torch.no_grad():
            for mean, log_std in self._actor_chunks(agent_id, states):
                dist = torch.distributions.Normal(mean, log_std.exp())
                act = dist.sample()
                outs.append(act); lps.append(dist.log_prob(act).sum(self._logp_dims))
        return torch.cat(outs), torch.cat(lps)

    def rollout_logp(self, agent_id, states, actions):
        """Log-probabilities of `actions` [n,G,G] under the current actor, evaluated over `states` in the SAME batch composition
        `get_action` uses (same chunks, same padding, same precision): with unchanged weights this reproduces the log-probabilities
        `get_action` returned for those rows.  `evaluate` over a different composition (a 64-row minibatch of the update) does not:
        BatchNorm in training mode makes the actor's output a function of the whole batch -- the reference has the same property
        (roll-out on batches of one, IPPO.py:95-105; update on minibatches, IPPO.py:236-241)."""
        torch = self.torch
        lps = []
        with torch.no_grad():
            for (mean, log_std), a in zip(self._actor_chunks(agent_id, states), actions.split(self.infer_chunk)):
                lps.append(torch.distributions.Normal(mean, log_std.exp()).log_prob(a.float()).sum(self._logp_dims))
        return torch.cat(lps)

    def _forward(self, net, x, inference=False):
        """One forward pass over a chunk / minibatch of states.  bfloat16 states (VecWRSN(obs_dtype="bfloat16")) go in as they are under
        autocast; otherwise this chunk alone is widened to float32 (exact), never a whole buffer."""
        torch = self.torch
        if x.dtype == torch.bfloat16 and not (inference and self.inference_dtype is not None):
            x = x.float()
        if self._cl:
            x = x.contiguous(memory_format=torch.channels_last)
        if inference and self.inference_dtype is not None:
            with torch.autocast(self.device.type, dtype=self.inference_dtype):
                return net(x)
        return net(x)

    def evaluate(self, agent_id, batch_states, batch_actions):  # IPPO.py:107-113
        torch = self.torch
        mean, log_std = self._forward(self.actors[agent_id], batch_states)
        dist = torch.distributions.Normal(mean, log_std.exp())
        return dist.log_prob(batch_actions).sum(self._logp_dims), dist.entropy().sum(self._logp_dims)

    def get_value(self, agent_id, state):                     # IPPO.py:115-117
        return self._forward(self.critics[agent_id], state).sum(1)

    def _values(self, agent_id, states):
        torch = self.torch
        with torch.no_grad():
            return torch.cat([self._forward(self.critics[agent_id], s, inference=True).float().sum(1) for s in states.split(self.infer_chunk)])

    def cal_rt_adv(self, id, states, rewards, next_states, terminals):
        """IPPO.py:71-93.  `terminals` follows the reference's convention (the stored flags multiply the bootstrap term);
        every stored transition has terminal == False, so the recursion collapses to returns == rewards."""
        torch = self.torch
        with torch.no_grad():
            values = self._values(id, states)
            next_values = self._values(id, next_states)
            tm = terminals.to(rewards.dtype)
            if self.gae:
                advantages = torch.zeros_like(rewards)
                last = torch.zeros((), dtype=rewards.dtype, device=rewards.device)
                for t in reversed(range(len(rewards))):
                    delta = rewards[t] + self.gamma * next_values[t] * tm[t] - values[t]
                    last = delta + self.gamma * self.gae_lambda * tm[t] * last
                    advantages[t] = last
                returns = advantages + values
            else:
                # the reference's plain branch reads returns[t + 1] at t = len - 1 and raises IndexError on every non-empty
                # input (IPPO.py:86-90; alg_args/ippo.yaml ships gae: True): same behaviour here
                if len(rewards) > 0:
                    raise IndexError("index %d is out of bounds for dimension 0 with size %d" % (len(rewards), len(rewards)))
                returns = torch.zeros_like(rewards); advantages = returns - values
        return returns, advantages, values

    # -- update ------------------------------------------------------------------------------------------------------
    def _allreduce_grads(self, id):
        """Data-parallel step: average the gradients of actor + critic of charger `id` over the ranks with
        one all-reduce of the flattened bucket."""
        if self.world <= 1:
            return
        torch = self.torch
        params = [p for p in list(self.actors[id].parameters()) + list(self.critics[id].parameters()) if p.grad is not None]
        flat = torch.cat([p.grad.reshape(-1) for p in params])
        torch.distributed.all_reduce(flat, group=self.group)
        flat /= self.world
        o = 0
        for p in params:
            n = p.numel(); p.grad.copy_(flat[o:o + n].view_as(p)); o += n

    def sync_buffers(self, id):
        """Data-parallel: BatchNorm running statistics are local to a rank (every rank normalises its own minibatches); average
        them over the ranks so that what is written to a checkpoint does not depend on which rank writes it."""
        if self.world <= 1:
            return
        torch = self.torch
        bufs = [b for b in list(self.actors[id].buffers()) + list(self.critics[id].buffers()) if b.dtype.is_floating_point]
        if not bufs:
            return
        flat = torch.cat([b.reshape(-1) for b in bufs])
        torch.distributed.all_reduce(flat, group=self.group)
        flat /= self.world
        o = 0
        for b in bufs:
            n = b.numel(); b.copy_(flat[o:o + n].view_as(b)); o += n

    def save_checkpoint(self, id, folder):
        """IPPO.py:296-309: `<folder>/{actor,critic}.pth`.  Under data-parallel training every rank calls this (the buffer average is
        a collective); rank 0 alone writes."""
        torch = self.torch
        self.sync_buffers(id)
        rank = torch.distributed.get_rank(self.group) if self.world > 1 else 0
        if rank == 0:
            os.makedirs(folder, exist_ok=True)
            torch.save(self.actors[id].state_dict(), os.path.join(folder, "actor.pth"))
            torch.save(self.critics[id].state_dict(), os.path.join(folder, "critic.pth"))

    def minibatch_loss(self, id, batch, mb):
        """The loss of IPPO.py:236-262 on the rows `mb` of `batch` for charger `id`: (loss, pg_loss, v_loss, entropy, approx_kl,
        clipfrac).  Forward passes run in training mode (BatchNorm statistics of this minibatch), like the reference's."""
        torch = self.torch
        newlogprob, entropy = self.evaluate(id, batch["states"][mb], batch["actions"][mb])
        newvalue = self.get_value(id, batch["states"][mb]).view(-1)
        logratio = newlogprob - batch["log_probs"][mb]
        ratio = logratio.exp()
        with torch.no_grad():
            approx_kl = ((ratio - 1) - logratio).mean()
            clipfrac = ((ratio - 1.0).abs() > self.clip).to(ratio.dtype).mean().item()
        adv = batch["advantages"][mb]
        if self.norm_adv:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - self.clip, 1 + self.clip)).mean()
        if self.clip_vloss:
            v_un = (newvalue - batch["returns"][mb]) ** 2
            v_cl = batch["values"][mb] + torch.clamp(newvalue - batch["values"][mb], -self.clip, self.clip)
            v_loss = 0.5 * torch.max(v_un, (v_cl - batch["returns"][mb]) ** 2).mean()
        else:
            v_loss = 0.5 * ((newvalue - batch["returns"][mb]) ** 2).mean()
        entropy_loss = entropy.mean()
        loss = pg_loss - self.ent_coef * entropy_loss + v_loss * self.vf_coef
        return loss, pg_loss, v_loss, entropy_loss, approx_kl, clipfrac

    def apply_gradients(self, id):
        """IPPO.py:264-268 after `loss.backward()`: (data-parallel: average the gradients over the ranks,) clip the actor's and the
        critic's gradient norms separately, Adam step."""
        nn = self.torch.nn
        self._allreduce_grads(id)
        nn.utils.clip_grad_norm_(self.actors[id].parameters(), self.max_grad_norm)
        nn.utils.clip_grad_norm_(self.critics[id].parameters(), self.max_grad_norm)
        self.optimizers[id].step()

    def update(self, id, batch, shuffle=np.random.shuffle):
        """IPPO.py:229-271 for charger `id`; returns the last minibatch's (pg_loss, v_loss, entropy, approx_kl, clipfrac).
        `approx_kl` / `clipfrac` of the FIRST minibatch after a roll-out are not small, here as in the reference: the stored
        log-probabilities were computed with the BatchNorm statistics of the roll-out batch (`get_action`; the reference: a batch of
        one), the update recomputes them over a minibatch -- see `rollout_logp`."""
        torch = self.torch
        b_inds = np.arange(self.batch_size)
        clipfracs = []
        stats = None
        for _ in range(self.n_updates_per_iteration):
            shuffle(b_inds)
            for start in range(0, self.batch_size, self.minibatch_size):
                mb = torch.as_tensor(b_inds[start:start + self.minibatch_size], device=batch["states"].device, dtype=torch.long)
                loss, pg_loss, v_loss, entropy_loss, approx_kl, clipfrac = self.minibatch_loss(id, batch, mb)
                clipfracs.append(clipfrac)
                self.optimizers[id].zero_grad()
                loss.backward()
                self.apply_gradients(id)
                self.loggers[id]["losses"].append(float(loss.detach()))
                stats = (float(pg_loss.detach()), float(v_loss.detach()), float(entropy_loss.detach()), float(approx_kl), float(np.mean(clipfracs)))
        return stats


class RolloutDriver:
    """The batched roll-out and the training loop on top of a learner (`PPOLearner` or a subclass, which follows this class in the bases of a
    trainer): timers, `step_batch`, `roll_out`, `train`.  A trainer says how its policy chooses (`_choose`), what it hands to `env.step` if
    that is not what it stores (`_action3`), whether a launch checks the status rows (`_check_status`) and the shape `evaluate` takes
    the stored actions in (`_stored_actions`)."""

    _check_status = False                                      # raise when a row comes back from the step with status < 0
    _ledger = None                                             # an EpisodeLog the roll-out books its requests into (log_episodes), or None

    def _attach(self, env, buffers, log):
        self.env, self.buffers, self.log = env, buffers, log
        self.timers = {"env_s": 0.0, "policy_s": 0.0, "glue_s": 0.0, "prepare_s": 0.0, "train_s": 0.0, "launches": 0, "requests": 0}
        self._req = None

    # -- roll-out ----------------------------------------------------------------------------------------------------
    def _sync_time(self):
        self.torch.cuda.synchronize(self.device) if self.device.type == "cuda" else None
        return time.perf_counter()

    def _choose_per_charger(self, ids, width, gather):
        """One `get_action` per charger over the rows that ask for it, `gather(rows)` being its input for those rows: (actions
        [B, width], log-probabilities [B]), zeros where nobody asks."""
        torch, env = self.torch, self.env
        out = torch.zeros((env.num_env, width), dtype=torch.float32, device=env.device)
        logp = torch.zeros((env.num_env,), dtype=torch.float32, device=env.device)
        for a in range(self.num_agent):
            rows = torch.nonzero(ids == a).flatten()
            if rows.numel() == 0:
                continue
            act, lp = self.get_action(a, gather(rows))
            out.index_copy_(0, rows, act.reshape(rows.numel(), width).float()); logp.index_copy_(0, rows, lp.float())
        return out, logp

    def _choose(self, r, ids):
        """(what the buffers store [B, action_elems], log-probabilities [B], the float64 [B, 3] `env.step` takes or None: `_action3`
        widened) for the request `r`, whose charger ids are `ids`."""
        raise NotImplementedError

    def _action3(self, ids, stored):
        """The 3-vector of a launch, from what the policy chose and the buffers store."""
        return stored

    def _stored_actions(self, actions):
        """Stored action rows [n, action_elems] in the shape `evaluate` takes."""
        return actions

    def step_batch(self):
        """One launch of the batched roll-out: act for every environment that carries a request, step, collect."""
        torch, env = self.torch, self.env
        r = self._req
        ids = r["agent_id"].clone()                           # the request's ids, detached from the tensor the step writes
        t0 = self._sync_time()
        stored, logp, handed = self._choose(r, ids)
        t1 = self._sync_time()
        self.buffers.record(ids, stored, logp)
        act3 = self._action3(ids, stored)
        t2 = self._sync_time()
        r = env.step(ids, act3.double() if handed is None else handed)
        t3 = self._sync_time()
        if self._check_status:
            bad = torch.nonzero(r["status"] < 0).flatten()
            if bad.numel():
                raise RuntimeError("environment rows %s report status %s" % (bad.tolist(), r["status"][bad].tolist()))
        if self._ledger is not None:                          # the ledger first and without consuming: the requests are the buffers' too
            env.episodes_collect(self._ledger, 0.0, consume=False)
        self.buffers.collect()
        t4 = self._sync_time()
        tm = self.timers
        tm["policy_s"] += t1 - t0; tm["glue_s"] += (t2 - t1) + (t4 - t3); tm["env_s"] += t3 - t2; tm["launches"] += 1
        tm["requests"] += int((ids >= 0).sum())
        self.last_ids, self.last_action3 = ids, act3          # what this launch handed to the environments (tests / logging)
        self._req = r
        return r

    def roll_out(self, max_launches=100000, fresh_episodes=False):
        """IPPO.py:119-210 over the batch: launches until every charger has `batch_size` transitions, then the reference's
        per-charger batch selection.  Environments restart by auto-reset, so one roll-out spans many episodes.

        The environments live ACROSS roll-outs: the first call resets them, every later call goes on from the requests the
        previous one ended with (pending actions included -- their stored log-probabilities come from the policy that chose
        them, i.e. the one before the last update).  With a large batch the per-charger quota is reached within a few launches;
        restarting every roll-out from `reset()` would then only ever store the first decision after the warm-up snapshot (all
        chargers at the base station, no node death, no terminal return), which is not what the reference's roll_out collects: it
        runs every episode to its terminal (IPPO.py:130-190).  `fresh_episodes=True` restores the restart-per-roll-out behaviour."""
        torch, env = self.torch, self.env
        if not env.auto_reset:
            raise ValueError("%s needs VecWRSN(auto_reset=True)" % type(self).__name__)
        if fresh_episodes or self._req is None:
            self.buffers.clear()
            self._req = env.reset()
            if self._ledger is not None:                      # every row starts an episode: what ran before is not booked
                env.episodes_collect(self._ledger, 0.0, consume=False)
        else:
            self.buffers.clear(keep_pending=True)
        for _ in range(max_launches):
            self.step_batch()
            if min(self.buffers.counts()) >= self.batch_size:
                break
        t0 = self._sync_time()                                 # `prepare_s`: everything from here on -- selection, gathers, values, GAE
        short = [a for a, n in enumerate(self.buffers.stored()) if n < self.batch_size]
        if short:
            raise RuntimeError("roll_out stopped after %d launches with %s transitions per charger, fewer than batch_size %d (buffer capacity %d): "
                               "raise max_launches / capacity or lower batch_size" % (max_launches, self.buffers.stored(), self.batch_size, self.buffers.capacity))
        out = self._prepare_batches()
        self.timers["prepare_s"] += self._sync_time() - t0
        return out

    def _episode_stats(self):
        """The reference's `_log_summary` fields (IPPO.py:316-317) over the episodes the ledger closed since it was last emptied:
        `avg_ep_lifetime` (mean env.now of the closing returns), `avg_ep_lens` (mean requests per charger and episode; the reference's
        `cnt` leaves out each charger's first) and `episodes` (how many closed; NaN averages when none did).  One host read; the log is
        emptied, the sums of the episodes in progress stay."""
        log = self._ledger
        fin = log.finished.cpu().numpy()
        stored = np.arange(log.episodes)[:, None] < np.minimum(fin, log.episodes)[None, :]      # [E, B]: slots that hold an episode
        life, dec, closed = log.lifetime.cpu().numpy()[stored], log.decisions.cpu().numpy()[stored], int(fin.sum())
        dropped = int(log.dropped.sum())
        if dropped:                                           # the averages cover the stored episodes only: say so instead of hiding it
            warnings.warn("%d of %d episodes closed since the last read did not fit the %d slots per environment: avg_ep_lifetime and "
                          "avg_ep_lens leave them out (raise episode_slots)" % (dropped, closed, log.episodes))
        log.clear(keep_running=True)                          # after the reads: on a CPU device `fin` is a view of the log
        nan = float("nan")
        return dict(avg_ep_lifetime=float(life.mean()) if life.size else nan, avg_ep_lens=float(dec.mean()) if dec.size else nan,
                    episodes=closed)

    def _prepare_batches(self):
        """The tail of `roll_out`: per charger the reference's batch selection, the gathers and `cal_rt_adv`; the list of batch dicts."""
        torch, env = self.torch, self.env
        out = []
        for a in range(self.num_agent):
            n = self.buffers.stored()[a]
            rewards = self.buffers.reward[a, :n]
            idx_np = select_batch(rewards.cpu().numpy(), self.batch_size)
            idx = torch.as_tensor(idx_np, device=env.device, dtype=torch.long)
            states = self.buffers.state[a].index_select(0, idx); nxt = self.buffers.next_state[a].index_select(0, idx)
            rew = rewards.index_select(0, idx)
            # the reference runs cal_rt_adv per episode over the transitions of that episode (IPPO.py:171); with terminals all
            # False neither returns nor advantages couple two transitions, so one call over the selected batch gives the same values
            returns, adv, values = self.cal_rt_adv(a, states, rew, nxt, torch.zeros_like(rew))
            out.append(dict(states=states, actions=self._stored_actions(self.buffers.action[a].index_select(0, idx)),
                            log_probs=self.buffers.logp[a].index_select(0, idx), rewards=rew, next_states=nxt, advantages=adv, returns=returns,
                            values=values))
            self.loggers[a]["rewards"].append(float(rew.mean()))
        return out

    def train(self, trained_iterations, save_folder=None):
        """IPPO.py:212-311: roll out, update every charger, log, checkpoint every `save_freq` iterations.  With `log_episodes` the
        episode fields of an iteration cover everything the ledger closed since it was last read: a `roll_out()` called directly in
        front of `train()` is counted into the first iteration's rows."""
        torch = self.torch
        start = time.time(); i_so_far = 0; rows = []
        while i_so_far <= trained_iterations:
            batches = self.roll_out()
            i_so_far += 1
            episodes = self._episode_stats() if self._ledger is not None else {}
            t0 = self._sync_time()
            joint = self.update_all(batches) if getattr(self, "joint_update", False) else None   # every charger's update at once
            for id in range(self.num_agent):
                lg = self.loggers[id]
                lg["t_so_far"] += self.batch_size; lg["i_so_far"] += 1
                st = joint[id] if joint is not None else self.update(id, batches[id])
                y_pred, y_true = batches[id]["values"].cpu().numpy(), batches[id]["returns"].cpu().numpy()
                var_y = np.var(y_true)
                ev = float("nan") if var_y == 0 else 1 - np.var(y_true - y_pred) / var_y
                row = dict(iteration=lg["i_so_far"], timesteps=lg["t_so_far"], agent=id, policy_loss=st[0], value_loss=st[1], entropy=st[2],
                           approx_kl=st[3], clipfrac=st[4], explained_variance=float(ev), mean_reward=lg["rewards"][-1],
                           sps=i_so_far / (time.time() - start))
                row.update(episodes)
                rows.append(row)
                if self.log:
                    self.log(row)
                if save_folder is not None and lg["i_so_far"] % self.save_freq == 0:      # IPPO.py:296-309 layout: <iter>/<agent>/{actor,critic}.pth
                    self.save_checkpoint(id, os.path.join(save_folder, str(lg["i_so_far"]), str(id)))
            self.timers["train_s"] += self._sync_time() - t0
        return rows


class BatchedIPPO(RolloutDriver, PPOLearner):
    """`IPPO(args, env, device, model_path=None)` of the reference (IPPO.py:17-69) over a `VecWRSN` with density-map actions
    (`density_map=True` environments of runner/IPPO.py:19-21): the actor's G x G output is the action and is turned into the
    3-vector on the device (`VecWRSN.density_to_action`)."""

    def __init__(self, args, env, device=None, model_path=None, capacity=None, infer_chunk=1024, process_group=None, log=None, inference_dtype=None,
                 min_bucket=16):
        super().__init__(args, env.num_agent, env.map_size, device if device is not None else env.device, model_path, infer_chunk, process_group,
                         inference_dtype, min_bucket)
        self._attach(env, TransitionBuffers(env, capacity or 2 * self.batch_size, env.map_size * env.map_size), log)

    def _choose(self, r, ids):
        G = self.env.map_size
        return self._choose_per_charger(ids, G * G, lambda rows: r["state"].index_select(0, rows)) + (None,)

    def _action3(self, ids, maps):                            # float64: `step_batch` hands it to `env.step` as it is
        G = self.env.map_size
        return self.env.density_to_action(ids, maps.view(self.env.num_env, G, G).double())

    def _stored_actions(self, actions):
        return actions.view(-1, self.env.map_size, self.env.map_size)


# ------------------------------------------------------------------------------------------------------------------
# training from the entity observation: packed rows, a permutation-invariant actor / critic, the trainer on top
# ------------------------------------------------------------------------------------------------------------------
def entity_row_elems(n_node, num_agent):
    """Floats of one packed entity row: node [N][8], then mc [M][12], then env [8] (include/wrsn_hip.h, wrsn_transition_buffers)."""
    return _lib.ENT_NODE_F * int(n_node) + _lib.ENT_MC_F * int(num_agent) + _lib.ENT_ENV_F


class EntityTransitionBuffers(_TransitionBuffers):
    """`TransitionBuffers` for the entity observation (`wrsn_rollout_record_entities` / `wrsn_rollout_collect_entities`): a stored
    state is one packed float32 row of R = 8 N + 12 M + 8 elements, `pend_state` [B, M, R], `state` / `next_state` [M, capacity, R].

    env          : VecWRSN(entities=True); needs no image (`render=False`) -- the rows are read from the buffers it registered
    capacity     : transitions kept per charger (further ones are counted in `count` and dropped)
    action_elems : size of the policy's raw output per decision (3: the action vector itself)"""

    def __init__(self, env, capacity, action_elems=3):
        if not getattr(env, "entities", False):
            raise ValueError("EntityTransitionBuffers needs a VecWRSN with the entity observation (entities=True)")
        self.row_elems = entity_row_elems(env.n_node, env.num_agent)
        super().__init__(env, capacity, action_elems, (self.row_elems,), env.torch.float32)

    @staticmethod
    def split(rows, num_agent):
        """Views (nodes [n,N,8], chargers [n,M,12], env_feat [n,8]) of packed rows [n,R] for M = num_agent chargers."""
        M = int(num_agent)
        nf, mf, ef = _lib.ENT_NODE_F, _lib.ENT_MC_F, _lib.ENT_ENV_F
        n, R = rows.shape[0], rows.shape[-1]
        N = (R - mf * M - ef) // nf
        if N < 0 or entity_row_elems(N, M) != R:
            raise ValueError("rows of %d floats are no packed entity rows of %d chargers" % (R, M))
        return (rows[..., :nf * N].reshape(n, N, nf), rows[..., nf * N:nf * N + mf * M].reshape(n, M, mf), rows[..., nf * N + mf * M:])

    @staticmethod
    def pack(nodes, chargers, env_feat):
        """Packed rows [n,R] of entity tensors (nodes [n,N,8], chargers [n,M,12], env_feat [n,8]): what the device kernels store."""
        torch = _torch()
        return torch.cat([nodes.flatten(1), chargers.flatten(1), env_feat.flatten(1)], 1)

    def record(self, agent_ids, actions, logp):
        """The chargers `agent_ids` [B] (< 0: none) are about to receive `actions` [B, action_elems], chosen on the entity rows the
        environment holds now (IPPO.py:141-142)."""
        self._record(self.env._h.rollout_record_entities, agent_ids, actions, logp)

    def collect(self, consume=True):
        """Append the transitions the request just returned by `env.step` completes (IPPO.py:144-155).  consume=False leaves the
        requests to the `TransitionBuffers.collect` of the same launch that follows."""
        self._collect(self.env._h.rollout_collect_entities, None, consume)


def _entity_parts(n_agent_rows):
    """(torch, lin, _Trunk): what the entity networks of `n_agent_rows` chargers share -- the row-wise Linear and the trunk class."""
    torch = _torch()
    nn = torch.nn
    F = torch.nn.functional
    M = int(n_agent_rows)
    n_alive, c_alive, c_self = _lib.ENT_NODE["alive"], _lib.ENT_MC["alive"], _lib.ENT_MC["is_self"]
    e_agent, e_nnode = _lib.ENT_ENV["agent"], _lib.ENT_ENV["n_node"]

    def lin(layer, x):
        """`layer` on x [n, r, K] as n separate [r, K] x [K, O] products (a batched matrix product over the rows of the batch): one
        flattened [n r, K] GEMM is tiled over all rows, and which tile -- hence which summation order -- a row falls into depends on the
        batch around it; here the arithmetic done for a row is the same whatever the batch holds."""
        return torch.bmm(x, layer.weight.t().unsqueeze(0).expand(x.shape[0], -1, -1)) + layer.bias

    class _Trunk(nn.Module):
        def __init__(self):
            super().__init__()
            self.node1 = _ortho(nn.Linear(_lib.ENT_NODE_F, 64)); self.node2 = _ortho(nn.Linear(64, 64))
            self.mc1 = _ortho(nn.Linear(_lib.ENT_MC_F, 32)); self.mc2 = _ortho(nn.Linear(32, 32))
            self.head1 = _ortho(nn.Linear(64 + 64 + 32 + 32 + _lib.ENT_ENV_F, 128)); self.head2 = _ortho(nn.Linear(128, 128))

        def forward(self, rows):
            return self.embed(rows)[0]

        def embed(self, rows):
            """(z [n, 1, 128], the node embeddings h [n, N, 64], alive [n, N], and the views nodes, mcs, env of `rows`)."""
            nodes, mcs, env = EntityTransitionBuffers.split(rows, M)
            alive = nodes[..., n_alive] == 1                                             # [n, N]
            x = torch.where(alive.unsqueeze(-1), nodes, torch.zeros_like(nodes))       # a select, not a product: NaN / inf in a dead row vanish too
            h = F.relu(lin(self.node2, F.relu(lin(self.node1, x))))
            z = self._head(h, alive, nodes, mcs, env)
            return z, h, alive, nodes, mcs, env

        def _head(self, h, alive, nodes, mcs, env):
            w = alive.unsqueeze(-1).to(h.dtype)
            cnt = w.sum(1)                                                               # [n, 1] live nodes of the row
            mean = (h * w).sum(1) / cnt.clamp(min=1.0)
            mx = h.masked_fill(~alive.unsqueeze(-1), float("-inf")).max(1).values
            mx = torch.where(cnt > 0, mx, torch.zeros_like(mx))                           # no live node: zeros
            g = F.relu(lin(self.mc2, F.relu(lin(self.mc1, mcs))))
            cw = (mcs[..., c_alive] == 1).unsqueeze(-1).to(g.dtype)
            cmean = (g * cw).sum(1) / cw.sum(1).clamp(min=1.0)
            own = (g * (mcs[..., c_self] == 1).unsqueeze(-1).to(g.dtype)).sum(1)          # the asking charger's embedding
            scale = torch.ones(_lib.ENT_ENV_F, dtype=env.dtype, device=env.device)       # charger index and node count as fractions
            scale[e_agent] = 1.0 / M; scale[e_nnode] = 1.0 / max(1, nodes.shape[1])
            x = torch.cat([mean, mx, cmean, own, env * scale], 1).unsqueeze(1)
            return F.relu(lin(self.head2, F.relu(lin(self.head1, x))))               # [n, 1, 128]: the heads go on row by row

    return torch, lin, _Trunk


def build_entity_networks(n_agent_rows):
    """Returns (EntityActor, EntityCritic) classes over packed entity rows [n, R] of `n_agent_rows` chargers (the node count follows
    from R).  A set policy: a per-node MLP pooled by masked mean and masked max over the live nodes, a per-charger MLP pooled by
    masked mean plus the asking charger's own embedding, and a head over the pools and the environment row.  No BatchNorm and no other
    operation across rows: a row's output does not depend on the batch it is evaluated in, so the log-probabilities of the roll-out and of
    the update agree.  Dead and padded node rows have no influence whatever they hold: their inputs are replaced by zeros and their
    embeddings masked out of both pools; a row without a live node pools to zeros."""
    torch, lin, _Trunk = _entity_parts(n_agent_rows)
    nn = torch.nn

    class EntityActor(nn.Module):
        """Packed rows [n, R] -> (mean [n, 3], log_std [n, 3]) of a diagonal Gaussian over the action vector; log_std in [-4, 1]."""

        def __init__(self):
            super().__init__()
            self.trunk = _Trunk()
            self.mean = _ortho(nn.Linear(128, 3), std=0.01)
            self.log_std = _ortho(nn.Linear(128, 3), std=0.01)

        def forward(self, rows):
            z = self.trunk(rows)
            return lin(self.mean, z).squeeze(1), lin(self.log_std, z).squeeze(1).clamp(-4.0, 1.0)

    class EntityCritic(nn.Module):
        """Packed rows [n, R] -> value [n, 1]."""

        def __init__(self):
            super().__init__()
            self.trunk = _Trunk()
            self.value = _ortho(nn.Linear(128, 1), std=0.01)

        def forward(self, rows):
            return lin(self.value, self.trunk(rows)).squeeze(1)

    return EntityActor, EntityCritic


LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def build_entity_pointer_networks(n_agent_rows, mask_claimed=False):
    """Returns (EntityPointerActor, EntityCritic) classes over packed entity rows [n, R] of `n_agent_rows` chargers; the critic is the
    class `build_entity_networks` returns.  The actor names a node: on the set policy's trunk (z [n, 128] and the per-node embeddings
    h [n, N, 64]) a query q = query(z) scores every alive node, l_i = 0.125 <h_i, q>, the decision is one alive node k drawn from
    softmax(l) and a charge variable x ~ N(mu, exp(log_std)) with (mu, log_std) = charge([z, the chosen node's eight features]); the
    action is (u_k, v_k, min_charge + (1 - min_charge) sigmoid(x)).  A row with no alive node has k = -1, no node term in
    log-probability and entropy, zeros for the node's features and the asking charger's own position as destination.  Like the set
    policy, nothing couples the rows of a batch (`lin` / `bmm`), and dead or padded node rows have no influence whatever they hold.

    mask_claimed=True: the choice runs over the CANDIDATES of a row instead of its alive nodes (`EntityPointerActor.candidates`, the rule
    of `wrsn_set_entity_pointer_mask` in include/wrsn_hip.h): the alive nodes outside the charging disc around every other live
    charger's destination, and every alive node when that leaves none.  Logits, node_logp, log-sum-exp, arg-max, the categorical
    entropy and the node term of a stored decision see candidates only; the pools behind z still run over all alive nodes and the
    charge head reads the stored node's features as they stand.  The parameters are the same: a block packs and unpacks either way."""
    torch, lin, _Trunk = _entity_parts(n_agent_rows)
    nn = torch.nn
    M = int(n_agent_rows)
    c_self, c_alive, e_agent = _lib.ENT_MC["is_self"], _lib.ENT_MC["alive"], _lib.ENT_ENV["agent"]
    masked = bool(mask_claimed)
    _, EntityCritic = build_entity_networks(n_agent_rows)

    class EntityPointerActor(nn.Module):
        def __init__(self):
            super().__init__()
            self.trunk = _Trunk()
            self.query = _ortho(nn.Linear(128, 64), std=0.01)
            self.charge = _ortho(nn.Linear(128 + _lib.ENT_NODE_F, 2), std=0.01)

        mask_claimed = masked

        @staticmethod
        def candidates(alive, nodes, mcs, env):
            """cand [n, N] of the views of packed rows: alive and not claimed, or alive where a row holds no such node.  Formed in float32
            from float32 copies of the row slices whatever dtype the rows have, one elementwise operation at a time -- the bits the
            device forms (wrsn_eh_claims), so a float64 reference sees the mask the kernel sees.  A claimer is a charger row with
            alive == 1 and is_self != 1; a NaN compares false and claims nothing."""
            f = torch.float32
            u, v = nodes[..., 0].detach().to(f).unsqueeze(2), nodes[..., 1].detach().to(f).unsqueeze(2)          # [n, N, 1]
            cx, cy = mcs[..., 6].detach().to(f).unsqueeze(1), mcs[..., 7].detach().to(f).unsqueeze(1)            # [n, 1, M]: destinations
            hx, hy = env[:, 0].detach().to(f).view(-1, 1, 1), env[:, 1].detach().to(f).view(-1, 1, 1)            # the disc's half-axes
            dx, dy = (u - cx) / hx, (v - cy) / hy
            inside = (dx * dx + dy * dy) <= 1.0                                                                   # [n, N, M]
            claimer = (mcs[..., c_alive] == 1) & ~(mcs[..., c_self] == 1)                                         # [n, M]
            free = alive & ~(inside & claimer.unsqueeze(1)).any(2)
            return torch.where(free.any(1, keepdim=True), free, alive)

        def scores(self, rows):
            """(z [n, 1, 128], logits l [n, N] with -inf for nodes that are not alive, node_logp [n, N] likewise, alive [n, N], the views
            nodes, mcs, env of `rows`).  Every -inf is put in by a select on finite numbers: no NaN, forward or backward.  With
            `mask_claimed` "alive" is "candidate" in everything returned: z alone is pooled over all alive nodes."""
            z, h, alive, nodes, mcs, env = self.trunk.embed(rows)
            if self.mask_claimed:
                alive = self.candidates(alive, nodes, mcs, env)
            q = lin(self.query, z)                                                       # [n, 1, 64]
            raw = 0.125 * torch.bmm(h, q.transpose(1, 2)).squeeze(2)                     # [n, N], finite everywhere: h of a dead node comes from zeros
            ninf = torch.full_like(raw, float("-inf"))
            any_alive = alive.any(1, keepdim=True)
            m = torch.where(any_alive, torch.where(alive, raw, ninf).max(1, keepdim=True).values.detach(), torch.zeros_like(raw[:, :1]))
            ex = torch.where(alive, (torch.where(alive, raw, m) - m).exp(), torch.zeros_like(raw))
            s = ex.sum(1, keepdim=True)
            lse = m + torch.where(any_alive, s, torch.ones_like(s)).log()
            return z, torch.where(alive, raw, ninf), torch.where(alive, raw - lse, ninf), alive, nodes, mcs, env

        @staticmethod
        def choose(logits, alive, gumbel=None):
            """k [n] = the alive node with the largest l + g (g None: l alone, the mode), the lowest index among equal scores; -1 when no
            node is alive."""
            N = logits.shape[1]
            sc = logits if gumbel is None else logits + gumbel.to(logits.dtype)
            sc = torch.where(alive & (sc > float("-inf")), sc, torch.full_like(sc, float("-inf")))      # a NaN never beats a number
            best = sc.max(1, keepdim=True).values
            idx = torch.arange(N, device=logits.device).expand_as(sc)
            k = torch.where(alive & (sc == best), idx, torch.full_like(idx, N)).min(1).values
            return torch.where(k < N, k, torch.full_like(k, -1))

        def charge_head(self, z, nodes, k):
            """(mu [n], log_std [n] in [-4, 1], x_k [n, 8]) of the charge variable for the chosen nodes k [n] (-1: zeros for x_k)."""
            has = (k >= 0).unsqueeze(1)
            xk = nodes.gather(1, k.clamp(min=0).view(-1, 1, 1).expand(-1, 1, nodes.shape[2])).squeeze(1)
            xk = torch.where(has, xk, torch.zeros_like(xk))
            out = lin(self.charge, torch.cat([z, xk.unsqueeze(1)], 2)).squeeze(1)
            return out[:, 0], out[:, 1].clamp(-4.0, 1.0), xk

        @staticmethod
        def destination(nodes, mcs, env, k):
            """(u, v) [n, 2] of the decision: the chosen node's position; for k = -1 the asking charger's own -- the lowest-index charger
            row with is_self == 1, else the row the environment row names."""
            n = nodes.shape[0]
            is_self = mcs[..., c_self] == 1
            idx = torch.arange(M, device=nodes.device).expand(n, M)
            first = torch.where(is_self, idx, torch.full_like(idx, M)).min(1).values
            agent = torch.nan_to_num(env[:, e_agent]).long().clamp(0, M - 1)
            me = torch.where(first < M, first, agent)
            own = mcs.gather(1, me.view(-1, 1, 1).expand(-1, 1, mcs.shape[2])).squeeze(1)[:, :2]
            at = nodes.gather(1, k.clamp(min=0).view(-1, 1, 1).expand(-1, 1, nodes.shape[2])).squeeze(1)[:, :2]
            return torch.where((k >= 0).unsqueeze(1), at, own)

        def act(self, rows, gumbel=None, eps=None, min_charge=0.0):
            """Draw a decision per row: dict of node [n], x [n], logp [n], action [n, 3], node_logp [n, N], mean [n], log_std [n]."""
            z, l, nlp, alive, nodes, mcs, env = self.scores(rows)
            k = self.choose(l, alive, gumbel)
            mu, ls, _ = self.charge_head(z, nodes, k)
            ep = torch.zeros_like(mu) if eps is None else eps.to(mu.dtype)
            x = mu + ls.exp() * ep
            c = min_charge + (1.0 - min_charge) * torch.sigmoid(x)
            lp = self._node_term(nlp, k) + (-0.5 * ep * ep - ls - LOG_SQRT_2PI)
            return dict(node=k, x=x, logp=lp, action=torch.cat([self.destination(nodes, mcs, env, k), c.unsqueeze(1)], 1), node_logp=nlp,
                        mean=mu, log_std=ls)

        @staticmethod
        def _node_term(nlp, k):
            picked = torch.where(nlp > float("-inf"), nlp, torch.zeros_like(nlp)).gather(1, k.clamp(min=0).unsqueeze(1)).squeeze(1)
            return torch.where(k >= 0, picked, torch.zeros_like(picked))

        def forward(self, rows, node, x):
            """(log-probability [n], entropy [n]) of the decisions (node [n] integer, -1: none; x [n]) on `rows`."""
            z, l, nlp, alive, nodes, mcs, env = self.scores(rows)
            k = node.long()
            mu, ls, _ = self.charge_head(z, nodes, k)
            ep = (x.to(mu.dtype) - mu) / ls.exp()
            lp = self._node_term(nlp, k) + (-0.5 * ep * ep - ls - LOG_SQRT_2PI)
            safe = torch.where(alive, nlp, torch.zeros_like(nlp))
            ent = -(torch.where(alive, safe.exp(), torch.zeros_like(safe)) * safe).sum(1) + ls + 0.5 + LOG_SQRT_2PI
            return lp, ent

    return EntityPointerActor, EntityCritic


def _pointer_layers(actor):
    t = actor.trunk
    return (t.node1, t.node2, t.mc1, t.mc2, t.head1, t.head2, actor.query, actor.charge)


def pack_entity_pointer_actor(actor):
    """The `EntityPointerActor` as the float32 block `wrsn_entity_pointer_act` reads (layout: include/wrsn_hip.h): the trunk at the offsets
    of the set actor's block, then query and charge, every Linear transposed to [in, out] and followed by its bias, zeros up to a
    multiple of 4 floats (56 980).  A new tensor [P] on the actor's device; it does not follow later changes of the parameters."""
    torch = _torch()
    parts = []
    for layer in _pointer_layers(actor):
        parts += [layer.weight.detach().t().reshape(-1), layer.bias.detach().reshape(-1)]
    flat = torch.cat([p.to(torch.float32) for p in parts])
    return torch.cat([flat, flat.new_zeros((-flat.numel()) % 4)])


def unpack_entity_pointer_actor(block, actor):
    """`pack_entity_pointer_actor` backwards: `copy_` of the block's floats into the parameters of `actor` (unpack(pack(x)) is x bit for bit)."""
    torch = _torch()
    o = 0
    with torch.no_grad():
        for layer in _pointer_layers(actor):
            w, b = layer.weight, layer.bias
            w.copy_(block[o:o + w.numel()].view(w.shape[1], w.shape[0]).t()); o += w.numel()
            b.copy_(block[o:o + b.numel()]); o += b.numel()


def pack_entity_actor(actor):
    """The `EntityActor` as the float32 block `wrsn_entity_act` reads (layout: include/wrsn_hip.h): node1, node2, mc1, mc2, head1, head2,
    mean, log_std, every Linear transposed to [in, out] and followed by its bias, zeros up to a multiple of 4 floats.  A new tensor [P] on
    the actor's device; it does not follow later changes of the parameters."""
    torch = _torch()
    t = actor.trunk
    parts = []
    for layer in (t.node1, t.node2, t.mc1, t.mc2, t.head1, t.head2, actor.mean, actor.log_std):
        parts += [layer.weight.detach().t().reshape(-1), layer.bias.detach().reshape(-1)]
    flat = torch.cat([p.to(torch.float32) for p in parts])
    return torch.cat([flat, flat.new_zeros((-flat.numel()) % 4)])


def _entity_layers(net):
    t = net.trunk
    return (t.node1, t.node2, t.mc1, t.mc2, t.head1, t.head2) + ((net.value,) if hasattr(net, "value") else (net.mean, net.log_std))


def pack_entity_critic(critic):
    """The `EntityCritic` as the float32 block `wrsn_entity_eval` / `wrsn_entity_ppo_grad` read (layout: include/wrsn_hip.h): the trunk at
    the offsets of the actor block, then `value`, every Linear transposed to [in, out] and followed by its bias, zeros up to a multiple of
    4 floats.  A new tensor; it does not follow later changes of the parameters."""
    torch = _torch()
    parts = []
    for layer in _entity_layers(critic):
        parts += [layer.weight.detach().t().reshape(-1), layer.bias.detach().reshape(-1)]
    flat = torch.cat([p.to(torch.float32) for p in parts])
    return torch.cat([flat, flat.new_zeros((-flat.numel()) % 4)])


def _unpack_entity(block, net):
    torch = _torch()
    o = 0
    with torch.no_grad():
        for layer in _entity_layers(net):
            w, b = layer.weight, layer.bias
            w.copy_(block[o:o + w.numel()].view(w.shape[1], w.shape[0]).t()); o += w.numel()
            b.copy_(block[o:o + b.numel()]); o += b.numel()


def unpack_entity_actor(block, actor):
    """`pack_entity_actor` backwards: `copy_` of the block's floats into the parameters of `actor` (unpack(pack(x)) is x bit for bit)."""
    _unpack_entity(block, actor)


def unpack_entity_critic(block, critic):
    """`pack_entity_critic` backwards: `copy_` of the block's floats into the parameters of `critic`."""
    _unpack_entity(block, critic)


class EntityPPOLearner(PPOLearner):
    """`PPOLearner` with the set networks of `build_entity_networks` over packed entity rows and 3-vector actions.  `evaluate`,
    `get_value`, `cal_rt_adv`, `minibatch_loss`, `update`, the data-parallel gradient exchange and the checkpoints are inherited.
    Unlike the image learner's, the log-probabilities `get_action` stores are the ones `evaluate` recomputes at unchanged weights
    (float32 rounding apart): the first minibatch of an update has ratio 1."""

    _logp_dims = (1,)                                          # the action is a 3-vector: `get_action` gives (action [n, 3], log-prob [n])
    _pad_on_cpu = True                                         # a small set of GEMM shapes everywhere; the padding cannot change a row's output

    def __init__(self, args, num_agent, device, model_path=None, infer_chunk=1024, process_group=None, min_bucket=16):
        super().__init__(args, num_agent, 0, device, model_path, infer_chunk, process_group, None, min_bucket)

    def _build_networks(self):
        self._cl = False
        Actor, Critic = build_entity_networks(self.num_agent)
        return ([Actor().to(self.device) for _ in range(self.num_agent)], [Critic().to(self.device) for _ in range(self.num_agent)])

    def _forward(self, net, x, inference=False):
        return net(x)

    def packed_actors(self):
        """The actors as `wrsn_entity_act` takes them: a new float32 tensor [M, P] on the device, built from the parameters as they are
        now.  Nothing here keeps it: whoever does must rebuild it after every `update` and every checkpoint load."""
        return self.torch.stack([pack_entity_actor(a) for a in self.actors]).contiguous()


class DeviceUpdateDriver(RolloutDriver):
    """`RolloutDriver` for the two entity trainers, whose `update` may run on the device: the options' state, the block-layout Adam state and
    gradient tensors, `_values`, `update` per charger, `update_all`, the fused `_prepare_batches` and the packing at the start of
    `roll_out`.  The options are documented at the trainers.  A trainer says what differs:"""

    _update_option = None                                      # the name of its public option: "fused_update" / "device_update"
    _action_width = None                                       # floats of a stored action
    _pack_actor = _unpack_actor = None                         # the actor's block layout (staticmethods); the critic's is pack_entity_critic
    _pa, _pc = None, _lib.ENTITY_CRITIC_FLOATS                 # floats of the actor's and the critic's block
    _env_calls = None                                          # the names of env's (gradient, gradient multi, Adam multi, update) calls
    _critic_only = False                                       # `pretrain(critic_iters=...)`: `_update_charger` skips the actor's Adam call

    def _init_options(self, env, fused_policy, on_device, joint_update, fused_prepare, log_episodes, episode_slots):
        """The tail of both constructors, after `_attach`; on_device: the value of the `_update_option` argument."""
        opt = self._update_option
        self.log_episodes = bool(log_episodes)
        if self.log_episodes:
            self._ledger = env.new_episode_log(episode_slots, quota=0)
        self.fused_policy = bool(fused_policy)
        self._packed = None                                   # packed_actors() of the weights as they are now, or None: rebuilt before use
        setattr(self, opt, bool(on_device))
        self.joint_update = bool(joint_update)
        self.fused_prepare = bool(fused_prepare)               # needs the device update: the values must be the HIP critic's for the two paths to agree
        for k in ("joint_update", "fused_prepare"):
            if getattr(self, k) and not on_device:
                raise ValueError("%s=True needs %s=True" % (k, opt))
        self._joint_per_step = False                          # tests: the per-step path of `update_all` (the data-parallel one) at world == 1
        self.first_minibatch_stats = [None] * self.num_agent  # device update: (loss, pg, v_loss, entropy, approx_kl, clipfrac) of an update's first minibatch
        if on_device:
            z = lambda n: self.torch.zeros(n, dtype=self.torch.float32, device=env.device)
            self._grad = z(self._pa + self._pc)               # ONE tensor: what the data-parallel exchange reduces
            self._grad_all = None                             # joint_update: the same for every charger, [M, P_actor + P_critic], at first use
            self._adam = [dict(m_a=z(self._pa), v_a=z(self._pa), m_c=z(self._pc), v_c=z(self._pc), step=0) for _ in range(self.num_agent)]

    @property
    def _on_device(self):
        return getattr(self, self._update_option)

    def roll_out(self, max_launches=100000, fresh_episodes=False):
        if self.fused_policy:
            self._packed = self.packed_actors()
        return super().roll_out(max_launches, fresh_episodes)

    def update(self, id, batch, shuffle=np.random.shuffle):
        self._packed = None                                   # the weights change: never carried across an update
        if self._on_device:
            return self._update_charger(id, batch, shuffle)
        return super().update(id, batch, shuffle)

    def _values(self, agent_id, states):
        if not self._on_device:
            return super()._values(agent_id, states)
        torch = self.torch
        blk = pack_entity_critic(self.critics[agent_id]).to(self.env.device)
        return self.env.entity_eval(states.to(torch.float32).contiguous(), critic=blk)[2]

    def _update_charger(self, id, batch, shuffle):
        """`PPOLearner.update` of one charger on the device: the same epochs, the same shuffles and minibatches, the same return value."""
        torch, env = self.torch, self.env
        ppo_grad = getattr(env, self._env_calls[0])
        dev = env.device
        f32 = lambda x: x.to(device=dev, dtype=torch.float32).contiguous()
        blk_a, blk_c = f32(self._pack_actor(self.actors[id])), f32(pack_entity_critic(self.critics[id]))
        rows = f32(batch["states"])
        b = {"actions": f32(batch["actions"]).reshape(-1, self._action_width), "log_probs": f32(batch["log_probs"]), "advantages": f32(batch["advantages"]),
             "returns": f32(batch["returns"]), "values": f32(batch["values"])}
        hyper = dict(clip=self.clip, ent_coef=self.ent_coef, vf_coef=self.vf_coef, norm_adv=self.norm_adv, clip_vloss=self.clip_vloss)
        per_epoch = (self.batch_size + self.minibatch_size - 1) // self.minibatch_size
        table = torch.zeros((self.n_updates_per_iteration * per_epoch, 8), dtype=torch.float32, device=dev)
        st, ga, gc, lr = self._adam[id], self._grad[:self._pa], self._grad[self._pa:], self.args["lr"]
        b_inds = np.arange(self.batch_size)
        k, keep = 0, []
        for _ in range(self.n_updates_per_iteration):
            shuffle(b_inds)
            idx = torch.from_numpy(b_inds.astype(np.int32)).to(dev)      # uploaded once per epoch
            keep.append(idx)                                          # the launches are asynchronous: alive until the table is read
            for start in range(0, self.batch_size, self.minibatch_size):
                ppo_grad(blk_a, blk_c, rows, idx[start:start + self.minibatch_size], b, hyper, self._grad, table[k])
                if self.world > 1:
                    torch.distributed.all_reduce(self._grad, group=self.group)
                    self._grad /= self.world
                st["step"] += 1
                if not self._critic_only:                             # `pretrain(critic_iters=...)`: the actor's block and moments stay as they are
                    env.entity_adam(blk_a, ga, st["m_a"], st["v_a"], st["step"], lr, self.max_grad_norm)
                env.entity_adam(blk_c, gc, st["m_c"], st["v_c"], st["step"], lr, self.max_grad_norm)
                k += 1
        self._unpack_actor(blk_a, self.actors[id]); unpack_entity_critic(blk_c, self.critics[id])
        t = table.cpu().numpy().astype(np.float64)                   # the one read of the update
        self.loggers[id]["losses"].extend(float(x) for x in t[:, 0])
        self.first_minibatch_stats[id] = tuple(float(x) for x in t[0, :6])
        return (float(t[-1, 1]), float(t[-1, 2]), float(t[-1, 3]), float(t[-1, 4]), float(np.mean(t[:, 5])))

    def update_all(self, batches, shuffle=np.random.shuffle):
        """`update(id, batches[id])` for every charger at once (joint_update): the list of the tuples `update` returns.  The shuffles are
        drawn in the order the per-charger loop draws them (charger 0's epochs, then charger 1's, ...), so under one seed the two paths
        give the same bytes.  One process: one index upload and one update call of the environment (`entity_ppo_update` /
        `entity_pointer_ppo_update`).  Data-parallel (or `_joint_per_step`): per minibatch step one multi-group gradient call into one
        flat [M (P_actor + P_critic)] tensor, one all-reduce of it, one multi-group Adam call."""
        if not self.joint_update:
            raise ValueError("update_all needs joint_update=True")
        self._packed = None
        torch, env = self.torch, self.env
        _, grad_multi, adam_multi, ppo_update = (getattr(env, k) for k in self._env_calls)
        dev, M = env.device, self.num_agent
        f32 = lambda x: x.to(device=dev, dtype=torch.float32).contiguous()
        epochs, bs, mb = self.n_updates_per_iteration, self.batch_size, self.minibatch_size
        per_epoch = (bs + mb - 1) // mb
        steps = epochs * per_epoch
        if self._grad_all is None:
            self._grad_all = torch.zeros((M, self._pa + self._pc), dtype=torch.float32, device=dev)   # ONE tensor: what the exchange reduces
        groups = []
        for id in range(M):
            batch, st = batches[id], self._adam[id]
            b = {"actions": f32(batch["actions"]).reshape(-1, self._action_width), "log_probs": f32(batch["log_probs"]), "advantages": f32(batch["advantages"]),
                 "returns": f32(batch["returns"]), "values": f32(batch["values"])}
            groups.append(dict(actor=f32(self._pack_actor(self.actors[id])), critic=f32(pack_entity_critic(self.critics[id])), grad=self._grad_all[id],
                               rows=f32(batch["states"]), batch=b, m_a=st["m_a"], v_a=st["v_a"], m_c=st["m_c"], v_c=st["v_c"], step=st["step"]))
        idx_np = np.empty((M, epochs, bs), dtype=np.int32)
        for id in range(M):
            b_inds = np.arange(bs)
            for e in range(epochs):
                shuffle(b_inds)
                idx_np[id, e] = b_inds
        idx = torch.from_numpy(idx_np).to(dev)                       # the one upload of the update
        hyper = dict(clip=self.clip, ent_coef=self.ent_coef, vf_coef=self.vf_coef, norm_adv=self.norm_adv, clip_vloss=self.clip_vloss)
        lr = self.args["lr"]
        if self.world == 1 and not self._joint_per_step:
            table = torch.zeros((M, steps, 8), dtype=torch.float32, device=dev)
            ppo_update(groups, idx, mb, hyper, table, lr, self.max_grad_norm)
            for st in self._adam:
                st["step"] += steps
        else:
            by_step = torch.zeros((steps, M, 8), dtype=torch.float32, device=dev)
            k, keep = 0, []
            for e in range(epochs):
                for start in range(0, bs, mb):
                    mbi = idx[:, e, start:start + mb].contiguous()
                    keep.append(mbi)                                  # the launches are asynchronous: alive until the table is read
                    grad_multi(groups, mbi, hyper, by_step[k])
                    if self.world > 1:
                        torch.distributed.all_reduce(self._grad_all, group=self.group)
                        self._grad_all /= self.world
                    adam_multi(groups, lr, self.max_grad_norm)
                    for g, st in zip(groups, self._adam):
                        st["step"] += 1; g["step"] = st["step"]
                    k += 1
            table = by_step.permute(1, 0, 2)
        for id, g in enumerate(groups):
            self._unpack_actor(g["actor"], self.actors[id]); unpack_entity_critic(g["critic"], self.critics[id])
        t = table.cpu().numpy().astype(np.float64)                   # the one read of the update
        out = []
        for id in range(M):
            self.loggers[id]["losses"].extend(float(x) for x in t[id, :, 0])
            self.first_minibatch_stats[id] = tuple(float(x) for x in t[id, 0, :6])
            out.append((float(t[id, -1, 1]), float(t[id, -1, 2]), float(t[id, -1, 3]), float(t[id, -1, 4]), float(np.mean(t[id, :, 5]))))
        return out

    def _prepare_batches(self):
        """With fused_prepare the tail of `roll_out` on the device.  Stored actions of 3 floats (the set policy): `wrsn_entity_prepare`
        gathers the actions itself.  Of 2 (the node-pointer policy): its `out_action` stays NULL and the [M, batch_size, 2] stored pairs
        are gathered from `buffers.action` with the uploaded index by one torch gather on the device."""
        if not self.fused_prepare:
            return super()._prepare_batches()
        torch, env, buf, width = self.torch, self.env, self.buffers, self._action_width
        dev, M, bs = env.device, self.num_agent, self.batch_size
        if not self.gae:                                      # the reference's plain branch raises (`cal_rt_adv`): the same, before any launch
            raise IndexError("index %d is out of bounds for dimension 0 with size %d" % (bs, bs))
        stored = buf.stored()
        host = buf.reward[:, :max(stored)].cpu().numpy()      # the one host read
        idx_np = np.empty((M, bs), dtype=np.int32)
        for a in range(M):                                    # in charger order: the `np.random` stream of the default path
            idx_np[a] = select_batch(host[a, :stored[a]], bs)
        idx = torch.from_numpy(idx_np).to(dev)                # the one upload
        critics = torch.stack([pack_entity_critic(c) for c in self.critics]).to(device=dev, dtype=torch.float32).contiguous()
        new = lambda *sh: torch.empty((M, bs) + sh, dtype=torch.float32, device=dev)
        R = buf.row_elems
        o = dict(value=new(), advantage=new(), ret=new(), out_state=new(R), out_next_state=new(R))
        if width == 3:
            o["out_action"] = new(3)
        o.update(out_logp=new(),
                 out_reward=torch.empty((M, (-bs) % 64 + bs), dtype=torch.float32, device=dev)[:, :bs])    # every charger's rewards start on a 256-byte boundary, as a tensor of their own would
        groups = []
        for a in range(M):
            g = dict(critic=critics[a], state=buf.state[a], next_state=buf.next_state[a], reward=buf.reward[a], logp=buf.logp[a])
            if width == 3:
                g["action"] = buf.action[a]
            g.update({k: v[a] for k, v in o.items()})
            groups.append(g)
        env.entity_prepare(groups, idx, self.gamma, self.gae_lambda)       # stored terminal flags are all 0: terminal = NULL
        acts = o["out_action"] if width == 3 else buf.action.gather(1, idx.long().unsqueeze(2).expand(M, bs, width))
        out = [dict(states=o["out_state"][a], actions=self._stored_actions(acts[a]), log_probs=o["out_logp"][a], rewards=o["out_reward"][a],
                    next_states=o["out_next_state"][a], advantages=o["advantage"][a], returns=o["ret"][a], values=o["value"][a]) for a in range(M)]
        # the logged mean is torch's float32 reduction of the gathered rewards -- the default path's `float(rew.mean())` on the same floats
        means = torch.stack([b["rewards"].mean() for b in out]).cpu()
        for a in range(M):
            self.loggers[a]["rewards"].append(float(means[a]))
        return out


class BatchedEntityIPPO(DeviceUpdateDriver, EntityPPOLearner):
    """The roll-out of `BatchedIPPO` on entity rows: `VecWRSN(entities=True)` (no image needed: `render=False`), the set policy's
    3-vector is the action `env.step` takes, and the transitions live in `EntityTransitionBuffers`.

    fused_policy : True = the device chooses the actions itself (`VecWRSN.entity_act`, `wrsn_entity_act`): one call on the entity rows the
                   environment holds, with the actors packed at the start of the roll-out (`packed_actors`) and standard-normal draws
                   of `torch.randn`; no row gathering and no per-charger forward pass.  False (the default): `get_action` per charger.
    fused_update : True = `update` runs on the device (`wrsn_entity_ppo_grad`, `wrsn_entity_adam`): per minibatch one gradient call into
                   one flat tensor, (data-parallel: one all-reduce of it,) one Adam call each for actor and critic, nothing read back
                   until the update is over; `_values` (hence `cal_rt_adv`) goes through `wrsn_entity_eval`.  The modules stay the source
                   of truth between updates (they are packed at the start of `update` and written back at its end, so checkpoints load
                   and save as ever), but the Adam moments and step counts live in this object in block layout and the torch optimisers
                   are never stepped.  The mode is fixed at construction.  False (the default): the PyTorch update, no new launch.
    joint_update : True (needs fused_update) = `train` updates every charger at once through `update_all`: the chargers are independent
                   learners, so their minibatch steps go through the same launches (`wrsn_entity_ppo_update`; data-parallel: per step
                   `wrsn_entity_ppo_grad_multi`, one all-reduce, `wrsn_entity_adam_multi`).  Bit for bit what `update` per charger gives
                   under the same shuffles.  False (the default): nothing new is launched.
    fused_prepare: True (needs fused_update: the values must be the HIP critic's for the two paths to agree) = the tail of `roll_out` runs on
                   the device (`wrsn_entity_prepare`): one host read of the stored rewards, the reference's selection per charger on the
                   host (the `np.random` stream of the default path), one index upload, the critics packed once, and ONE call that
                   writes every charger's values, advantages, returns and gathered rows into [M, batch_size, ...] tensors; the batch
                   dicts hold per-charger views of them, bit for bit what the default path returns.  False (the default): the
                   per-charger `index_select`s and `cal_rt_adv`, no new launch.
    log_episodes : True = every launch of the roll-out also runs the episode ledger (`wrsn_episodes_collect`, never parking, no time limit,
                   not consuming) in front of the buffers' collect, and every row `train` logs gains `avg_ep_lifetime`, `avg_ep_lens`
                   and `episodes` over the episodes that closed in that iteration (at most `episode_slots` per environment are kept;
                   more are counted in `episodes` only).  Batches, weights and optimiser state are unchanged, bit for bit.  False (the
                   default): nothing new is launched and the rows have the keys they always had.

    `evaluate_episodes(eval_env, ...)` measures the policy over whole episodes on ANOTHER batch of environments (`evaluate.evaluate_policy`;
    `evaluate` itself is the reference's `evaluate(agent, states, actions)` of the learner)."""

    _check_status = True
    _update_option, _action_width, _pa = "fused_update", 3, _lib.ENTITY_ACTOR_FLOATS
    _pack_actor, _unpack_actor = staticmethod(pack_entity_actor), staticmethod(unpack_entity_actor)
    _env_calls = ("entity_ppo_grad", "entity_ppo_grad_multi", "entity_adam_multi", "entity_ppo_update")

    def __init__(self, args, env, device=None, model_path=None, capacity=None, infer_chunk=1024, process_group=None, log=None, min_bucket=16,
                 fused_policy=False, fused_update=False, joint_update=False, fused_prepare=False, log_episodes=False, episode_slots=64):
        if not getattr(env, "entities", False):
            raise ValueError("BatchedEntityIPPO needs a VecWRSN with the entity observation (entities=True)")
        super().__init__(args, env.num_agent, device if device is not None else env.device, model_path, infer_chunk, process_group, min_bucket)
        self._attach(env, EntityTransitionBuffers(env, capacity or 2 * self.batch_size, 3), log)
        self._init_options(env, fused_policy, fused_update, joint_update, fused_prepare, log_episodes, episode_slots)

    def evaluate_episodes(self, eval_env, episodes=1, deterministic=True, generator=None, **kw):
        """`evaluate_policy` of the actors as they are now -- their mode, or with deterministic=False a sample per decision -- on
        `eval_env`, a `VecWRSN(entities=True, auto_reset=False)` with this trainer's number of chargers; `kw` goes to `evaluate_policy`.
        ValueError when `eval_env` is the trainer's own batch: its environments live across roll-outs and must not be disturbed."""
        from .evaluate import EntityPolicy, evaluate_policy
        if eval_env is self.env:
            raise ValueError("evaluate on a batch of its own: the trainer's environments live across roll-outs")
        return evaluate_policy(eval_env, EntityPolicy(self.packed_actors(), deterministic, generator), episodes, **kw)

    def _choose(self, r, ids):
        if not self.fused_policy:
            return self._choose_per_charger(ids, 3, lambda rows: EntityTransitionBuffers.pack(
                r["nodes"].index_select(0, rows), r["chargers"].index_select(0, rows), r["env_feat"].index_select(0, rows))) + (None,)
        torch, env = self.torch, self.env                     # the policy on the device: draw eps, `entity_act`
        if self._packed is None:
            self._packed = self.packed_actors()
        eps = torch.randn((env.num_env, 3), dtype=torch.float32, device=env.device)
        act3, act64, logp = env.entity_act(ids, self._packed, eps)
        return act3, logp, act64


# ------------------------------------------------------------------------------------------------------------------
# the node-pointer entity policy: a learner and a trainer next to the Gaussian set policy's
# ------------------------------------------------------------------------------------------------------------------
class EntityPointerPPOLearner(EntityPPOLearner):
    """`EntityPPOLearner` with the actors of `build_entity_pointer_networks`.  A decision is stored as two floats, (node, x): the chosen
    node's index (-1: no node was alive) and the raw charge variable; `evaluate` recomputes its log-probability from them and the stored
    row.  `minibatch_loss`, `update`, the data-parallel gradient exchange and the checkpoints are inherited."""

    mask_claimed = False                                      # BatchedEntityPointerIPPO sets it before the networks are built

    def _build_networks(self):
        self._cl = False
        Actor, Critic = build_entity_pointer_networks(self.num_agent, self.mask_claimed)
        return ([Actor().to(self.device) for _ in range(self.num_agent)], [Critic().to(self.device) for _ in range(self.num_agent)])

    def get_action(self, agent_id, states):
        """Packed rows [n, R] -> (stored [n, 2] = (node, x), log-probability [n]): Gumbel noise -log(-log(u)) per node and a
        standard-normal draw per row, u from `torch.rand`."""
        torch = self.torch
        outs, lps = [], []
        with torch.no_grad():
            for s in states.split(self.infer_chunk):
                n, N = s.shape[0], EntityTransitionBuffers.split(s, self.num_agent)[0].shape[1]
                g = -torch.log(-torch.log(torch.rand((n, N), dtype=torch.float32, device=s.device)))
                d = self.actors[agent_id].act(s, g, torch.randn((n,), dtype=torch.float32, device=s.device))
                outs.append(torch.stack([d["node"].to(d["x"].dtype), d["x"]], 1)); lps.append(d["logp"])
        return torch.cat(outs), torch.cat(lps)

    def evaluate(self, agent_id, batch_states, batch_actions):
        """(log-probability [n], entropy [n]) of the stored decisions `batch_actions` [n, 2] = (node, x) on `batch_states`."""
        return self.actors[agent_id](batch_states, batch_actions[:, 0], batch_actions[:, 1])

    def packed_actors(self):
        """The actors as `wrsn_entity_pointer_act` takes them: a new float32 tensor [M, P] on the device, built from the parameters as
        they are now."""
        return self.torch.stack([pack_entity_pointer_actor(a) for a in self.actors]).contiguous()


class BatchedEntityPointerIPPO(DeviceUpdateDriver, EntityPointerPPOLearner):
    """The roll-out of `BatchedEntityIPPO` with the node-pointer policy: `VecWRSN(entities=True)`, transitions in
    `EntityTransitionBuffers(action_elems=2)` -- (node, x) per decision --, the PyTorch update of `PPOLearner`.

    min_charge   : the third component of every action is min_charge + (1 - min_charge) sigmoid(x): with min_charge > 0 (default 0.02)
                   every decision spends at least min_charge * charging_time_max seconds of simulated time, so a request cannot come back
                   at the same instant forever.
    fused_policy : True = the device chooses (`VecWRSN.entity_pointer_act`, `wrsn_entity_pointer_act`): one call on the entity rows the
                   environment holds, with the actors packed at the start of the roll-out and noise derived from `torch.rand` /
                   `torch.randn`.  False (the default): `get_action` per charger.
    log_episodes : as `BatchedEntityIPPO`.

    device_update: True = `update` runs on the device for ONE learner per call (`wrsn_entity_pointer_ppo_grad`, `wrsn_entity_adam`): the
                   actor and critic are packed at its start (`pack_entity_pointer_actor`, `pack_entity_critic`), the epochs, shuffles and
                   minibatches are `PPOLearner.update`'s with one int32 index upload per epoch, and per minibatch there is one gradient call
                   into one flat tensor [P_pointer + P_critic], (data-parallel: one all-reduce of it,) and one Adam call each for actor and
                   critic; the statistics go to a device table read once at the end, when the blocks are unpacked into the modules.  The
                   Adam moments and step counts live in this object in block layout and the torch optimisers are never stepped; `_values`
                   goes through `wrsn_entity_eval`.  The same return value as the default; `first_minibatch_stats` is filled.  The mode is
                   fixed at construction.  False (the default): the PyTorch update, nothing new is launched.

    joint_update : True (needs device_update) = `train` updates every charger at once through `update_all`, as `BatchedEntityIPPO` does:
                   one index upload and one `wrsn_entity_pointer_ppo_update` (data-parallel: per step
                   `wrsn_entity_pointer_ppo_grad_multi`, one all-reduce, `wrsn_entity_pointer_adam_multi`) -- ten gradient and two Adam
                   launches per minibatch step however many chargers there are.  Bit for bit what `update` per charger gives under
                   the same shuffles.  False (the default): nothing new is launched.
    fused_prepare: True (needs device_update) = the tail of `roll_out` runs on the device as `BatchedEntityIPPO`'s does
                   (`wrsn_entity_prepare` with `out_action` NULL); the [M, batch_size, 2] stored pairs are gathered from the buffers with
                   the uploaded index by one torch gather.  The batch dicts are bit for bit the default path's.  False (the default):
                   the per-charger `index_select`s and `cal_rt_adv`.

    mask_claimed : True = the actors choose among the candidates of a row, not its alive nodes (`build_entity_pointer_networks`,
                   `VecWRSN.set_entity_pointer_mask`): never a node inside the charging disc around another live charger's destination
                   while another alive node is left.  The modules are built with the flag and the mode is set on `env` at construction
                   and on the evaluation batch by `evaluate_episodes`, so every path -- acting in PyTorch or on the device, the update
                   in PyTorch or on the device, per charger or joint -- recomputes under the mask what acting stored.  False (the
                   default): every alive node, and `env` is set to that.

    `fused_update` is the set policy's option (BatchedEntityIPPO) and always raises here: this actor's is `device_update`."""

    _check_status = True
    _update_option, _action_width, _pa = "device_update", 2, _lib.ENTITY_POINTER_FLOATS
    _pack_actor, _unpack_actor = staticmethod(pack_entity_pointer_actor), staticmethod(unpack_entity_pointer_actor)
    _env_calls = ("entity_pointer_ppo_grad", "entity_pointer_ppo_grad_multi", "entity_pointer_adam_multi", "entity_pointer_ppo_update")

    def __init__(self, args, env, device=None, model_path=None, capacity=None, infer_chunk=1024, process_group=None, log=None, min_bucket=16,
                 min_charge=0.02, fused_policy=False, log_episodes=False, episode_slots=64, fused_update=False, joint_update=False,
                 fused_prepare=False, device_update=False, mask_claimed=False):
        if fused_update:
            raise ValueError("BatchedEntityPointerIPPO has no fused_update: that is the Gaussian set policy's option (BatchedEntityIPPO); "
                             "this actor's is device_update")
        if not getattr(env, "entities", False):
            raise ValueError("BatchedEntityPointerIPPO needs a VecWRSN with the entity observation (entities=True)")
        if not 0.0 <= float(min_charge) < 1.0:
            raise ValueError("min_charge must lie in [0, 1)")
        self.mask_claimed = bool(mask_claimed)                # before the networks are built
        super().__init__(args, env.num_agent, device if device is not None else env.device, model_path, infer_chunk, process_group, min_bucket)
        self._attach(env, EntityTransitionBuffers(env, capacity or 2 * self.batch_size, 2), log)
        env._h.set_entity_pointer_mask(_lib.POINTER_MASK_CLAIMED if self.mask_claimed else _lib.POINTER_MASK_NONE)   # `VecWRSN.set_entity_pointer_mask`
        self.min_charge = float(min_charge)
        self._bc = None                                       # `pretrain`: the imitation settings while it collects, else None
        self._init_options(env, fused_policy, device_update, joint_update, fused_prepare, log_episodes, episode_slots)

    def evaluate_episodes(self, eval_env, episodes=1, deterministic=True, generator=None, **kw):
        """`evaluate_policy` of the actors as they are now (`evaluate.PointerPolicy`) on `eval_env`, another batch than the trainer's."""
        from .evaluate import PointerPolicy, evaluate_policy
        if eval_env is self.env:
            raise ValueError("evaluate on a batch of its own: the trainer's environments live across roll-outs")
        return evaluate_policy(eval_env, PointerPolicy(self.packed_actors(), deterministic, generator, self.min_charge, self.mask_claimed),
                               episodes, **kw)

    def pretrain(self, iters, beta=1.0, beta_end=None, epochs=None, ent_coef=0.0, charge_scale=1.0, x_clip=4.0, critic_iters=0, max_launches=100000):
        """Imitation pretraining from the heuristic (`wrsn_entity_heuristic_label`, `wrsn_entity_pointer_bc_update`): `iters` iterations of
        collect-and-clone as a warm start that `train` then fine-tunes.  Needs device_update=True; works with and without mask_claimed,
        fused_policy, joint_update and fused_prepare.

        Collection goes through `step_batch` and the transition buffers.  Per launch `entity_heuristic_label` gives the expert's stored
        pair and action for the requesting rows; a per-row uniform draw executes the expert's action with probability beta_i and the
        learner's sampled action (`entity_pointer_act` with fused_policy, `get_action` without) otherwise, beta_i going linearly from
        `beta` in the first iteration to `beta_end` (default: `beta`) in the last.  With beta_i == 1 the learner is never asked and no
        draw is made.  The pair RECORDED for a row is always the expert's (DAgger; beta = 1 throughout is plain behaviour cloning on the
        heuristic's own trajectories).  The buffers' rules stay: each charger's first transition is dropped, and pending decisions are
        discarded at a terminal return -- so the decisions just before a network dies are never cloned.  Rewards ride along unused; the
        stored log-probabilities are zeros.  Pending decisions from before the call are dropped at its start and its own at its end, so
        no PPO batch ever holds a label and no cloning batch a learner's decision.  The executed expert action is the heuristic's own
        (its c, not the squashed one): on networks where the heuristic stands still (a full node under the charger, c = 0: DESIGN.md
        section 19) a row asks again at the same instant for ever, the other chargers of that environment never ask, and the
        collection ends at `max_launches` with a RuntimeError.

        Per iteration, once every charger holds batch_size transitions, its first batch_size stored transitions are the batch;
        `epochs` (default n_updates_per_iteration) uniform random permutations per charger are drawn from `np.random` (not
        `select_batch`, which is reward-driven) and ONE `entity_pointer_bc_update` steps every charger's actor block: minibatch_size,
        lr and max_grad_norm are the trainer's, the Adam moments and step counts are the block-layout state `device_update` keeps, so
        PPO continues from them.  No critic is touched.  The blocks are unpacked into the modules at the end (and after every iteration
        in which the unfused learner may be asked).

        critic_iters > 0: afterwards that many ordinary iterations (`roll_out`, then `_update_charger` per charger -- also with
        joint_update=True) in which the actor's Adam call is skipped, so that fine-tuning does not start from an untrained value
        function.  The shared step count of a charger advances in them as in any update.

        Returns one dict per iteration and charger: iteration, agent, beta, `first` and `last` -- the first and last row of the device
        table (loss, -mean logp, node part, charge part, mean entropy, top-1, share of rows with a live stored node, 0), read once per
        iteration."""
        if not self.device_update:
            raise ValueError("pretrain needs device_update=True")
        torch, env = self.torch, self.env
        if not env.auto_reset:
            raise ValueError("%s needs VecWRSN(auto_reset=True)" % type(self).__name__)
        iters, dev, M, bs, mb = int(iters), env.device, self.num_agent, self.batch_size, self.minibatch_size
        beta_end = beta if beta_end is None else beta_end
        epochs = self.n_updates_per_iteration if epochs is None else int(epochs)
        steps = epochs * ((bs + mb - 1) // mb)
        if self._grad_all is None:
            self._grad_all = torch.zeros((M, self._pa + self._pc), dtype=torch.float32, device=dev)
        blocks = self.packed_actors().to(device=dev, dtype=torch.float32).contiguous()      # [M, P]: stepped in place
        if self._req is None:
            self.buffers.clear(); self._req = env.reset()
            if self._ledger is not None:
                env.episodes_collect(self._ledger, 0.0, consume=False)
        out = []
        try:
            for i in range(iters):
                b = float(beta) if iters <= 1 else float(beta) + (float(beta_end) - float(beta)) * i / (iters - 1)
                self._bc = dict(beta=b, charge_scale=float(charge_scale), x_clip=float(x_clip))
                self._packed = blocks if self.fused_policy else None      # the learner acts with the blocks as the last update left them
                self.buffers.clear(keep_pending=i > 0)                    # pending decisions from before the call are no labels: dropped
                for _ in range(max_launches):
                    self.step_batch()
                    if min(self.buffers.counts()) >= bs:
                        break
                if min(self.buffers.stored()) < bs:
                    raise RuntimeError("pretrain stopped after %d launches with %s transitions per charger, fewer than batch_size %d (buffer "
                                       "capacity %d)" % (max_launches, self.buffers.stored(), bs, self.buffers.capacity))
                idx_np = np.stack([np.stack([np.random.permutation(bs) for _ in range(epochs)]) for _ in range(M)]).astype(np.int32)
                idx = torch.from_numpy(idx_np).to(dev)                    # the one upload of the iteration
                groups = [dict(actor=blocks[a], grad=self._grad_all[a], rows=self.buffers.state[a, :bs], stored=self.buffers.action[a, :bs],
                               m_a=self._adam[a]["m_a"], v_a=self._adam[a]["v_a"], step=self._adam[a]["step"]) for a in range(M)]
                table = torch.zeros((M, steps, 8), dtype=torch.float32, device=dev)
                env.entity_pointer_bc_update(groups, idx, mb, float(ent_coef), table, self.args["lr"], self.max_grad_norm)
                for st in self._adam:
                    st["step"] += steps
                self.bc_index = idx_np                                    # the permutations of the last update (tests, logging)
                ends = table[:, [0, steps - 1]].cpu().numpy().astype(np.float64)      # the one read of the iteration
                for a in range(M):
                    out.append(dict(iteration=i, agent=a, beta=b, first=tuple(float(x) for x in ends[a, 0]), last=tuple(float(x) for x in ends[a, 1])))
                    if self.log:
                        self.log(out[-1])
                if not self.fused_policy and (float(beta) < 1.0 or float(beta_end) < 1.0):
                    for a in range(M):
                        unpack_entity_pointer_actor(blocks[a], self.actors[a])
        finally:
            self._bc = None
            self._packed = None
        for a in range(M):
            unpack_entity_pointer_actor(blocks[a], self.actors[a])
        self.buffers.clear()                                              # the pending labels: not a PPO roll-out's business
        self._critic_only = True
        try:
            for _ in range(int(critic_iters)):
                batches = self.roll_out(max_launches)
                for a in range(M):
                    self._packed = None
                    self._update_charger(a, batches[a], np.random.shuffle)
        finally:
            self._critic_only = False
        return out

    def _choose_bc(self, r, ids):
        """`_choose` while `pretrain` collects: the expert's stored pair is recorded, the executed action is the expert's with probability
        beta per row and the learner's sample otherwise."""
        torch, env, bc = self.torch, self.env, self._bc
        stored, _, act64 = env.entity_heuristic_label(ids, bc["charge_scale"], self.min_charge, bc["x_clip"])
        stored, act64 = stored.clone(), act64.clone()                     # the environment writes its own tensors again at the next call
        logp = torch.zeros((env.num_env,), dtype=torch.float32, device=env.device)
        if bc["beta"] < 1.0:
            mine, _, handed = self._choose_learner(r, ids)
            own = handed if handed is not None else self.stored_action3(mine).double()
            expert = torch.rand((env.num_env,), dtype=torch.float32, device=env.device) < bc["beta"]
            act64 = torch.where(expert.unsqueeze(1), act64, own)
        self._handed = act64
        return stored, logp, act64

    def _choose(self, r, ids):
        if self._bc is not None:
            return self._choose_bc(r, ids)
        return self._choose_learner(r, ids)

    def _choose_learner(self, r, ids):
        torch, env = self.torch, self.env
        if not self.fused_policy:
            return self._choose_per_charger(ids, 2, lambda rows: EntityTransitionBuffers.pack(
                r["nodes"].index_select(0, rows), r["chargers"].index_select(0, rows), r["env_feat"].index_select(0, rows))) + (None,)
        if self._packed is None:
            self._packed = self.packed_actors()
        g = -torch.log(-torch.log(torch.rand((env.num_env, env.n_node), dtype=torch.float32, device=env.device)))
        eps = torch.randn((env.num_env,), dtype=torch.float32, device=env.device)
        stored, act64, logp, _ = env.entity_pointer_act(ids, self._packed, g, eps, self.min_charge)
        self._handed = act64
        return stored, logp, act64

    def _action3(self, ids, stored):
        """The 3-vector of a launch: the device's own when it chose (fused_policy), else `stored_action3`."""
        return self._handed if self.fused_policy or self._bc is not None else self.stored_action3(stored)

    def stored_action3(self, stored):
        """(u, v) of the stored node from the request's node rows -- the asking charger's own position for node -1 --, and the squashed x:
        what `wrsn_entity_pointer_act` writes as `action` for the same decision (the tests hold the two together)."""
        torch, r = self.torch, self._req
        Actor = type(self.actors[0])
        k = stored[:, 0].long()
        uv = Actor.destination(r["nodes"], r["chargers"], r["env_feat"], k)
        c = self.min_charge + (1.0 - self.min_charge) * torch.sigmoid(stored[:, 1])
        return torch.cat([uv, c.unsqueeze(1)], 1)
