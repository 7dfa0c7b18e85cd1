"""The one roll-out driver and the one transition-buffer base of ippo.py, on the emulated library through sides.EmuVec: `step_batch`
stores, bit for bit, what the three bodies it replaced stored (the unfused entity body is pinned the same way in tests/test_entity_act.py),
and the two buffer classes lay out what they always did."""
import os
import re

from sides import EmuSide, EmuVec

STORED = ("state", "action", "next_state", "reward", "logp", "now", "count", "pend_action", "pend_logp")


def _image_step_batch_before(self):
    """BatchedIPPO.step_batch as it stood before the driver, statement for statement (the timers left out)."""
    torch, env = self.torch, self.env
    r = self._req
    ids = r["agent_id"]
    G = env.map_size
    maps = torch.zeros((env.num_env, G * G), dtype=torch.float32, device=env.device)
    logp = torch.zeros((env.num_env,), dtype=torch.float32, device=env.device)
    for a in range(self.num_agent):
        rows = torch.nonzero(ids == a).flatten()
        if rows.numel() == 0:
            continue
        act, lp = self.get_action(a, r["state"].index_select(0, rows))
        maps.index_copy_(0, rows, act.reshape(rows.numel(), G * G).float()); logp.index_copy_(0, rows, lp.float())
    self.buffers.record(ids, maps, logp)
    act3 = env.density_to_action(ids, maps.view(env.num_env, G, G).double())
    r = env.step(ids.clone(), act3)
    self.buffers.collect()
    self.last_ids, self.last_action3 = ids, act3
    self._req = r
    return r


def _fused_step_batch_before(self):
    """BatchedEntityIPPO._step_batch_fused as it stood before the driver, statement for statement (the timers left out)."""
    torch, env = self.torch, self.env
    r = self._req
    ids = r["agent_id"].clone()
    if self._packed is None:
        self._packed = self.packed_actors()
    eps = torch.randn((env.num_env, 3), dtype=torch.float32, device=env.device)
    act3, act64, logp = env.entity_act(ids, self._packed, eps)
    self.buffers.record(ids, act3, logp)
    r = env.step(ids, act64)
    bad = torch.nonzero(r["status"] < 0).flatten()
    if bad.numel():
        raise RuntimeError("environment rows %s report status %s" % (bad.tolist(), r["status"][bad].tolist()))
    self.buffers.collect()
    self.last_ids, self.last_action3 = ids, act3
    self._req = r
    return r


def _emu_env(entity):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, synth_scenario
    return EmuVec(EmuSide([synth_scenario(300 + e, 70, 60) for e in range(3)], DEFAULT_MC_SPEC, 2, map_size=12, render=not entity,
                          entities=entity, auto_reset=True))


def _stored_by(step, entity, launches=6, **kw):
    """What 6 launches of `step(algo)` leave in the buffers of a freshly seeded trainer, and the 3-vectors they handed out."""
    import torch
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, BatchedIPPO
    torch.set_num_threads(2)
    env = _emu_env(entity)
    torch.manual_seed(11)
    algo = (BatchedEntityIPPO if entity else BatchedIPPO)(dict(batch_size=8, minibatch_size=4, n_updates_per_iteration=1), env, device="cpu", **kw)
    algo.buffers.clear(); algo._req = env.reset()
    torch.manual_seed(12)
    acts = []
    for _ in range(launches):
        step(algo)
        acts.append(algo.last_action3.clone())
    out = {k: getattr(algo.buffers, k).clone() for k in STORED}
    out["last_action3"] = torch.stack(acts)
    env.side.close()
    return out


def _same_bits(before, entity, **kw):
    import torch
    a = _stored_by(lambda algo: algo.step_batch(), entity, **kw)
    b = _stored_by(before, entity, **kw)
    assert int(a["count"].sum()) > 0
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_emulated_image_roll_out_is_untouched():
    """BatchedIPPO.step_batch stores, over a seeded roll-out on the emulator (UNet and critic at a 12 x 12 map), bit for bit what the
    step_batch of before the driver stores."""
    _same_bits(_image_step_batch_before, False)


def test_emulated_fused_roll_out_is_untouched():
    """fused_policy=True: the same for BatchedEntityIPPO._step_batch_fused of before the driver."""
    _same_bits(_fused_step_batch_before, True, fused_policy=True)


def test_transition_buffers_lay_out_what_they_did():
    """Both buffer classes expose the attributes, shapes and dtypes they had as separate classes, and the wrsn_transition_buffers struct
    built from them carries capacity, action_elems and the twelve addresses in the order of include/wrsn_hip.h."""
    import torch
    from multi_agent_rl_wrsn_amd import EntityTransitionBuffers, TransitionBuffers, _lib
    B, M, G, N, C = 3, 2, 12, 70, 5
    f32, names = torch.float32, ("pend_state", "pend_action", "pend_logp", "pend_valid", "state", "action", "next_state", "reward", "logp", "now",
                                 "env_index", "count")
    for entity, A in ((False, G * G), (True, 3)):
        env = _emu_env(entity)
        buf = (EntityTransitionBuffers if entity else TransitionBuffers)(env, C, A)
        row = (8 * N + 12 * M + 8,) if entity else (4, G, G)
        want = dict(pend_state=((B, M) + row, f32), pend_action=((B, M, A), f32), pend_logp=((B, M), f32), pend_valid=((B, M), torch.uint8),
                    state=((M, C) + row, f32), action=((M, C, A), f32), next_state=((M, C) + row, f32), reward=((M, C), f32), logp=((M, C), f32),
                    now=((M, C), torch.float64), env_index=((M, C), torch.int32), count=((M,), torch.int32))
        assert set(vars(buf)) == set(names) | {"env", "capacity", "action_elems", "_c"} | ({"row_elems"} if entity else set())
        assert (buf.capacity, buf.action_elems) == (C, A) and (not entity or buf.row_elems == row[0])
        for k in names:
            t = getattr(buf, k)
            assert (tuple(t.shape), t.dtype) == want[k] and t.is_contiguous() and not t.any(), k
        fields = [f for f, _ in _lib.WrsnTransitionBuffers._fields_]
        assert fields == ["capacity", "action_elems"] + [{"env_index": "env"}.get(k, k) for k in names]
        assert [getattr(buf._c, f) for f in fields] == [C, A] + [getattr(buf, k).data_ptr() for k in names]
        env.side.close()


def test_both_trainers_are_learners_on_one_driver():
    from multi_agent_rl_wrsn_amd import BatchedEntityIPPO, BatchedIPPO, EntityPPOLearner, PPOLearner, ippo
    assert issubclass(BatchedIPPO, PPOLearner) and not issubclass(BatchedIPPO, EntityPPOLearner)
    assert issubclass(BatchedEntityIPPO, EntityPPOLearner) and not issubclass(BatchedEntityIPPO, BatchedIPPO)
    assert ippo.DeviceUpdateDriver.__mro__[1] is ippo.RolloutDriver      # the entity trainers' driver: RolloutDriver and the device update
    for cls, driver in ((BatchedIPPO, ippo.RolloutDriver), (BatchedEntityIPPO, ippo.DeviceUpdateDriver)):
        assert cls.__mro__[1] is driver
        for name in ("step_batch", "train", "_sync_time"):
            assert getattr(cls, name) is getattr(ippo.RolloutDriver, name), (cls, name)
    assert BatchedIPPO.roll_out is ippo.RolloutDriver.roll_out
    assert not re.search(r"BatchedIPPO\.(roll_out|train|_sync_time)", open(os.path.splitext(ippo.__file__)[0] + ".py").read())
