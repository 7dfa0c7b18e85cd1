"""The update of several independent learners at once on the device: the bodies of tests/test_entity_update_joint.py on VecSide."""
import pytest
from sides import VecSide, need_gpu

import test_entity_update_joint as body

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", body.GRAD_CASES)
def test_entity_ppo_grad_multi(case):
    body.gradient_matches(VecSide, case)


def test_entity_groups_are_independent():
    body.groups_are_independent(VecSide)


def test_entity_adam_multi():
    body.adam_matches(VecSide)


def test_entity_ppo_update():
    body.update_matches(VecSide)


def test_entity_update_joint_extent():
    body.extent_is_respected(VecSide)


def test_entity_update_joint_bad_arguments():
    body.bad_arguments_leave_everything_untouched(VecSide)


def test_joint_update_trainer():
    """The shapes of test_fused_update_trainer_end_to_end: B = 64, N = 70, M = 3, batch 32, minibatch 16, two epochs."""
    need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario

    def make_env():
        return VecWRSN([synth_scenario(300 + e, 70, 60) for e in range(64)], None, 3, render=False, entities=True, auto_reset=True, step_budget=1250)

    body.trainer_paths_agree(make_env, dict(batch_size=32, minibatch_size=16, n_updates_per_iteration=2), 100).close()
