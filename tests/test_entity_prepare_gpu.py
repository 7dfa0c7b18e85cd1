"""The batch preparation of several learners at once on the device: the bodies of tests/test_entity_prepare.py on VecSide."""
import pytest
from sides import VecSide, need_gpu

import test_entity_prepare as body

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", body.CASES)
def test_entity_prepare(case):
    body.prepare_matches(VecSide, case)


def test_entity_prepare_null_terminal_and_inf():
    body.null_terminal_and_inf(VecSide)


def test_entity_prepare_groups_are_independent():
    body.groups_are_independent(VecSide)


def test_entity_prepare_extent():
    body.extent_is_respected(VecSide)


def test_entity_prepare_bad_arguments():
    body.bad_arguments_leave_everything_untouched(VecSide)


def test_prepare_trainer():
    """The shapes of test_joint_update_trainer: B = 64, N = 70, M = 3, batch 32, minibatch 16, two epochs."""
    need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN, synth_scenario

    def make_env():
        return VecWRSN([synth_scenario(300 + e, 70, 60) for e in range(64)], None, 3, render=False, entities=True, auto_reset=True, step_budget=1250)

    for env in body.trainer_paths_agree(make_env, dict(batch_size=32, minibatch_size=16, n_updates_per_iteration=2), 100):
        env.close()
