"""The node-pointer policy's update of several independent learners at once, and the trainer's joint_update and fused_prepare options, on
the device: the bodies of tests/test_entity_pointer_joint.py on VecSide."""
import pytest
from sides import VecSide, need_gpu

import test_entity_pointer_joint as body

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", body.GRAD_CASES)
def test_pointer_ppo_grad_multi(case):
    body.gradient_matches(VecSide, case)


def test_pointer_groups_are_independent():
    body.groups_are_independent(VecSide)


def test_pointer_adam_multi():
    body.adam_matches(VecSide)


def test_pointer_ppo_update():
    body.update_matches(VecSide)


def test_pointer_joint_extent():
    body.extent_is_respected(VecSide)


def test_pointer_joint_bad_arguments():
    body.bad_arguments_leave_everything_untouched(VecSide)


def _env():
    need_gpu()
    from test_entity_pointer_gpu import _train_env
    return _train_env()


def test_pointer_joint_update_trainer():
    body.trainer_paths_agree(_env, None)


def test_pointer_prepare_trainer():
    body.prepare_paths_agree(_env, None)


def test_pointer_joint_options():
    body.options_are_checked(_env, None)
