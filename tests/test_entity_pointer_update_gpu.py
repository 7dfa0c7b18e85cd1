"""The PPO gradient of the node-pointer policy and the trainer's device_update option on the device: the bodies of
tests/test_entity_pointer_update.py on VecSide and on the environments of tests/test_entity_pointer_gpu.py.  (The default path,
device_update=False, is compared with PPOLearner.update on the CPU only: PyTorch's backward on the device is not bit-reproducible from
run to run, so two PyTorch updates under equal seeds differ there whatever this option does.)"""
import pytest
from sides import VecSide, need_gpu

import test_entity_pointer_update as body
from test_entity_pointer_gpu import _train_env

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", list(body.GRAD_CASES))
def test_pointer_eval(shape):
    body.eval_matches(VecSide, shape)


def test_pointer_eval_reproduces_act():
    body.eval_reproduces_act(VecSide)


@pytest.mark.parametrize("hi", range(len(body.HYPERS)))
@pytest.mark.parametrize("shape", list(body.GRAD_CASES))
def test_pointer_ppo_grad(shape, hi):
    body.gradient_matches(VecSide, shape, hi)


def test_pointer_update_bad_arguments():
    body.bad_arguments_leave_everything_untouched(VecSide)


def test_pointer_adam():
    body.adam_matches(VecSide)


def test_pointer_trainer_updates_on_the_device(tmp_path):
    need_gpu()
    body.trainer_updates_on_the_device(_train_env, None, tmp_path)
