"""`evaluate_policy`, the policies and the trainer's episode log on the device: the bodies of tests/test_evaluate.py on VecWRSN."""
import pytest
from sides import need_gpu

import test_evaluate as body

pytestmark = pytest.mark.gpu


def gpu_env(B=8, max_time=body.MAX_TIME, auto_reset=False, **kw):
    need_gpu()
    from multi_agent_rl_wrsn_amd import VecWRSN
    kw.setdefault("entities", True)
    return VecWRSN(body.scenarios(B, max_time=max_time), None, 3, map_size=12, render=not kw["entities"], auto_reset=auto_reset, **kw)


@pytest.mark.parametrize("which", ["uniform", "sampled"])
def test_evaluation_is_deterministic_and_matches_the_reference(which):
    for env in body.evaluation_is_deterministic_and_matches_the_reference(gpu_env, which):
        env.close()


@pytest.mark.parametrize("which,cap", [("heuristic", 48), ("mode", 24)])
def test_named_policies_are_deterministic_and_match_the_reference(which, cap):
    for env in body.named_policies_are_deterministic_and_match_the_reference(gpu_env, which, cap):
        env.close()


def test_pooled_evaluation():
    body.pooled_evaluation(gpu_env).close()


def test_policies_and_errors():
    made = []

    def wrong():
        made.extend([gpu_env(2, auto_reset=True), gpu_env(2, entities=False)])
        return made

    made.append(body.policies_and_errors(gpu_env, wrong))
    for env in made:
        env.close()


def test_trainer_logs_episodes():
    """The shapes of the emulator's test: B = 16, N = 33, M = 3, batch 32, minibatch 16, two epochs."""
    env = body.trainer_logs_episodes(lambda: gpu_env(16, max_time=1e9, auto_reset=True), dict(batch_size=32, minibatch_size=16, n_updates_per_iteration=2), 200)
    env.close()
