"""The node-pointer entity policy on the device: the bodies of tests/test_entity_pointer.py on VecSide / VecWRSN."""
import pytest
from sides import VecSide

import test_entity_pointer as body

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,M", body.SHAPES)
@pytest.mark.parametrize("sampled", [True, False])
def test_pointer_scores_and_choice(N, M, sampled):
    body.scores_and_choice_match(VecSide, N, M, sampled)


def test_pointer_ties():
    body.ties_go_to_the_lower_index(VecSide)


def test_pointer_masks():
    body.masks_are_selects(VecSide)


def test_pointer_independence():
    body.rows_are_independent(VecSide)


def test_pointer_bad_arguments():
    body.bad_arguments_leave_everything_untouched(VecSide)


def _train_env(B=3, M=2):
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, VecWRSN, synth_scenario
    return VecWRSN([synth_scenario(300 + e, 70, 60) for e in range(B)], DEFAULT_MC_SPEC, M, map_size=12, render=False, entities=True, auto_reset=True)


def test_device_action_is_the_stored_decisions_action():
    body.device_action_is_the_stored_decisions_action(_train_env, None)


def test_fused_roll_out_stores_what_evaluate_recomputes():
    body.fused_roll_out_stores_what_evaluate_recomputes(_train_env, None)


@pytest.mark.parametrize("fused", [False, True])
def test_pointer_trainer_trains(fused):
    body.trainer_trains(_train_env, None, fused)


def _eval_env():
    from multi_agent_rl_wrsn_amd import DEFAULT_MC_SPEC, VecWRSN
    from test_evaluate import scenarios
    return VecWRSN(scenarios(8), DEFAULT_MC_SPEC, 3, map_size=12, render=False, entities=True, auto_reset=False)


def test_pointer_cannot_stand_still():
    body.cannot_stand_still(_eval_env)
