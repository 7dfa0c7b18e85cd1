"""The candidate mask of the node-pointer policy on the device: the bodies of tests/test_entity_pointer_mask.py on VecSide / VecWRSN."""
import pytest
from sides import VecSide

import test_entity_pointer_mask as body
from test_entity_pointer_gpu import _eval_env, _train_env

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,M", body.SHAPES)
def test_mask_bits(N, M):
    body.mask_bits_match(VecSide, N, M)


@pytest.mark.parametrize("N,M", body.SHAPES)
@pytest.mark.parametrize("sampled", [True, False])
def test_masked_scores_and_choice(N, M, sampled):
    body.masked_scores_and_choice_match(VecSide, N, M, sampled)


def test_zero_query():
    body.zero_query_picks_the_first_candidate(VecSide)


def test_edges():
    body.edges_hold(VecSide)


def test_claims_across_tiles():
    body.claims_across_tiles_keep_ties(VecSide)


def test_no_op_masks():
    body.no_op_masks_give_mode_0_bytes(VecSide)


def test_masked_independence():
    body.masked_rows_are_independent(VecSide)


def test_masked_eval():
    body.masked_eval_reproduces_act(VecSide)


@pytest.mark.parametrize("hi", range(len(body.U.HYPERS)))
@pytest.mark.parametrize("shape", list(body.MASK_GRAD_CASES))
def test_masked_ppo_grad(shape, hi):
    body.masked_gradient_matches(VecSide, shape, hi)


def test_masked_joint_calls():
    body.masked_joint_calls_match(VecSide)


@pytest.mark.parametrize("fused_policy", [False, True])
@pytest.mark.parametrize("device_update", [False, True])
def test_masked_trainer(fused_policy, device_update):
    body.masked_trainer_recomputes_what_acting_stored(_train_env, None, fused_policy, device_update)


def test_masked_trainer_joint():
    body.masked_trainer_recomputes_what_acting_stored(_train_env, None, True, True, joint=True)


def test_masked_policy_cannot_stand_still():
    body.masked_policy_cannot_stand_still(_eval_env)
