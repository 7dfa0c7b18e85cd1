"""Imitation pretraining of the node-pointer policy on the device: the bodies of tests/test_entity_pointer_bc.py on VecSide / VecWRSN."""
import pytest
from sides import VecSide

import test_entity_pointer_bc as body
from test_entity_pointer_gpu import _eval_env, _train_env

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,M", body.B.SHAPES)
def test_label(N, M):
    body.label_matches(VecSide, N, M)


def test_label_edges():
    body.label_edges(VecSide)


def test_label_bad_arguments():
    body.label_bad_arguments(VecSide)


def test_label_rows_are_independent():
    body.label_rows_are_independent(VecSide)


@pytest.mark.parametrize("N,M", body.B.SHAPES)
def test_label_is_a_candidate(N, M):
    body.label_is_a_candidate(VecSide, N, M)


@pytest.mark.parametrize("ent_coef", body.B.ENT_COEFS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", body.B.GRAD_SHAPES)
def test_bc_grad(shape, masked, ent_coef):
    body.bc_gradient_matches(VecSide, shape, masked, ent_coef)


@pytest.mark.parametrize("n,N,M,masked", body.PPO_CASES)
def test_bc_grad_is_the_ppo_gradient(n, N, M, masked):
    body.bc_grad_is_the_ppo_gradient(VecSide, n, N, M, masked)


@pytest.mark.parametrize("G,n,n_all,N,M", body.MULTI_CASES)
def test_bc_grad_multi(G, n, n_all, N, M):
    body.bc_multi_matches_single(VecSide, G, n, n_all, N, M)


@pytest.mark.parametrize("masked", [False, True])
def test_bc_update(masked):
    body.bc_update_matches(VecSide, masked)


def test_bc_update_learns():
    body.bc_update_learns(VecSide)


def test_bc_bad_arguments():
    body.bc_bad_arguments(VecSide)


@pytest.mark.parametrize("beta,beta_end", [(1.0, None), (0.5, 0.0)])
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("mask_claimed", [False, True])
@pytest.mark.parametrize("fused_policy", [False, True])
def test_pretrain(fused_policy, mask_claimed, joint, beta, beta_end):
    body.pretrain_clones_the_heuristic(_train_env, None, fused_policy, mask_claimed, joint, beta, beta_end)


def test_pretrain_options():
    body.pretrain_options(_train_env, None)


def test_label_policy_cannot_stand_still():
    body.label_policy_cannot_stand_still(_eval_env)
