"""GPU tier (-m gpu): gradients through the SMPL-joint feedback roll-out (HumorModel(..., smpl_joint_gradients=True), glue_bwd_fb_kernel) and
MotionOptimizer fitting with such a prior on a real MI355X, against the reference's autograd (tests/golden/rollout_smpl_joints_grad.npz)."""
import pytest
import torch

import smpl_joint_grad_checks as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', GC.CASES)
def test_feedback_gradients_match_reference(gpu_lib, dev, name):
    """B = 2 / 5 (three genders, two feedback links) / 5 without prior cotangents / 33 (second row tile) / 1 canonicalised: every forward output
    to 1e-4, dL/d(initial state), dL/dz and dL/dbetas to 1e-3 of the reference's largest entry."""
    GC.check_fixture_case(gpu_lib, dev, name)


def test_rest_gradient_reaches_betas(gpu_lib, dev):
    GC.check_rest_gradient_reaches_betas(gpu_lib, dev)


def test_backward_twice_is_bit_identical(gpu_lib, dev):
    GC.check_backward_twice_bit_identical(gpu_lib, dev)


def test_batch_permutation(gpu_lib, dev):
    GC.check_batch_permutation(gpu_lib, dev)


def test_without_gender_or_betas_is_the_plain_rollout(gpu_lib, dev):
    GC.check_without_gender_is_plain(gpu_lib, dev)


def test_keyword_default_refuses(gpu_lib, dev):
    GC.check_keyword_default_refuses(gpu_lib, dev)


def test_stash_mixup_is_refused(gpu_lib, dev):
    GC.check_stash_mixup_is_refused(gpu_lib, dev)


def test_rollout_latent_motion_passes_gender_and_betas(gpu_lib, dev, smplh_npz):
    GC.check_rollout_latent_motion_passes_gender_and_betas(gpu_lib, dev, smplh_npz)


def test_stage3_nodes_equal_separate_functions_with_feedback_prior(gpu_lib, dev, smplh_npz):
    GC.check_stage3_nodes_equal_separate_functions(gpu_lib, dev, smplh_npz)


def test_stage3_iterations_with_feedback_prior(gpu_lib, dev, smplh_npz):
    GC.check_stage3_iterations(gpu_lib, dev, smplh_npz)


def test_fit_refusals(gpu_lib, dev, smplh_npz):
    GC.check_fit_refusals(gpu_lib, dev, smplh_npz)
