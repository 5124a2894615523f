"""GPU tier (-m gpu): HumorModel.roll_out with SMPL-joint feedback (model_use_smpl_joint_inputs + smplh_path, the HuMoR-Qual configuration) on a
real MI355X, against reference-generated vectors (tests/golden/rollout_smpl_joints.npz)."""
import pytest
import torch

import smpl_joint_inputs_checks as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', list(SC.CASES))
def test_feedback_rollout_matches_reference(gpu_lib, dev, name):
    """Given z / prior mean / sampled at B = 5 (three genders), B = 33 (second row tile), B = 1 canonicalised: every output, every step, 1e-4."""
    SC.check_fixture_case(gpu_lib, dev, name)


def test_feedback_is_live(gpu_lib, dev):
    SC.check_feedback_is_live(gpu_lib, dev)


def test_without_gender_or_betas_is_the_plain_rollout(gpu_lib, dev):
    SC.check_without_gender_is_plain(gpu_lib, dev)


def test_batch_permutation(gpu_lib, dev):
    SC.check_batch_permutation(gpu_lib, dev)


def test_smpl_batch_size_is_honoured(gpu_lib, dev):
    SC.check_smpl_batch_size(gpu_lib, dev)


def test_required_gradient_is_refused(gpu_lib, dev):
    SC.check_gradient_is_refused(gpu_lib, dev)


def test_qual_sampling_sequence_vs_reference(gpu_lib, dev):
    SC.check_qual_sampling_sequence(gpu_lib, dev)
