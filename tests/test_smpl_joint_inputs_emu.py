"""CPU tier: HumorModel.roll_out with SMPL-joint feedback through the host SIMT emulator build of the kernels, and the parts of the feature that
need no kernel (constructor, state dict, prepare_input, the fixture against the live reference)."""
import pytest
import torch

import smpl_joint_inputs_checks as SC

CPU = torch.device('cpu')


@pytest.mark.slow
def test_emu_feedback_rollout_two_rows_two_steps(emu_lib):
    """The first two sequences (male, female) and two steps of the B = 5 given-z case.  Slow tier: the two steps' prior and decoder layers take
    the emulator 65 to 75 s (all of it inside the one entry-point call), more than the default tier has room for."""
    SC.check_fixture_case(emu_lib, CPU, 'b5_given', rows=2, steps=2)


@pytest.mark.slow
@pytest.mark.parametrize('name', list(SC.CASES))
def test_emu_feedback_rollout_matches_reference(emu_lib, name):
    SC.check_fixture_case(emu_lib, CPU, name)


@pytest.mark.slow
def test_emu_feedback_is_live(emu_lib):
    SC.check_feedback_is_live(emu_lib, CPU)


@pytest.mark.slow
def test_emu_without_gender_or_betas_is_the_plain_rollout(emu_lib):
    SC.check_without_gender_is_plain(emu_lib, CPU)


@pytest.mark.slow
def test_emu_batch_permutation(emu_lib):
    SC.check_batch_permutation(emu_lib, CPU)


@pytest.mark.slow
def test_emu_smpl_batch_size_is_honoured(emu_lib):
    SC.check_smpl_batch_size(emu_lib, CPU)


@pytest.mark.slow
def test_emu_required_gradient_is_refused(emu_lib):
    SC.check_gradient_is_refused(emu_lib, CPU)


@pytest.mark.slow
def test_emu_qual_sampling_sequence_vs_reference(emu_lib):
    SC.check_qual_sampling_sequence(emu_lib, CPU)


def test_constructor_and_state_dict():
    SC.check_constructor_and_state_dict()


def test_prepare_input_structure():
    SC.check_prepare_input_structure()


def test_prepare_input_vs_reference():
    SC.check_prepare_input_vs_reference()


def test_fixture_regenerates_from_the_reference():
    SC.check_fixture_regenerates()
