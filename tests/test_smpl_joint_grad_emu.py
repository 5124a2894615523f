"""CPU tier: gradients through the SMPL-joint feedback roll-out on the host SIMT emulator build of the kernels (slow tier; kernel runs use the
B = 2, S = 2 case only), and the parts that need no kernel (the fixture's own figures, its live regeneration from the reference)."""
import pytest
import torch

import smpl_joint_grad_checks as GC

CPU = torch.device('cpu')


@pytest.mark.slow
def test_emu_feedback_gradients_match_reference(emu_lib):
    """About 40 s on the emulator (two steps forward and backward at one row tile)."""
    GC.check_fixture_case(emu_lib, CPU, 'g_b2')


@pytest.mark.slow
def test_emu_stash_mixup_is_refused(emu_lib):
    GC.check_stash_mixup_is_refused(emu_lib, CPU)


@pytest.mark.slow
def test_emu_keyword_default_refuses(emu_lib):
    GC.check_keyword_default_refuses(emu_lib, CPU)


def test_keyword_is_off_by_default():
    from humor_amd.humor_model import HumorModel
    kw = dict(in_rot_rep='mat', out_rot_rep='aa', model_use_smpl_joint_inputs=True, smplh_path='/nonexistent/never/probed')
    assert HumorModel(**kw).smpl_joint_gradients is False and HumorModel(smpl_joint_gradients=True, **kw).smpl_joint_gradients is True


def test_fixture_carries_its_figures():
    GC.check_fixture_carries_its_figures()


def test_fixture_regenerates_from_the_reference():
    GC.check_fixture_regenerates()
