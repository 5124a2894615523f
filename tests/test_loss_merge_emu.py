"""CPU tier: the merged loss-side launches (ha_tune_set "loss_merge") on the SIMT-emulator build -- several frames per block with wave
barriers beside the mixture's blocks, the LDS-staged reductions, the row-sum block role -- bit-equal to the one-launch-per-kernel form and
within the fit tests' tolerances of the term-by-term / op-chain references."""
import pytest
import torch

import fitloss_checks as FL
import loss_merge_checks as LM

CPU = torch.device('cpu')


# The emulator pays for every lane of every frame, so this tier takes the smallest sizes at which the merged kernels change path (the GPU tier
# runs the full table of tests/loss_merge_checks.py): one frame wave in a block of eight and K = 1 (1 x 2), two blocks of frame waves with
# idle waves in the last (3 x 5), and 260 frames = a full trip of the 256-frame loop + a remainder, both LDS buffers of the reduction
# (2 x 130).  A reduction over more than 2048 frames -- a second group of chunks -- takes it half a minute: GPU tier only.
@pytest.mark.parametrize('B,T,K', [(1, 2, 1), (3, 5, 12), (2, 130, 12)])
def test_emu_fit_loss_with_mixture_merged_equals_separate(emu_lib, B, T, K):
    print('worst relative gradient difference', LM.check_fit_loss(emu_lib, CPU, B, T, K, 'motion', seed=B + T))


def test_emu_fit_loss_without_mixture_merged_equals_separate(emu_lib):
    print('worst relative gradient difference', LM.check_fit_loss(emu_lib, CPU, 3, 5, 12, 'smpl', seed=3))


def test_emu_fit_loss_halo_and_standard_normal_prior(emu_lib):
    LM.check_fit_loss(emu_lib, CPU, 3, 5, 12, 'motion', halo=True, seed=2)
    LM.check_fit_loss(emu_lib, CPU, 3, 5, 12, 'motion', cond=False, seed=3)


# 2 x 65: more frames than lanes, two staged chunks of 64 frames
@pytest.mark.parametrize('B,T,cam', [(1, 2, True), (3, 5, False), (2, 65, True)])
def test_emu_post_reduction_with_row_sum_merged_equals_separate(emu_lib, B, T, cam):
    for add1, add2 in ((True, True), (True, False), (False, False)):
        LM.check_post_backward(emu_lib, CPU, B, T, cam, add1, add2, seed=T)
    print('op chain: worst relative gradient difference', FL.check_rollout_post(emu_lib, CPU, B=B, S=T - 1, seed=T, cam=cam))
