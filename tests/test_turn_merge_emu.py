"""CPU tier: the turn-around riders (ha_tune_set "turn_merge") on the SIMT-emulator build -- the block roles of ha_fit_pre_backward,
ha_rollout_post_backward and ha_fit_pre_forward against the same work as launches of their own, bit for bit, and against references.  The
emulator has no persistent roll-out kernels: the roll-out entry points refuse every rider flag there (the GPU tier runs them)."""
import pytest
import torch

import turn_merge_checks as TM

CPU = torch.device('cpu')


# The roles need no more rows than blocks: one sequence and S = 2, the partial team of three sequences with the addend.  (B = 32, a full set of
# teams, and S = 8: GPU tier.)
@pytest.mark.parametrize('B,S,add', [(1, 2, False), (3, 2, True)])
def test_emu_dz_reduction_rides_in_fit_pre_backward(emu_lib, B, S, add):
    TM.check_dz_in_fit_pre(emu_lib, CPU, B, S, add, seed=B)


# 2 x 2 without the row-sum task (the riders' blocks follow the reduction's directly), 3 x 2 with it; a padded slab (104 channels) and an
# exchange region of two full clearing blocks and a part of a third
@pytest.mark.parametrize('B,S,with_sum', [(2, 2, False), (3, 2, True)])
def test_emu_post_launch_with_layout_and_clear(emu_lib, B, S, with_sum):
    TM.check_post_merged(emu_lib, CPU, B, S, with_sum, seed=S + B)


def test_emu_forward_clear_rides_in_fit_pre_forward(emu_lib):
    TM.check_fwd_clear(emu_lib, CPU, 1)


def test_emu_malformed_tasks_are_refused(emu_lib):
    TM.check_task_argument_refusals(emu_lib, CPU)


def test_emu_rider_flags_are_refused_on_the_launch_chain(emu_lib):
    _, h = TM.make_net(emu_lib, CPU)
    TM.check_flag_refusals(emu_lib, CPU, h, persistent=False, B=1, S=1)      # (one step: the emulator pays for the forward that fills the stash)
