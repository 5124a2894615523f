"""GPU tier: the turn-around riders (ha_tune_set "turn_merge", default all bits) against knob 0 -- every ridden kernel a launch of its own -- bit
for bit: the block roles alone, the roll-out entry points with the riders done by their neighbours, and whole stage-3 closures eager and under
hipGraph replay.  Allocations are poisoned (conftest), so an output a role leaves unwritten shows as NaN."""
import pytest
import torch

import turn_merge_checks as TM
from humor_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def net(gpu_lib, dev):
    return TM.make_net(gpu_lib, dev)


@pytest.fixture
def persistent(gpu_lib, net):
    status = net[0].persistent_rollout_status(torch.device('cuda:0'))
    if not status[0]:
        pytest.skip('the persistent roll-out kernels are not available on this device')


# the partial team at B = 3 and a full set of teams at B = 32 are the path changes
@pytest.mark.parametrize('B', [1, 3, 32])
@pytest.mark.parametrize('S', [2, 8])
def test_dz_reduction_rides_in_fit_pre_backward(gpu_lib, dev, B, S):
    for add in (False, True):
        TM.check_dz_in_fit_pre(gpu_lib, dev, B, S, add, seed=B + S)


@pytest.mark.parametrize('B,with_sum', [(2, False), (3, True), (32, True)])
@pytest.mark.parametrize('S', [2, 8])
def test_post_launch_with_layout_and_clear(gpu_lib, dev, B, S, with_sum):
    TM.check_post_merged(gpu_lib, dev, B, S, with_sum, seed=B + S)


@pytest.mark.parametrize('B', [1, 32])
def test_forward_clear_rides_in_fit_pre_forward(gpu_lib, dev, B):
    TM.check_fwd_clear(gpu_lib, dev, B)


def test_malformed_tasks_are_refused(gpu_lib, dev):
    TM.check_task_argument_refusals(gpu_lib, dev)


def test_unbacked_rider_flags_are_refused(gpu_lib, dev, net, persistent):
    TM.check_flag_refusals(gpu_lib, dev, net[1], persistent=True)


@pytest.mark.parametrize('B,S', [(3, 2), (32, 8)])
def test_rollout_entry_points_with_every_rider(gpu_lib, dev, net, persistent, B, S):
    TM.check_entry_points_with_riders(gpu_lib, dev, net[1], B, S, seed=B)


# launches fewer than knob 0 in one eager evaluation, per knob value
SAVED = {0: 0, TM.ALL: 4, _lib.TURN_DZ: 1, _lib.TURN_POST: 2, _lib.TURN_FWD_CLEAR: 1}


@pytest.mark.parametrize('graphs', [False, True])
@pytest.mark.parametrize('B,T,knobs', [(2, 8, (0, TM.ALL, _lib.TURN_DZ, _lib.TURN_POST, _lib.TURN_FWD_CLEAR)), (32, 3, (0, TM.ALL))])
def test_stage3_closure_every_knob_value(gpu_lib, dev, smplh_npz, persistent, B, T, knobs, graphs):
    """2 x 8 and 32 x 3, eager and graph-replayed, four evaluations with every variable changed in place between them: the loss and all nine
    gradients bit for bit across the knob values, the persistent error word 0 after every evaluation, and each part takes its launches away."""
    res = {}
    with TM.knob_values(gpu_lib, knobs) as values:
        for v in values:
            res[v] = TM.run_closure(gpu_lib, dev, smplh_npz, B, T, graphs)
    for v in knobs[1:]:
        TM.assert_same_evaluations(res[v][0], res[0][0], ('turn_merge', v, 'graphs', graphs))
        if not graphs:
            print('turn_merge', v, ':', res[v][1], 'launches per evaluation against', res[0][1])
            assert res[0][1] - res[v][1] == SAVED[v], (v, res[v][1], res[0][1])


@pytest.mark.parametrize('case', ['pipelined', 'launch chain'])
def test_fall_backs_keep_their_launches(gpu_lib, dev, smplh_npz, case):
    """33 sequences (the pipelined kernels) and the launch-chain knob: no part rides -- the launch count and the results of knob 0 with the merge on."""
    B, T = (33, 3) if case == 'pipelined' else (2, 8)
    res = {}
    try:
        if case == 'launch chain':
            gpu_lib.call('ha_tune_set', b'rollout_persist', 0)
        with TM.knob_values(gpu_lib, (0, TM.ALL)) as values:
            for v in values:
                res[v] = TM.run_closure(gpu_lib, dev, smplh_npz, B, T, False, reps=2)
    finally:
        gpu_lib.call('ha_tune_set', b'rollout_persist', 1)
    assert res[TM.ALL][1] == res[0][1], (res[TM.ALL][1], res[0][1])
    TM.assert_same_evaluations(res[TM.ALL][0], res[0][0], case)
