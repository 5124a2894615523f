"""GPU tier of the layout passes folded into the batched GEMM (tests/gemm_fold_checks.py) at the closure's real row counts."""
import pytest
import torch

import gemm_fold_checks as FC
import gemm_split_checks as GC
from humor_amd import mlp as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('N', [32, 45, 1888])
def test_gemm_fold_bitwise_equal_to_separate_passes(gpu_lib, dev, N):
    """y and g_x of gemm_fold 1 and 0 bitwise equal on every network of gemm_split_checks.NETS, NaN behind the last row untouched
    (45: a second row tile with 13 live rows)."""
    for dims, act in GC.NETS:
        FC.check_mlp_net(gpu_lib, dev, dims, act, N, seed=len(dims) + dims[0])
    # the row-major A operand's guards (in_dim no multiple of 4 / of 32, exactly one slice, behind a GroupNorm epilogue)
    for dims, act in (((19, 512, 126), 'leaky_relu'), ((64, 96), 'leaky_relu'), ((48, 512, 32), 'gn_relu')):
        FC.check_mlp_net(gpu_lib, dev, dims, act, N, seed=20 + dims[0])


def test_gemm_fold_keeps_the_rotation_tail(gpu_lib, dev):
    FC.check_mlp_net(gpu_lib, dev, (32, 512, 126), 'leaky_relu', N=32, seed=11, tail=M.TAIL_ROT6D_AA)
    FC.check_mlp_net(gpu_lib, dev, (32, 512, 126), 'leaky_relu', N=33, seed=12, tail=M.TAIL_ROT6D_AA)


@pytest.mark.parametrize('B,S', [(5, 4), (31, 59), (40, 3), (70, 5)])
def test_gemm_fold_prior_outputs_and_gradients(gpu_lib, dev, B, S):
    """The prior-shaped case (96 outputs, S > 1, B not a multiple of 32) behind the persistent (B <= 32) and the pipelined roll-out: world,
    prior_mu, prior_var and the gradients bitwise equal to the prior_io_kernel path; nothing stored beyond sequence B."""
    FC.check_prior(gpu_lib, dev, B, S, seed=B + S)


def test_gemm_fold_prior_outputs_launch_chain(gpu_lib, dev):
    gpu_lib.call('ha_tune_set', b'rollout_persist', 0)
    try:
        FC.check_prior(gpu_lib, dev, 7, 3, seed=4)
    finally:
        gpu_lib.call('ha_tune_set', b'rollout_persist', 1)
