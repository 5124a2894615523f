"""CPU tier (SIMT emulator) of the layout passes folded into the batched GEMM: tests/gemm_fold_checks.py on the networks of
tests/gemm_split_checks.py at one and two row tiles, and a short roll-out for the prior's mean | log-variance store."""
import pytest
import torch

import gemm_fold_checks as FC
import gemm_split_checks as GC
from humor_amd import mlp as M

CPU = torch.device('cpu')


@pytest.mark.parametrize('dims,act', GC.NETS, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_emu_gemm_fold_bitwise_equal_to_separate_passes(emu_lib, dims, act):
    """y and g_x of gemm_fold 1 and 0 bitwise equal, NaN behind the last row untouched: every (TN, KS) form, odd and even line widths
    (339: single-float stores; 126, 96: float pairs), partial last tiles (126, 339, 96), one 32-row tile."""
    FC.check_mlp_net(emu_lib, CPU, dims, act, N=32, seed=len(dims) + dims[0])


# the row-major A operand's own guards: in_dim no multiple of 4 (19: c < in_dim inside a quad, in_dim != in_pad), of 32 (48: the upper half-wave
# ends early), exactly one slice (64: leaves the full-slice path for the guarded loader), and behind a GroupNorm epilogue (TN 2)
A_NETS = [((19, 512, 126), 'leaky_relu'), ((64, 96), 'leaky_relu'), ((48, 512, 32), 'gn_relu')]


@pytest.mark.parametrize('dims,act', A_NETS, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_emu_gemm_fold_row_major_a_operand(emu_lib, dims, act):
    FC.check_mlp_net(emu_lib, CPU, dims, act, N=33, seed=20 + dims[0])


def test_emu_gemm_fold_ragged_rows(emu_lib):
    # two row tiles, the second with one live row / a single sequence: the row guard of the row-major store and of the row-major A operand
    FC.check_mlp_net(emu_lib, CPU, (32, 512, 126), 'leaky_relu', N=33, seed=7)
    FC.check_mlp_net(emu_lib, CPU, (512, 512, 48), 'gn_relu', N=33, seed=8)
    FC.check_mlp_net(emu_lib, CPU, (126, 96), 'leaky_relu', N=1, seed=9)
    FC.check_mlp_net(emu_lib, CPU, (339, 96, 339), 'leaky_relu', N=45, seed=10)


def test_emu_gemm_fold_keeps_the_rotation_tail(emu_lib):
    # the 6-D -> axis-angle tail stays a kernel of its own behind the last layer (its groups of six straddle the 32-column tiles)
    FC.check_mlp_net(emu_lib, CPU, (32, 512, 126), 'leaky_relu', N=33, seed=11, tail=M.TAIL_ROT6D_AA)


def test_emu_gemm_fold_prior_outputs_and_gradients(emu_lib):
    """The prior-shaped case (96 outputs, S = 2 steps, B = 3 sequences of one partial row tile): world, prior_mu, prior_var and the gradients
    (the adjoint reads the stash the folded forward left) bitwise equal to the prior_io_kernel path, nothing stored beyond sequence B."""
    FC.check_prior(emu_lib, CPU, B=3, S=2, seed=2, want_grads=True)
