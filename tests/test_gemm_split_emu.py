"""CPU tier (SIMT emulator) of the batched GEMM's short-chain forms: tests/gemm_split_checks.py at one and two row tiles."""
import pytest
import torch

import gemm_split_checks as GC

CPU = torch.device('cpu')


@pytest.mark.parametrize('dims,act', GC.NETS, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_emu_gemm_split_forms_against_fp64(emu_lib, dims, act):
    """Every (TN, KS) form behind every epilogue it serves: error against fp64 at most twice the plain form's, two runs bitwise equal,
    launches the policy leaves unsplit bitwise equal to the plain form (gemm_ks 0)."""
    GC.check_net(emu_lib, CPU, dims, act, N=32, seed=len(dims) + dims[0])


def test_emu_gemm_split_ragged_rows(emu_lib):
    # two row tiles, the second with one live row: the idle waves of a split block and the row guards of the epilogue
    GC.check_net(emu_lib, CPU, (32, 512, 126), 'leaky_relu', N=33, seed=7)
    GC.check_net(emu_lib, CPU, (512, 512, 48), 'gn_relu', N=33, seed=8)


def test_emu_gemm_split_forced_everywhere(emu_lib):
    """gemm_ks 3 (force the deepest split, TN = 1 where the epilogue allows) on a network whose launches all split: same bar against fp64."""
    lin, gns = GC.make_net((339, 512, 339), 'leaky_relu', 5)
    from humor_amd import mlp as M
    f = M.FusedMLP(emu_lib, 0, lin, act='leaky_relu', slope=GC.SLOPE)
    g = torch.Generator().manual_seed(9)
    x, w = torch.randn(40, 339, generator=g), torch.randn(40, 339, generator=g)
    y_ref, gx_ref = GC.reference(lin, gns, x, w)
    y0, gx0 = GC.run(emu_lib, CPU, f, x, w, 0)
    y3, gx3 = GC.run(emu_lib, CPU, f, x, w, 3)
    err = lambda a, r: (a.double() - r).abs().max().item()
    print('forced split: y', err(y0, y_ref), err(y3, y_ref), 'gx', err(gx0, gx_ref), err(gx3, gx_ref))
    assert err(y3, y_ref) <= 2.0 * err(y0, y_ref) and err(gx3, gx_ref) <= 2.0 * err(gx0, gx_ref)
