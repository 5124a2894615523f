"""GPU tier of the batched GEMM's short-chain forms at the closure's real row counts (32 sequences; 32 x 59 = 1888 prior rows)."""
import pytest
import torch

import gemm_split_checks as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu_lib():
    from humor_amd import _lib
    return _lib.get_lib()


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('N', [32, 1888])
def test_gemm_split_forms_against_fp64(gpu_lib, dev, N):
    """Error against fp64 at most twice the plain form's, two runs bitwise equal, and every launch the policy must leave alone (fewer than
    four K slices, or more than 512 plain-form waves) bitwise equal to gemm_ks 0."""
    GC.check_all(gpu_lib, dev, N)


def test_gemm_policy_pins_the_square_products(gpu_lib, dev):
    """1888 x 1024 x 1024 with the GroupNorm epilogues (the prior's hidden layers) and 1888 x 339 -> 1024, 1888 x 1024 <- 96 (944 plain-form
    waves each): gemm_ks 2 must take the instantiation and grid of gemm_ks 0 -- outputs and gradients bit for bit."""
    dims = (339, 1024, 1024, 1024, 96)
    lin, gns = GC.make_net(dims, 'gn_relu', 3)
    from humor_amd import mlp as M
    f = M.FusedMLP(gpu_lib, 0, lin, act='gn_relu', gns=gns)
    g = torch.Generator().manual_seed(4)
    x, w = torch.randn(1888, dims[0], generator=g), torch.randn(1888, dims[-1], generator=g)
    y0, gx0 = GC.run(gpu_lib, dev, f, x, w, 0)
    y2, gx2 = GC.run(gpu_lib, dev, f, x, w, 2)
    # forward: 339 -> 1024 -> 1024 -> 1024 are pinned; the last layer (1024 -> 96, 236 plain-form waves) is split, so compare what is pinned:
    # the adjoint of the pinned layers sees a split first adjoint launch only through 96 -> 1024, which is pinned itself (K = 96)
    f3 = M.FusedMLP(gpu_lib, 0, lin[:3], act='gn_relu', gns=gns[:2])
    w3 = torch.randn(1888, 1024, generator=g)
    a0, ga0 = GC.run(gpu_lib, dev, f3, x, w3, 0)
    a2, ga2 = GC.run(gpu_lib, dev, f3, x, w3, 2)
    assert torch.equal(a0, a2), 'a pinned forward launch changed bits'
    # its adjoint ends in 1024 -> 339 (472 plain-form waves): split by design, so the input gradient may differ in the last bits -- the
    # pinned part of the adjoint is checked through a network whose first layer is square
    lin_sq, gns_sq = GC.make_net((1024, 1024, 1024), 'gn_relu', 6)
    fs = M.FusedMLP(gpu_lib, 0, lin_sq, act='gn_relu', gns=gns_sq)
    xs = torch.randn(1888, 1024, generator=g)
    s0, gs0 = GC.run(gpu_lib, dev, fs, xs, w3, 0)
    s2, gs2 = GC.run(gpu_lib, dev, fs, xs, w3, 2)
    assert torch.equal(s0, s2) and torch.equal(gs0, gs2), 'a pinned square product changed bits'
    assert torch.isfinite(y2).all() and torch.isfinite(gx2).all() and (y0 - y2).abs().max().item() <= 1e-4 * max(1.0, y0.abs().max().item())
