"""CPU tier: the points3d op (csrc/points_fit.hip) on the host SIMT emulator build of the kernels -- the cases of the GPU tier except
the V = 6890 ones -- and the dispatch of FittingLoss.points3d_loss."""
import pytest
import torch

import points_fit_checks as PC

CPU = torch.device('cpu')


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (3, 5, 257, 1030), (2, 2, 64, 1), (1, 2, 130, 3), (1, 1, 2600, 5)])
def test_emu_op_matches_yardstick(emu_lib, shape):
    """N = 1; N odd with V across the 1024-candidate LDS chunk and a ragged tail; up to 64 lanes of one wave on the same vertex
    (ordered in-wave accumulation over multiplicities 1 .. 64 and over wave steps); more observations per frame than five staged groups of
    the backward (512 each) with a ragged sixth, and N past one four-key trip of the select passes (2048) with a ragged tail."""
    PC.check_case(emu_lib, CPU, *PC.make_case(*shape, seed=sum(shape)))


def test_emu_ties_and_zero_distance(emu_lib):
    PC.check_zero_distance_gradient(emu_lib, CPU)


def test_emu_mad_zero(emu_lib):
    PC.check_mad_zero(emu_lib, CPU)


def test_emu_narrow_range(emu_lib):
    PC.check_narrow_range(emu_lib, CPU)


def test_emu_nan_sequence(emu_lib):
    PC.check_nan_sequence(emu_lib, CPU)


def test_emu_no_robust_weights(emu_lib):
    PC.check_none(emu_lib, CPU)


def test_emu_determinism(emu_lib):
    PC.check_determinism(emu_lib, CPU, (2, 3, 70, 130))


def test_emu_fallbacks(emu_lib, monkeypatch):
    PC.check_fallbacks(emu_lib, CPU, monkeypatch)


def test_emu_points_only_objective_skips_the_fused_kernel(emu_lib, monkeypatch):
    """root_fit with points3d as the only weighted term: the op alone, no launch of the fused loss kernel on an all-zero weight vector; with
    a second weighted term the fused kernel evaluates it and the points term is an addend (equal to the term-by-term evaluation)."""
    from humor_amd import fit_kernels as FK
    obs, pred = PC.make_case(2, 3, 70, 130, seed=9)
    g = torch.Generator().manual_seed(9)
    jtr = torch.randn(2, 3, 22, 3, generator=g)
    obs_d = {'points3d': obs, 'joints3d': torch.randn(2, 3, 22, 3, generator=g)}
    res = {}
    for weights in ({'points3d': 0.7}, {'points3d': 0.7, 'joints3d': 1.3}):
        for fp in (True, False):
            fl = PC._fitting_loss(emu_lib, 'bisquare', fp, weights)
            p, j = pred.clone().requires_grad_(True), jtr.clone().requires_grad_(True)
            if fp and len(weights) == 1:
                with monkeypatch.context() as m:
                    m.setattr(FK.FusedFit, 'apply', lambda *a, **k: pytest.fail('FusedFit launched for a points3d-only objective'))
                    loss, stats = fl.root_fit(obs_d, {'joints3d': j, 'points3d': p})
            else:
                loss, stats = fl.root_fit(obs_d, {'joints3d': j, 'points3d': p})
            assert set(stats) == set(weights)
            res[(len(weights), fp)] = (loss.item(), torch.autograd.grad(loss, p)[0])
    for n in (1, 2):
        (l1, g1), (l0, g0) = res[(n, True)], res[(n, False)]
        assert abs(l1 - l0) <= 1e-5 * abs(l0), (n, l1, l0)
        assert float((g1 - g0).abs().max()) <= 1e-4 * float(g0.abs().max()), n


def test_no_cpu_fallback():
    """The product op refuses CPU tensors instead of computing somewhere else."""
    from humor_amd._lib import HumorAmdError
    from humor_amd.points_fit import robust_points_loss
    with pytest.raises(HumorAmdError):
        robust_points_loss(torch.zeros(1, 1, 4, 3), torch.zeros(1, 1, 5, 3))
