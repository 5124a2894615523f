"""CPU tier: the state-prior kernels (humor_amd/csrc/gmm_fit.hip) built for the host SIMT emulator, through humor_amd/state_prior.py,
against the fp64 yardstick of state_prior_checks.py."""
import numpy as np
import pytest
import torch

import state_prior_checks as SC
from humor_amd import _lib, state_prior as SP

CPU = torch.device('cpu')


@pytest.mark.parametrize('shape', SC.STEP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_one_e_step_and_one_m_step(emu_lib, shape):
    SC.check_steps(emu_lib, CPU, *shape)


def test_row_stride(emu_lib):
    """the states as a column slice of a wider table whose other columns hold NaN"""
    SC.check_steps(emu_lib, CPU, 65, 137, 2, strided=True)


def test_dense_precision_factor(emu_lib):
    """precisions_init gives a LOWER triangular factor (chol(precision)), which takes the E step's full contraction"""
    c = SC.step_case(70, 138, 12)
    prec = c['P'] @ c['P'].transpose(1, 2)
    Pl = torch.linalg.cholesky(prec)
    x = c['x'].to(torch.float32)
    eng = SP._Engine(x, 12, emu_lib)
    eng.estep(c['weights'], c['means'].to(torch.float32), Pl)
    ll, _ = SC.e_step(x.double(), c['weights'], c['means'], Pl)
    SC.check_scalar('loglik, lower triangular factor', eng.loglik, ll)


def test_six_iterations_small_case(emu_lib):
    case = SC.small_case()
    got = SP.fit_gmm(torch.as_tensor(case['x'], dtype=torch.float32), n_components=case['K'], tol=0.0, max_iter=6,
                     weights_init=case['weights_init'], means_init=case['means_init'], precisions_init=case['precisions_init'],
                     _lib_override=emu_lib)
    SC.check_fit('small case', got, SC.small_reference(6))


def test_two_runs_bit_identical(emu_lib):
    case = SC.small_case()
    run = lambda: SP.fit_gmm(torch.as_tensor(case['x'], dtype=torch.float32), n_components=case['K'], tol=0.0, max_iter=3,
                             weights_init=case['weights_init'], means_init=case['means_init'], precisions_init=case['precisions_init'],
                             _lib_override=emu_lib)
    a, b = run(), run()
    assert a.lower_bounds == b.lower_bounds
    for k in ('weights', 'means', 'covariances'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_score_samples_matches_gmm_nll(emu_lib):
    """the fitting path's ha_gmm_nll and the E step must describe the same density (3 rows, D = 138, K = 12)"""
    from humor_amd.fit_kernels import GmmNll
    from humor_amd.fitting_loss import _GMM
    c = SC.step_case(70, 138, 12)
    cov = torch.linalg.inv(c['P'] @ c['P'].transpose(1, 2))
    cov = 0.5 * (cov + cov.transpose(1, 2))
    x = c['x'][:3].to(torch.float32)
    ll = SP.score_samples(x, (c['weights'], c['means'], cov), _lib_override=emu_lib)
    gmm = _GMM(c['weights'].float(), c['means'].float(), cov.float())
    nll = torch.stack([GmmNll.apply(emu_lib, gmm, x[i:i + 1]) for i in range(3)])
    SC.check_scalar('score_samples against -ha_gmm_nll', ll, -nll)
    ref, _ = SC.e_step(x.double(), c['weights'], c['means'], c['P'])
    SC.check_scalar('score_samples against the yardstick', ll, ref)
    SC.check_scalar('score', SP.score(x, (c['weights'], c['means'], cov), _lib_override=emu_lib), float(ref.mean()))


def test_nan_row_raises(emu_lib):
    case = SC.small_case()
    x = torch.as_tensor(case['x'], dtype=torch.float32).clone()
    x[77, 2] = float('nan')
    with pytest.raises(ValueError, match='lower bound'):
        SP.fit_gmm(x, n_components=case['K'], max_iter=3, weights_init=case['weights_init'], means_init=case['means_init'],
                   precisions_init=case['precisions_init'], _lib_override=emu_lib)


def test_empty_component_keeps_reg_covar(emu_lib):
    """labels that leave component 2 without a row: its covariance is reg_covar I (and its mean 0), as in scikit-learn, and the fit goes on"""
    case = SC.small_case()
    x = torch.as_tensor(case['x'], dtype=torch.float32) + 3.0      # (away from the origin: the empty component sits at 0 and stays empty)
    labels = (torch.arange(x.shape[0]) % 2).numpy()
    got = SP.fit_gmm(x, n_components=3, tol=0.0, max_iter=2, labels_init=labels, _lib_override=emu_lib)
    ref = SC.fit(x.double(), 3, tol=0.0, max_iter=2, labels_init=labels)
    assert got.n_iter == 2
    assert torch.equal(got.covariances[2], 1e-6 * torch.eye(5, dtype=torch.float64)) and torch.equal(ref['covariances'][2], got.covariances[2])
    assert float(got.means[2].abs().max()) == 0.0
    SC.check_fit('empty component', got, ref)


def test_host_tensors_need_the_emulator_library():
    class NotEmu:
        emulator = False
    with pytest.raises(_lib.HumorAmdError, match='GPU only'):
        SP.fit_gmm(torch.zeros(8, 3), n_components=1, _lib_override=NotEmu())


def test_save_load_round_trip(tmp_path):
    w = np.array([0.25, 0.75])
    mu = np.arange(6.0).reshape(2, 3)
    cov = np.stack([np.eye(3), 2.0 * np.eye(3)])
    path = SP.save_gmm(str(tmp_path), (w, mu, cov))
    assert path.endswith('prior_gmm.npz') and sorted(np.load(path).files) == ['covariances', 'means', 'weights']
    back = SP.load_gmm(str(tmp_path))
    assert np.array_equal(back['weights'], w) and np.array_equal(back['means'], mu) and np.array_equal(back['covariances'], cov)
    prior = SP.as_init_motion_prior(back, CPU)
    assert set(prior) == {'gmm'} and [t.dtype for t in prior['gmm']] == [torch.float32] * 3 and prior['gmm'][2].shape == (2, 3, 3)
