"""CPU tier: the fp64 restatement of scikit-learn's EM that the state-prior kernels are measured against (state_prior_checks.py) is pinned
to scikit-learn itself where it is installed, and to a golden file of scikit-learn's outputs everywhere."""
import warnings

import numpy as np
import pytest
import torch

import state_prior_checks as SC

PIN = 1e-12


def _pin(name, got, ref):
    err = float(np.abs(np.asarray(got) - np.asarray(ref)).max())
    print(f'{name}: largest distance {err:.3e}')
    assert err <= PIN, f'{name}: {err:.3e} > {PIN:.0e}'


@pytest.mark.parametrize('which', ['small', 'large'])
def test_yardstick_equals_sklearn(which):
    mixture = pytest.importorskip('sklearn.mixture')
    case = SC.small_case() if which == 'small' else SC.large_case()
    iters = 6 if which == 'small' else 8
    start = {k: case[k] for k in ('weights_init', 'means_init', 'precisions_init')}
    gm = mixture.GaussianMixture(n_components=case['K'], covariance_type='full', tol=0.0, reg_covar=1e-6, max_iter=iters, **start)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                       # (tol = 0: it never reports convergence)
        gm.fit(case['x'])
    ours = SC.fit(case['x'], case['K'], tol=0.0, max_iter=iters, **start)
    assert ours['n_iter'] == gm.n_iter_ == iters
    _pin('weights', ours['weights'], gm.weights_)
    _pin('means', ours['means'], gm.means_)
    _pin('covariances', ours['covariances'], gm.covariances_)
    _pin('lower bounds', ours['lower_bounds'], gm.lower_bounds_)


def test_yardstick_equals_golden_sklearn_outputs():
    g = SC.small_golden()
    ref = SC.small_reference(int(g['iters']))
    _pin('weights', ref['weights'], g['weights'])
    _pin('means', ref['means'], g['means'])
    _pin('covariances', ref['covariances'], g['covariances'])
    _pin('lower bounds', ref['lower_bounds'], g['lower_bounds'])
    P = SC.precision_cholesky(ref['covariances'])
    ll, resp = SC.e_step(torch.as_tensor(g['x']), ref['weights'], ref['means'], P)
    _pin('score_samples', ll, g['score_samples'])
    _pin('responsibilities', resp, g['resp'])


def test_small_case_is_soft():
    """a hard-assigned input would let a kernel that mishandles fractional responsibilities pass: at least 20 % of the rows end with a
    largest responsibility below 0.9"""
    share = SC.soft_share(SC.small_reference()['last_resp'])
    print(f'rows with a largest responsibility below 0.9: {100 * share:.1f} %')
    assert share >= 0.20
