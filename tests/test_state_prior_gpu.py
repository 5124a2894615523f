"""GPU tier: fitting the init-state Gaussian mixture on gfx950 (humor_amd/state_prior.py, csrc/gmm_fit.hip) against the fp64 yardstick of
state_prior_checks.py (pinned to scikit-learn by test_state_prior_yardstick.py)."""
import functools

import numpy as np
import pytest
import torch

import state_prior_checks as SC
from humor_amd import state_prior as SP

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# the emulator tier's shapes, the large case's, and one at the limits of the ABI (D = 256, K = 64)
GPU_SHAPES = SC.STEP_SHAPES + [(4133, 138, 12), (300, 256, 64)]


def _large_fit(lib, **kw):
    case = SC.large_case()
    return SP.fit_gmm(torch.as_tensor(case['x'], dtype=torch.float32, device=DEV), n_components=case['K'], weights_init=case['weights_init'],
                      means_init=case['means_init'], precisions_init=case['precisions_init'], _lib_override=lib, **kw)


@functools.lru_cache(maxsize=None)
def _large_reference(tol, max_iter):
    case = SC.large_case()
    return SC.fit(case['x'], case['K'], tol=tol, max_iter=max_iter, weights_init=case['weights_init'], means_init=case['means_init'],
                  precisions_init=case['precisions_init'])


@pytest.mark.parametrize('shape', GPU_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_one_e_step_and_one_m_step(gpu_lib, shape):
    SC.check_steps(gpu_lib, DEV, *shape)


def test_row_stride(gpu_lib):
    SC.check_steps(gpu_lib, DEV, 65, 137, 2, strided=True)


def test_eight_iterations_large_case(gpu_lib):
    SC.check_fit('large case, 8 iterations', _large_fit(gpu_lib, tol=0.0, max_iter=8), _large_reference(0.0, 8))


def test_convergence_bookkeeping(gpu_lib):
    """tol = 5e-3 on the large case.  The yardstick's last non-converging change and its converging one must sit well clear of tol (>= 3 x and
    <= 1/3 x), so that fp32 cannot move the stopping iteration; the kernel path then stops at the same iteration with the same flag."""
    tol = 5e-3
    ref = _large_reference(tol, 200)
    lb = ref['lower_bounds']
    assert ref['converged'] and ref['n_iter'] >= 3
    last_open, closing = abs(lb[-2] - lb[-3]), abs(lb[-1] - lb[-2])
    print(f'yardstick: {ref["n_iter"]} iterations, last non-converging change {last_open:.4g}, converging change {closing:.4g}')
    assert last_open >= 3 * tol and closing <= tol / 3
    SC.check_fit('large case, tol = 5e-3', _large_fit(gpu_lib, tol=tol), ref)


def test_kmeans_init_on_planted_clusters(gpu_lib):
    """four planted clusters in D = 16 whose means are >= 20 standard deviations apart: init='kmeans' finds the planted partition (up to a
    permutation), and the fit from there equals the yardstick's fit from the same labels"""
    rng = np.random.default_rng(5)
    K, D, N = 4, 16, 600
    centres = 20.0 * np.eye(K, D) * np.sqrt(0.5) * 2.0          # pairwise distance 40 = 40 standard deviations (sd 1)
    planted = rng.integers(0, K, N)
    x = centres[planted] + rng.normal(size=(N, D))
    dist = np.linalg.norm(centres[:, None] - centres[None], axis=-1)
    assert dist[~np.eye(K, dtype=bool)].min() >= 20.0
    xt = torch.as_tensor(x, dtype=torch.float32, device=DEV)
    labels = SP.kmeans_labels(xt, K, seed=0, _lib_override=gpu_lib).cpu().numpy()
    table = np.zeros((K, K), dtype=np.int64)
    np.add.at(table, (planted, labels), 1)
    assert (table > 0).sum() == K and (table.sum(0) > 0).all(), f'labels do not match the planted partition:\n{table}'
    got = SP.fit_gmm(xt, n_components=K, tol=1e-3, init='kmeans', seed=0, _lib_override=gpu_lib)
    ref = SC.fit(xt.cpu().double(), K, tol=1e-3, labels_init=labels)
    SC.check_fit('planted clusters from k-means labels', got, ref)


def test_determinism_large_case(gpu_lib):
    a, b = _large_fit(gpu_lib, tol=0.0, max_iter=3), _large_fit(gpu_lib, tol=0.0, max_iter=3)
    assert a.lower_bounds == b.lower_bounds
    for k in ('weights', 'means', 'covariances'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.labels, b.labels)


def test_cli_writes_a_prior_the_fitting_loss_accepts(gpu_lib, tmp_path, capsys):
    """python -m humor_amd.state_prior --train-states X.npy --out DIR: prior_gmm.npz with the reference's keys, usable as init_motion_prior"""
    from humor_amd.fitting_loss import FittingLoss
    rng = np.random.default_rng(11)
    means, cov = SC.make_mixture(rng, 2, 138, 0.5, 0.3, 0.05)
    x, _ = SC.sample(rng, means, cov, 700)
    np.save(tmp_path / 'train.npy', x[:600].astype(np.float32))
    np.save(tmp_path / 'test.npy', x[600:].astype(np.float32))
    SP.main(['--train-states', str(tmp_path / 'train.npy'), '--test-states', str(tmp_path / 'test.npy'), '--out', str(tmp_path / 'out'),
             '--gmm-comps', '2'])
    out = capsys.readouterr().out
    assert 'test score' in out and 'fit (600, 138) states' in out
    loaded = SP.load_gmm(str(tmp_path / 'out' / 'prior_gmm.npz'))
    assert loaded['means'].shape == (2, 138) and abs(loaded['weights'].sum() - 1.0) < 1e-12
    loss = FittingLoss([{'init_motion_prior': 1.0}], init_motion_prior=SP.as_init_motion_prior(loaded, DEV), _lib_override=gpu_lib)
    s = torch.as_tensor(x[600:604], dtype=torch.float32, device=DEV)
    nll = loss.init_motion_prior_loss(s[:, :66].reshape(4, 22, 3), s[:, 66:132].reshape(4, 22, 3), s[:, 132:135], s[:, 135:138])
    SC.check_scalar('CLI prior: init_motion_prior_loss against -sum score_samples', float(nll),
                    -float(SP.score_samples(s, loaded, _lib_override=gpu_lib).double().sum()))


def test_round_trip_into_fitting_loss(gpu_lib, tmp_path):
    """save_gmm -> load_gmm -> as_init_motion_prior -> FittingLoss.init_motion_prior_loss on 4 states = -sum of score_samples"""
    from humor_amd.fitting_loss import FittingLoss
    c = SC.step_case(70, 138, 12)
    cov = torch.linalg.inv(c['P'] @ c['P'].transpose(1, 2))
    cov = 0.5 * (cov + cov.transpose(1, 2))
    SP.save_gmm(str(tmp_path), (c['weights'], c['means'], cov))
    loaded = SP.load_gmm(str(tmp_path))
    prior = SP.as_init_motion_prior(loaded, DEV)
    x = c['x'][:4].to(torch.float32).to(DEV)
    loss = FittingLoss([{'init_motion_prior': 1.0}], init_motion_prior=prior, _lib_override=gpu_lib)
    nll = loss.init_motion_prior_loss(x[:, :66].reshape(4, 22, 3), x[:, 66:132].reshape(4, 22, 3), x[:, 132:135], x[:, 135:138])
    ll = SP.score_samples(x, loaded, _lib_override=gpu_lib)
    SC.check_scalar('init_motion_prior_loss against -sum score_samples', float(nll), -float(ll.double().sum()))
    ref, _ = SC.e_step(x.cpu().double(), c['weights'], c['means'], c['P'])
    SC.check_scalar('score_samples against the yardstick', ll, ref)
