"""Yardstick and shared cases of the state-prior tests: an fp64 PyTorch restatement of scikit-learn's full-covariance GaussianMixture.fit
(sklearn/mixture/_gaussian_mixture.py, _base.py; 1.7) -- the EM that humor/train/train_state_prior.py:97-123 runs -- and the comparisons
of the kernel path (humor_amd/state_prior.py, csrc/gmm_fit.hip) against it.  test_state_prior_yardstick.py pins the restatement to
scikit-learn itself (where installed) and to a golden file of scikit-learn's outputs (everywhere).

Bars (the project's flat ones, tests/test_points_fit_gpu.py): scalars -- lower bounds, scores, log-likelihoods -- 1e-5 relative; arrays
1e-4 of the reference array's largest entry."""
import functools
import math
import os

import numpy as np
import torch

from humor_amd import state_prior as SP

SCALAR_RTOL = 1e-5
ARRAY_RTOL = 1e-4
EPS = float(np.finfo(np.float64).eps)

# (N, D, K) of the single-step comparisons: a ragged row tile on both sides of 64, odd and even D across the MFMA k-step of 2, D below, at
# and off a multiple of 32, K = 1
STEP_SHAPES = [(1, 1, 1), (63, 5, 3), (65, 137, 2), (70, 138, 12), (130, 32, 1)]
LARGE = dict(K=12, D=138, N=4133)
SMALL = dict(K=3, D=5, N=203)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the yardstick (fp64)
# ---------------------------------------------------------------------------------------------------------------------------------------
def precision_cholesky(cov):
    """_compute_precision_cholesky: solve_triangular(chol(cov), I, lower=True).T per component"""
    L = torch.linalg.cholesky(cov)
    eye = torch.eye(cov.shape[-1], dtype=cov.dtype).expand_as(cov)
    return torch.linalg.solve_triangular(L, eye, upper=False).transpose(1, 2)


def e_step(x, w, mu, P):
    """_estimate_log_prob_resp -> (loglik [N], resp [N, K])"""
    D = x.shape[1]
    y = torch.einsum('nkd,kde->nke', x[:, None, :] - mu[None], P)
    log_det = torch.log(torch.diagonal(P, dim1=-2, dim2=-1)).sum(-1)
    lp = -0.5 * (D * math.log(2.0 * math.pi) + (y * y).sum(-1)) + log_det + torch.log(w)
    ll = torch.logsumexp(lp, dim=1)
    return ll, torch.exp(lp - ll[:, None])


def gaussian_parameters(x, resp, reg_covar):
    """_estimate_gaussian_parameters -> (nk + 10 eps, means, covariances)"""
    nk = resp.sum(0) + 10.0 * EPS
    means = resp.t() @ x / nk[:, None]
    diff = x[:, None, :] - means[None]
    cov = torch.einsum('nk,nkd,nke->kde', resp, diff, diff) / nk[:, None, None]
    idx = torch.arange(x.shape[1])
    cov[:, idx, idx] += reg_covar
    return nk, means, cov


def moments(x, resp, shift):
    """what ha_gmm_fit_mstep returns: nk, sx, sxx about shift [K, D]"""
    diff = x[:, None, :] - shift[None]
    return resp.sum(0), torch.einsum('nk,nkd->kd', resp, diff), torch.einsum('nk,nkd,nke->kde', resp, diff, diff)


def fit(x, K, tol=1e-3, reg_covar=1e-6, max_iter=200, weights_init=None, means_init=None, precisions_init=None, labels_init=None):
    """BaseMixture.fit_predict with n_init = 1 from a given start -> dict like state_prior.GMMFit"""
    x = torch.as_tensor(x, dtype=torch.float64)
    N = x.shape[0]
    if labels_init is not None:
        resp = torch.nn.functional.one_hot(torch.as_tensor(labels_init, dtype=torch.int64), K).to(torch.float64)
        nk, means, cov = gaussian_parameters(x, resp, reg_covar)
        w, P = nk / N, precision_cholesky(cov)
    else:
        w, means = torch.as_tensor(weights_init, dtype=torch.float64), torch.as_tensor(means_init, dtype=torch.float64)
        P = torch.linalg.cholesky(torch.as_tensor(precisions_init, dtype=torch.float64))
    lower_bound, bounds, converged, n_iter, cov, resp = -math.inf, [], False, 0, None, None
    for n_iter in range(1, max_iter + 1):
        prev = lower_bound
        ll, resp = e_step(x, w, means, P)
        nk, means, cov = gaussian_parameters(x, resp, reg_covar)
        w = nk / nk.sum()
        P = precision_cholesky(cov)
        lower_bound = float(ll.mean())
        bounds.append(lower_bound)
        if abs(lower_bound - prev) < tol:
            converged = True
            break
    return dict(weights=w, means=means, covariances=cov, converged=converged, n_iter=n_iter, lower_bound=lower_bound, lower_bounds=bounds,
                last_resp=resp)


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases, from a seeded NumPy generator
# ---------------------------------------------------------------------------------------------------------------------------------------
def make_mixture(rng, K, D, mean_sd, a_sd, diag):
    means = rng.normal(0.0, mean_sd, (K, D))
    A = rng.normal(0.0, a_sd, (K, D, D)) / math.sqrt(D)
    cov = A @ A.transpose(0, 2, 1) + diag * np.eye(D)[None]
    return means, cov


def sample(rng, means, cov, N):
    K, D = means.shape
    lab = rng.integers(0, K, N)
    L = np.linalg.cholesky(cov)
    return means[lab] + np.einsum('nde,ne->nd', L[lab], rng.normal(size=(N, D))), lab


@functools.lru_cache(maxsize=None)
def large_case(seed=0):
    """K = 12, D = 138, N = 4133: means N(0, 0.1^2), covariances A A^T + 0.05 I with A ~ N(0, 0.3^2) / sqrt(D); the start: means perturbed by
    N(0, 0.3^2), uniform weights, precisions 2 I"""
    rng = np.random.default_rng(seed)
    K, D, N = LARGE['K'], LARGE['D'], LARGE['N']
    means, cov = make_mixture(rng, K, D, 0.1, 0.3, 0.05)
    x, _ = sample(rng, means, cov, N)
    return dict(x=x, K=K, weights_init=np.full(K, 1.0 / K), means_init=means + rng.normal(0.0, 0.3, (K, D)),
                precisions_init=np.tile(2.0 * np.eye(D), (K, 1, 1)))


@functools.lru_cache(maxsize=None)
def small_golden():
    """tests/golden/state_prior_small.npz (tools/make_golden_state_prior.py): the small case and scikit-learn's six iterations on it"""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'state_prior_small.npz')) as g:
        return {k: np.asarray(g[k]) for k in g.files}


def small_case():
    """K = 3, D = 5, N = 203: means N(0, 0.5^2), covariances A A^T + 0.5 I (A ~ N(0, 1) / sqrt(D)): a genuinely soft mixture; the start:
    means perturbed by N(0, 0.3^2), uniform weights, precisions 2 I.  Read from the golden file, so every tier sees the same rows."""
    g = small_golden()
    return dict(x=g['x'], K=SMALL['K'], weights_init=g['weights_init'], means_init=g['means_init'], precisions_init=g['precisions_init'])


@functools.lru_cache(maxsize=None)
def small_reference(iters=6):
    """the yardstick's `iters` iterations on the small case (tol = 0), computed once"""
    return fit(tol=0.0, max_iter=iters, **small_case())


def soft_share(resp):
    """share of the rows whose largest responsibility is below 0.9"""
    return float((resp.max(1).values < 0.9).double().mean())


@functools.lru_cache(maxsize=None)
def step_case(N, D, K, seed=0):
    """data from a mixture and the parameters of one E and one M step: the true mixture a little off (fp64 tensors)"""
    rng = np.random.default_rng(1000 * seed + 7 * N + 3 * D + K)
    means, cov = make_mixture(rng, K, D, 0.5, 1.0, 0.5)
    x, _ = sample(rng, means, cov, N)
    w = rng.uniform(0.5, 1.5, K)
    t = lambda v: torch.as_tensor(v, dtype=torch.float64)
    return dict(x=t(x), weights=t(w / w.sum()), means=t(means + rng.normal(0.0, 0.1, (K, D))), P=precision_cholesky(t(cov)))


@functools.lru_cache(maxsize=None)
def step_reference(N, D, K, seed=0):
    """the yardstick's E step on step_case (computed once, shared)"""
    c = step_case(N, D, K, seed)
    ll, resp = e_step(c['x'].to(torch.float32).double(), c['weights'], c['means'], c['P'])      # (the states are fp32 data)
    return dict(loglik=ll, resp=resp)


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------------------
def scalar_err(got, ref):
    """largest relative distance of scalars (or of every entry of an array of scalars)"""
    got, ref = torch.as_tensor(got, dtype=torch.float64).cpu(), torch.as_tensor(ref, dtype=torch.float64).cpu()
    return float(((got - ref).abs() / ref.abs()).max())


def array_err(got, ref):
    """largest distance over the reference array's largest entry"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max())


def check_scalar(name, got, ref):
    err = scalar_err(got, ref)
    print(f'{name}: relative distance {err:.3e} (bar {SCALAR_RTOL:.0e})')
    assert err <= SCALAR_RTOL, f'{name}: {err:.3e} > {SCALAR_RTOL:.0e}'


def check_array(name, got, ref):
    err = array_err(got, ref)
    print(f'{name}: distance / largest entry {err:.3e} (bar {ARRAY_RTOL:.0e})')
    assert err <= ARRAY_RTOL, f'{name}: {err:.3e} > {ARRAY_RTOL:.0e}'


def check_fit(name, got, ref):
    """a GMMFit against the yardstick's dict: the same iteration count and flag, bounds and parameters inside the bars"""
    assert got.n_iter == ref['n_iter'] and got.converged == ref['converged'], \
        f'{name}: n_iter / converged {got.n_iter} / {got.converged}, yardstick {ref["n_iter"]} / {ref["converged"]}'
    check_scalar(f'{name} lower bounds', got.lower_bounds, ref['lower_bounds'])
    check_scalar(f'{name} lower bound', got.lower_bound, ref['lower_bound'])
    for k in ('weights', 'means', 'covariances'):
        check_array(f'{name} {k}', getattr(got, k), ref[k])


def run_steps(lib, device, N, D, K, strided=False):
    """one ha_gmm_fit_estep and one ha_gmm_fit_mstep on step_case(N, D, K) through state_prior's engine -> (loglik, resp, nk, sx, sxx)"""
    c = step_case(N, D, K)
    x = c['x'].to(torch.float32)
    if strided:                                               # a column slice of a wider table: row stride D + 3, NaN around the rows
        wide = torch.full((N, D + 3), float('nan'), dtype=torch.float32)
        wide[:, 2:2 + D] = x
        x = wide.to(device)[:, 2:2 + D]
    else:
        x = x.to(device)
    x = SP._as_states(x)
    assert x.stride(0) == (D + 3 if strided else D)
    eng = SP._Engine(x, K, lib)
    m32 = c['means'].to(torch.float32)
    mean_ll = eng.estep(c['weights'], m32, c['P'])
    loglik, resp = eng.loglik.clone(), eng.resp.clone()
    nk, sx, sxx = eng.mstep(m32.double())
    return mean_ll, loglik, resp, nk, sx, sxx


def check_steps(lib, device, N, D, K, strided=False):
    ref = step_reference(N, D, K)
    mean_ll, loglik, resp, nk, sx, sxx = run_steps(lib, device, N, D, K, strided)
    tag = f'({N}, {D}, {K}){" strided" if strided else ""}'
    check_scalar(f'{tag} loglik', loglik, ref['loglik'])
    check_scalar(f'{tag} mean loglik', mean_ll, float(ref['loglik'].mean()))
    check_array(f'{tag} resp', resp, ref['resp'])
    # the M step is checked on the kernel's own responsibilities (its input), against fp64 moments of exactly those
    c = step_case(N, D, K)
    mom = moments(c['x'].to(torch.float32).double(), resp.cpu().double(), c['means'].to(torch.float32).double())
    for name, got, want in zip(('nk', 'sx', 'sxx'), (nk, sx, sxx), mom):
        check_array(f'{tag} {name}', got, want)
    assert torch.equal(sxx, sxx.transpose(1, 2)), f'{tag}: sxx is not exactly symmetric'
