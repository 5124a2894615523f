"""Training the init-state prior: a full-covariance Gaussian mixture over ``joints | joints_vel | trans_vel | root_orient_vel`` of a
canonicalised frame 0, fitted by EM on the GPU (humor/train/train_state_prior.py:97-123 fits it with scikit-learn's GaussianMixture on
the CPU: tol=1e-3, reg_covar=1e-6, max_iter=200, k-means initialisation).

The two data passes of an iteration are kernels (humor_amd/csrc/gmm_fit.hip, exact-fp32 MFMA): the E step forms the responsibilities and the
log-likelihoods with one read of the states, the M step the weighted moments about the means the E step used.  The K small [D, D] problems --
the new means and covariances, their Cholesky factors -- are finished on the host in fp64 (one read of K (1 + D + D^2) floats per
iteration; the convergence test needs a host value anyway).  Control flow and formulas are scikit-learn's, so a fit from the same start
gives the same mixture to fp32 accuracy.  GPU tensors only (host tensors with the emulator library of the test tier): no CPU fallback.

    python -m humor_amd.state_prior --train-states X.npy --out DIR [--gmm-comps 12] [--test-states Y.npy]
"""
import argparse
import ctypes as C
import math
import os
import time

import numpy as np
import torch

from . import _lib

MAX_DIM, MAX_COMPONENTS = 256, 64
GMM_FILE = 'prior_gmm.npz'
_EPS = float(np.finfo(np.float64).eps)


class GMMFit:
    """Result of fit_gmm (fp64 host tensors): weights [K], means [K, D], covariances [K, D, D]; converged, n_iter, lower_bound and
    lower_bounds (one per iteration) as scikit-learn's converged_, n_iter_, lower_bound_, lower_bounds_; labels [N] from the final E step."""

    def __init__(self, weights, means, covariances, converged=False, n_iter=0, lower_bound=-math.inf, lower_bounds=(), labels=None):
        self.weights, self.means, self.covariances = weights, means, covariances
        self.converged, self.n_iter, self.lower_bound, self.lower_bounds = bool(converged), int(n_iter), float(lower_bound), list(lower_bounds)
        self.labels = labels


def _resolve_lib(x, lib):
    lib = lib if lib is not None else _lib.get_lib()
    if not (x.is_cuda or lib.emulator):
        raise _lib.HumorAmdError('humor_amd.state_prior runs on the GPU only (no CPU fallback)')
    return lib


def _as_states(states):
    x = torch.as_tensor(states)
    if x.dim() != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= MAX_DIM:
        raise ValueError(f'state_prior: states [N, D] with N >= 1 and 1 <= D <= {MAX_DIM} expected, got {tuple(x.shape)}')
    x = x.to(torch.float32)
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()                                   # (a row stride is taken as it is: a column slice of a wider table is not copied)
    return x


def _precision_cholesky(cov):
    """scikit-learn's _compute_precision_cholesky: chol(cov)^-T per component (upper triangular), fp64"""
    L, info = torch.linalg.cholesky_ex(cov)
    if bool((info != 0).any()) or not bool(torch.isfinite(L).all()):
        raise ValueError('fit_gmm: a covariance is not positive definite (collapsed or degenerate component): fewer components or a larger '
                         'reg_covar')
    eye = torch.eye(cov.shape[-1], dtype=cov.dtype).expand_as(cov)
    return torch.triu(torch.linalg.solve_triangular(L, eye, upper=False).transpose(1, 2)).contiguous()


class _Engine:
    """The kernels' buffers for one table of states; parameters go up and moments come back as fp32."""

    def __init__(self, x, K, lib, e_step_only=False):
        self.x, self.lib, self.K = x, lib, K
        self.N, self.D = x.shape
        nblk, wsf = C.c_int64(0), C.c_int64(0)
        lib.call('ha_gmm_fit_workspace', self.N, self.D, K, C.byref(nblk), C.byref(wsf))
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=x.device)
        self.loglik, self.ll_part = new(self.N), new(int(nblk.value))
        if not e_step_only:                                  # (score_samples needs neither the responsibilities nor the M step's buffers)
            self.resp, self.ws = new(self.N, K), new(int(wsf.value))
            self.nk, self.sx, self.sxx = new(K), new(K, self.D), new(K, self.D, self.D)
        self.stream = _lib.stream_ptr(x)

    def _up(self, t):
        return t.to(torch.float32).contiguous().to(self.x.device)

    def estep(self, weights, means32, P, with_resp=True):
        """-> mean log-likelihood (fp64 host sum of the block partials); self.resp / self.loglik hold the rest.  weights, P: fp64 host."""
        D = self.D
        cst = torch.log(weights) + torch.log(torch.diagonal(P, dim1=-2, dim2=-1)).sum(-1) - 0.5 * D * math.log(2.0 * math.pi)
        upper = int(bool((torch.tril(P, -1) == 0).all()))
        self._params = means_d, P_d, cst_d = self._up(means32), self._up(P), self._up(cst)      # (kept alive while the launch is queued)
        self.lib.call('ha_gmm_fit_estep', self.N, D, self.K, C.c_void_p(self.x.data_ptr()), self.x.stride(0), _lib.ptr(means_d), _lib.ptr(P_d),
                      upper, _lib.ptr(cst_d), _lib.ptr(self.resp) if with_resp else None, _lib.ptr(self.loglik), _lib.ptr(self.ll_part),
                      self.stream)
        return float(self.ll_part.cpu().double().sum()) / self.N

    def mstep(self, shift32, resp=None):
        """-> (nk [K], sx [K, D], sxx [K, D, D]) about shift32, fp64 host"""
        resp = self.resp if resp is None else resp
        self._shift = shift_d = self._up(shift32)
        self.lib.call('ha_gmm_fit_mstep', self.N, self.D, self.K, C.c_void_p(self.x.data_ptr()), self.x.stride(0), _lib.ptr(resp),
                      _lib.ptr(shift_d), _lib.ptr(self.nk), _lib.ptr(self.sx), _lib.ptr(self.sxx), _lib.ptr(self.ws), self.stream)
        return self.nk.cpu().double(), self.sx.cpu().double(), self.sxx.cpu().double()


def _finish(nk, sx, sxx, m, reg_covar):
    """scikit-learn's _estimate_gaussian_parameters from moments about m: (nk + 10 eps, means, covariances), fp64"""
    nke = nk + 10.0 * _EPS
    means = (sx + nk[:, None] * m) / nke[:, None]
    d = means - m                                            # sum r (x - mu)(x - mu)^T with x - mu = (x - m) - d
    sd = sx[:, :, None] * d[:, None, :]
    cov = (sxx - sd - sd.transpose(1, 2) + nk[:, None, None] * d[:, :, None] * d[:, None, :]) / nke[:, None, None]
    idx = torch.arange(cov.shape[-1])
    cov[:, idx, idx] += reg_covar
    return nke, means, cov


def _kmeans_labels(x, K, seed, max_iter=100):
    """k-means++ seeding and Lloyd iterations with PyTorch operations on the states' device; the draws come from a seeded host generator.
    (Off the hot path: an [N, K] distance matrix per iteration.)  Not scikit-learn's draw: another random stream."""
    N = x.shape[0]
    gen = torch.Generator().manual_seed(int(seed))
    xx = (x * x).sum(1)

    def dist2(c):
        return (xx[:, None] - 2.0 * (x @ c.t()) + (c * c).sum(1)[None, :]).clamp_min_(0.0)

    first = int(torch.randint(N, (1,), generator=gen))
    centres = x[first:first + 1].clone()
    closest = dist2(centres)[:, 0]
    for _ in range(1, K):
        p = closest.double().cpu()
        total = float(p.sum())
        pick = int(torch.multinomial(p / total, 1, generator=gen)) if total > 0.0 and math.isfinite(total) else int(torch.randint(N, (1,), generator=gen))
        centres = torch.cat([centres, x[pick:pick + 1]], 0)
        closest = torch.minimum(closest, dist2(x[pick:pick + 1])[:, 0])
    labels = dist2(centres).argmin(1)
    for _ in range(max_iter):
        onehot = torch.nn.functional.one_hot(labels, K).to(x.dtype)
        count = onehot.sum(0)
        summed = onehot.t() @ x                              # (a product, not index_add_: no floating-point atomics)
        centres = torch.where(count[:, None] > 0, summed / count.clamp_min(1.0)[:, None], centres)      # an empty cluster keeps its centre
        new = dist2(centres).argmin(1)
        if bool((new == labels).all()):
            break
        labels = new
    return labels


def kmeans_labels(states, n_components, seed=0, _lib_override=None):
    """The labels init='kmeans' starts from, [N] int64 on the states' device."""
    x = _as_states(states)
    _resolve_lib(x, _lib_override)
    return _kmeans_labels(x.contiguous(), int(n_components), seed)


def fit_gmm(states, n_components=12, tol=1e-3, reg_covar=1e-6, max_iter=200, init='kmeans', weights_init=None, means_init=None,
            precisions_init=None, labels_init=None, seed=0, _lib_override=None):
    """EM for a full-covariance mixture over states [N, D], scikit-learn's GaussianMixture.fit step for step: E step, lower bound = mean
    log-likelihood, M step, stop when |change| < tol, a final E step.  Start: weights_init + means_init + precisions_init (all three; the
    precision factors are chol(precisions_init), as there), or labels_init [N] (the M step on one-hot responsibilities, what scikit-learn does
    after its own k-means), or init='kmeans' (kmeans_labels from `seed`, then the labels route).  Raises on a non-finite lower bound and on
    a covariance that does not factor.  -> GMMFit."""
    x = _as_states(states)
    lib = _resolve_lib(x, _lib_override)
    K = int(n_components)
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError(f'fit_gmm: 1 <= n_components <= {MAX_COMPONENTS}')
    if max_iter < 1:
        raise ValueError('fit_gmm: max_iter >= 1')
    N, D = x.shape
    eng = _Engine(x, K, lib)
    host = lambda v: torch.as_tensor(np.asarray(v.detach().cpu()) if torch.is_tensor(v) else np.asarray(v), dtype=torch.float64)
    given = [v is not None for v in (weights_init, means_init, precisions_init)]
    if all(given):
        weights, means, prec = host(weights_init), host(means_init), host(precisions_init)
        if weights.shape != (K,) or means.shape != (K, D) or prec.shape != (K, D, D):
            raise ValueError('fit_gmm: weights_init [K], means_init [K, D], precisions_init [K, D, D] expected')
        P, info = torch.linalg.cholesky_ex(prec)             # (lower triangular: scikit-learn's _compute_precision_cholesky_from_precisions)
        if bool((info != 0).any()):
            raise ValueError('fit_gmm: precisions_init is not positive definite')
    elif any(given):
        raise ValueError('fit_gmm: weights_init, means_init and precisions_init are given together or not at all')
    else:
        if labels_init is None:
            if init != 'kmeans':
                raise ValueError("fit_gmm: init must be 'kmeans' when no start is given")
            labels = _kmeans_labels(x.contiguous(), K, seed)
        else:
            labels = torch.as_tensor(labels_init).to(device=x.device, dtype=torch.int64)
            if labels.shape != (N,) or int(labels.min()) < 0 or int(labels.max()) >= K:
                raise ValueError('fit_gmm: labels_init [N] with values in [0, n_components) expected')
        resp0 = torch.nn.functional.one_hot(labels, K).to(torch.float32).contiguous()
        m = x.mean(0).double().cpu().expand(K, D).contiguous()      # no mean yet: moments about (roughly) the data's centre
        nk, sx, sxx = eng.mstep(m, resp0)
        nke, means, cov = _finish(nk, sx, sxx, m, reg_covar)
        weights = nke / N
        P = _precision_cholesky(cov)
    covariances = None
    lower_bound, bounds, converged, n_iter = -math.inf, [], False, 0
    for n_iter in range(1, int(max_iter) + 1):
        prev = lower_bound
        means32 = means.to(torch.float32)
        lower_bound = eng.estep(weights, means32, P)
        if not math.isfinite(lower_bound):
            raise ValueError(f'fit_gmm: the lower bound is {lower_bound} at iteration {n_iter} (non-finite states, or a component that cannot '
                             f'explain any row)')
        m = means32.double()
        nke, means, covariances = _finish(*eng.mstep(m), m, reg_covar)
        weights = nke / nke.sum()
        P = _precision_cholesky(covariances)
        bounds.append(lower_bound)
        if abs(lower_bound - prev) < tol:
            converged = True
            break
    final = eng.estep(weights, means.to(torch.float32), P)
    if not math.isfinite(final):
        raise ValueError(f'fit_gmm: the log-likelihood of the fitted mixture is {final}')
    return GMMFit(weights, means, covariances, converged, n_iter, lower_bound, bounds, labels=eng.resp.argmax(1))


def _mixture(gmm):
    if isinstance(gmm, GMMFit):
        gmm = (gmm.weights, gmm.means, gmm.covariances)
    if isinstance(gmm, dict):
        gmm = gmm['gmm'] if 'gmm' in gmm else (gmm['weights'], gmm['means'], gmm['covariances'])
    w, mu, cov = (torch.as_tensor(np.asarray(v.detach().cpu()) if torch.is_tensor(v) else np.asarray(v), dtype=torch.float64) for v in gmm)
    return w, mu, cov


def score_samples(states, gmm, _lib_override=None):
    """Log-likelihood of every row of states [N, D] under gmm (a GMMFit, a (weights, means, covariances) triple or load_gmm's dict),
    through the E-step kernel -> [N] fp32 on the states' device."""
    x = _as_states(states)
    lib = _resolve_lib(x, _lib_override)
    w, mu, cov = _mixture(gmm)
    if mu.shape[1] != x.shape[1]:
        raise ValueError(f'score_samples: the states have {x.shape[1]} dimensions, the mixture {mu.shape[1]}')
    eng = _Engine(x, mu.shape[0], lib, e_step_only=True)
    eng.estep(w / w.sum(), mu.to(torch.float32), _precision_cholesky(cov), with_resp=False)
    return eng.loglik


def score(states, gmm, _lib_override=None):
    """Mean log-likelihood per row (what the reference's test_results prints)."""
    return float(score_samples(states, gmm, _lib_override).double().mean())


def save_gmm(path, gmm):
    """Writes the reference's prior_gmm.npz (keys weights, means, covariances); `path` may be a directory."""
    if os.path.isdir(path):
        path = os.path.join(path, GMM_FILE)
    w, mu, cov = _mixture(gmm)
    np.savez(path, weights=w.numpy(), means=mu.numpy(), covariances=cov.numpy())
    return path


def load_gmm(path):
    """Reads a prior_gmm.npz (the reference's or save_gmm's) -> dict of numpy arrays weights [K], means [K, D], covariances [K, D, D]."""
    if os.path.isdir(path):
        path = os.path.join(path, GMM_FILE)
    with np.load(path) as res:
        out = {k: np.asarray(res[k]) for k in ('weights', 'means', 'covariances')}
    K, D = out['means'].shape
    if out['weights'].shape != (K,) or out['covariances'].shape != (K, D, D):
        raise ValueError(f'{path}: weights [K], means [K, D], covariances [K, D, D] expected')
    return out


def as_init_motion_prior(gmm, device):
    """The init_motion_prior argument of MotionOptimizer / FittingLoss: {'gmm': (weights, means, covariances)} as fp32 tensors on device
    (humor/fitting/run_fitting.py:248-261)."""
    return {'gmm': tuple(v.to(device=device, dtype=torch.float32) for v in _mixture(gmm))}


def main(argv=None):
    ap = argparse.ArgumentParser(description='Fit the init-state GMM prior to an array of states (the --train-states path of the '
                                             "reference's train_state_prior.py).")
    ap.add_argument('--train-states', required=True, help='.npy, [N, D] states of the training split')
    ap.add_argument('--test-states', default=None, help='.npy, [M, D]: its mean log-likelihood is printed')
    ap.add_argument('--out', required=True, help=f'output directory ({GMM_FILE} is written there)')
    ap.add_argument('--gmm-comps', type=int, default=12)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    train = torch.from_numpy(np.load(args.train_states)).to(dev)
    os.makedirs(args.out, exist_ok=True)
    t0 = time.time()
    fit = fit_gmm(train, n_components=args.gmm_comps, seed=args.seed)
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)
    print(f'fit {tuple(train.shape)} states, {args.gmm_comps} components: {time.time() - t0:.2f} s, {fit.n_iter} iterations, '
          f'converged={fit.converged}, lower bound {fit.lower_bound:.6f}')
    print('saved', save_gmm(args.out, fit))
    print(f'train score {score(train, fit):.6f}')
    if args.test_states:
        print(f'test score {score(torch.from_numpy(np.load(args.test_states)).to(dev), fit):.6f}')


if __name__ == '__main__':
    main()
