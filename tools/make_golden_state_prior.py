"""Writes tests/golden/state_prior_small.npz: the small case of the state-prior tests (K = 3, D = 5, N = 203, a soft mixture) and what
scikit-learn's GaussianMixture makes of it in six EM iterations from the stored start.  Needs scikit-learn (the tests do not: they read
the file).  `python tools/make_golden_state_prior.py`"""
import math
import os
import warnings

import numpy as np
from sklearn.mixture import GaussianMixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'state_prior_small.npz')
K, D, N, ITERS, REG = 3, 5, 203, 6, 1e-6


def main():
    rng = np.random.default_rng(0)
    means = rng.normal(0.0, 0.5, (K, D))
    A = rng.normal(0.0, 1.0, (K, D, D)) / math.sqrt(D)
    cov = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(D)[None]
    lab = rng.integers(0, K, N)
    x = means[lab] + np.einsum('nde,ne->nd', np.linalg.cholesky(cov)[lab], rng.normal(size=(N, D)))
    start = dict(weights_init=np.full(K, 1.0 / K), means_init=means + rng.normal(0.0, 0.3, (K, D)),
                 precisions_init=np.tile(2.0 * np.eye(D), (K, 1, 1)))
    gm = GaussianMixture(n_components=K, covariance_type='full', tol=0.0, reg_covar=REG, max_iter=ITERS, **start)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                       # (tol = 0: it never reports convergence)
        gm.fit(x)
    assert gm.n_iter_ == ITERS
    np.savez(OUT, x=x, iters=ITERS, reg_covar=REG, weights=gm.weights_, means=gm.means_, covariances=gm.covariances_,
             lower_bounds=np.asarray(gm.lower_bounds_), score_samples=gm.score_samples(x), resp=gm.predict_proba(x), **start)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
