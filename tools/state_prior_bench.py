#!/usr/bin/env python
"""One EM iteration of the init-state mixture fit (E step + M step) at training size: the kernels of humor_amd/csrc/gmm_fit.hip against the
same iteration written with PyTorch operations on the same GPU (the unfused alternative), and -- where scikit-learn is importable -- against
scikit-learn's own E and M step on the host at a smaller N.

One process; both GPU paths warmed up; device-synchronised windows of at least --window seconds, the two paths ALTERNATED window by window;
the states rotate over --copies buffers (580 MB each at the default size) so that no pass finds its rows in the Infinity Cache by accident.
Prints per phase the median time, the window spread and 2 N K D^2 flop per step over the time against the 157.3 TFLOP/s fp32 MFMA peak
(the M step's kernel computes only the upper triangle: its rate is quoted for the full product, as for the other path), then the agreement
of the two paths' outputs, and writes everything to --out (bench.json, bench.txt).  --trace-only: a few iterations of each path, nothing else.

usage: state_prior_bench.py [--N 1048576 --D 138 --K 12 --copies 2 --windows 5 --window 0.5 --sklearn-N 65536 --out DIR] [--trace-only]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from humor_amd import _lib, state_prior as SP            # noqa: E402

PEAK_TFLOPS = 157.3


def make_problem(N, D, K, copies, dev, seed=0):
    """`copies` tables of states drawn from one seeded mixture (means N(0, 0.1^2), covariances A A^T + 0.05 I, A ~ N(0, 0.3^2) / sqrt(D)),
    and that mixture as the parameters of the timed iteration (fp64 host tensors)."""
    g = torch.Generator().manual_seed(seed)
    means = 0.1 * torch.randn(K, D, generator=g, dtype=torch.float64)
    A = 0.3 * torch.randn(K, D, D, generator=g, dtype=torch.float64) / math.sqrt(D)
    cov = A @ A.transpose(1, 2) + 0.05 * torch.eye(D, dtype=torch.float64)
    L = torch.linalg.cholesky(cov)
    gd = torch.Generator(device=dev).manual_seed(seed)
    tables = []
    for _ in range(copies):
        lab = torch.randint(0, K, (N,), generator=gd, device=dev)
        x = torch.randn(N, D, generator=gd, device=dev)
        for k in range(K):
            rows = (lab == k).nonzero().squeeze(1)
            x[rows] = means[k].float().to(dev) + x[rows] @ L[k].float().to(dev).t()
        tables.append(x.contiguous())
    weights = torch.full((K,), 1.0 / K, dtype=torch.float64)
    return tables, weights, means, cov


def torch_e_step(x, means, P, cst):
    lp = torch.stack([cst[k] - 0.5 * ((x - means[k]) @ P[k]).square().sum(1) for k in range(means.shape[0])], 1)
    ll = torch.logsumexp(lp, 1)
    return ll, torch.exp(lp - ll[:, None])


def torch_m_step(x, resp, shift):
    nk = resp.sum(0)
    sx, sxx = [], []
    for k in range(shift.shape[0]):
        d = x - shift[k]
        rd = d * resp[:, k:k + 1]
        sx.append(rd.sum(0))
        sxx.append(rd.t() @ d)
    return nk, torch.stack(sx), torch.stack(sxx)


def time_sklearn(N, D, K, weights, means, cov, seed=0):
    try:
        from sklearn.mixture import GaussianMixture
    except ImportError:
        return None
    import numpy as np
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K, N)
    x = means.numpy()[lab] + np.einsum('nde,ne->nd', torch.linalg.cholesky(cov).numpy()[lab], rng.normal(size=(N, D)))
    gm = GaussianMixture(n_components=K, covariance_type='full', reg_covar=1e-6, tol=0.0, max_iter=1, weights_init=weights.numpy(),
                         means_init=means.numpy(), precisions_init=torch.linalg.inv(cov).numpy())
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        gm.fit(x)                                            # (sets the parameters up and warms the BLAS threads)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            _, log_resp = gm._e_step(x)
            t1 = time.perf_counter()
            gm._m_step(x, log_resp)
            times.append((t1 - t0, time.perf_counter() - t1))
    e, m = (statistics.median(t[i] for t in times) for i in (0, 1))
    cores = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else os.cpu_count()
    return dict(N=N, e_ms=e * 1e3, m_ms=m * 1e3, cores=cores, omp_num_threads=os.environ.get('OMP_NUM_THREADS'),
                us_per_row_and_iteration=(e + m) / N * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=1 << 20)
    ap.add_argument('--D', type=int, default=138)
    ap.add_argument('--K', type=int, default=12)
    ap.add_argument('--copies', type=int, default=2)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5, help='least seconds per timed window')
    ap.add_argument('--sklearn-N', type=int, default=1 << 16)
    ap.add_argument('--out', default=None, help='directory for bench.json / bench.txt')
    ap.add_argument('--trace-only', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('state_prior_bench.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    lib = _lib.get_lib()
    N, D, K = a.N, a.D, a.K
    tables, weights, means, cov = make_problem(N, D, K, a.copies, dev)
    P = SP._precision_cholesky(cov)
    means32 = means.to(torch.float32)
    engines = [SP._Engine(x, K, lib) for x in tables]
    cst_d = (torch.log(weights) + torch.log(torch.diagonal(P, dim1=-2, dim2=-1)).sum(-1) - 0.5 * D * math.log(2 * math.pi)).float().to(dev)
    means_d, P_d = means32.to(dev), P.float().to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the kernels' launches only (parameters already on the device, no host read): what the device does per iteration
    def kernel_e(i):
        e = engines[i % a.copies]
        lib.call('ha_gmm_fit_estep', N, D, K, _lib.ptr(e.x), D, _lib.ptr(means_d), _lib.ptr(P_d), 1, _lib.ptr(cst_d), _lib.ptr(e.resp),
                 _lib.ptr(e.loglik), _lib.ptr(e.ll_part), e.stream)

    def kernel_m(i):
        e = engines[i % a.copies]
        lib.call('ha_gmm_fit_mstep', N, D, K, _lib.ptr(e.x), D, _lib.ptr(e.resp), _lib.ptr(means_d), _lib.ptr(e.nk), _lib.ptr(e.sx),
                 _lib.ptr(e.sxx), _lib.ptr(e.ws), e.stream)

    held = {}

    def torch_e(i):
        held[i % a.copies] = torch_e_step(tables[i % a.copies], means_d, P_d, cst_d)

    def torch_m(i):
        return torch_m_step(tables[i % a.copies], held[i % a.copies][1], means_d)

    phases = dict(kernel_e=kernel_e, kernel_m=kernel_m, torch_e=torch_e, torch_m=torch_m)
    for name, fn in phases.items():                           # warm-up of every path on every table (the M steps need the E steps' outputs)
        for i in range(2 * a.copies):
            fn(i)
    torch.cuda.synchronize()
    if a.trace_only:
        return

    def window(fn):
        n, t0 = 0, time.perf_counter()
        while True:
            for i in range(a.copies):
                fn(n + i)
            n += a.copies
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= a.window:
                return dt / n * 1e3

    times = {name: [] for name in phases}
    for _ in range(a.windows):
        for name, fn in phases.items():                      # alternated: kernel E, kernel M, torch E, torch M, kernel E, ...
            times[name].append(window(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    flop = 2.0 * N * K * D * D
    say(f'one EM iteration at N = {N}, D = {D}, K = {K} ({N * D * 4 / 1e6:.0f} MB of states, {a.copies} tables in rotation); '
        f'2 N K D^2 = {flop / 1e12:.3f} TFLOP per step')
    for k in phases:
        say(f'{k:9s}: median {med[k]:8.3f} ms, windows {" ".join("%.3f" % t for t in times[k])} (spread {spread[k]:.3f} ms) '
            f'-> {flop / med[k] / 1e9:7.2f} TFLOP/s = {100 * flop / med[k] / 1e9 / PEAK_TFLOPS:5.1f} % of {PEAK_TFLOPS} (fp32 MFMA)')
    kt, tt = med['kernel_e'] + med['kernel_m'], med['torch_e'] + med['torch_m']
    say(f'E + M: kernels {kt:.3f} ms ({2 * flop / kt / 1e9:.2f} TFLOP/s of 4 N K D^2), PyTorch operations {tt:.3f} ms ({2 * flop / tt / 1e9:.2f} TFLOP/s): '
        f'the kernels take {kt / tt:.2f} x the time of the operation form')
    # one whole iteration of fit_gmm's loop, host finish included (wall clock)
    eng = engines[0]
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        eng.estep(weights, means32, P)
        nke, mu2, cov2 = SP._finish(*eng.mstep(means32.double()), means32.double(), 1e-6)
        SP._precision_cholesky(cov2)
    torch.cuda.synchronize()
    whole = (time.perf_counter() - t0) / reps * 1e3
    say(f'whole iteration as fit_gmm runs it (parameter upload, two host reads, fp64 finish and {K} Cholesky factors on the host): {whole:.3f} ms')
    # agreement of the two paths at this size
    kernel_e(0); kernel_m(0)
    ll_t, resp_t = torch_e_step(tables[0], means_d, P_d, cst_d)
    nk_t, sx_t, sxx_t = torch_m_step(tables[0], engines[0].resp, means_d)
    torch.cuda.synchronize()
    e0 = engines[0]
    agree = dict(mean_loglik_kernel=float(e0.loglik.double().mean()), mean_loglik_torch=float(ll_t.double().mean()),
                 resp_max_abs_diff=float((e0.resp - resp_t).abs().max()),
                 nk_rel=float((e0.nk - nk_t).abs().max() / nk_t.abs().max()), sx_rel=float((e0.sx - sx_t).abs().max() / sx_t.abs().max()),
                 sxx_rel=float((e0.sxx - sxx_t).abs().max() / sxx_t.abs().max()))
    say('outputs, kernels against PyTorch operations (fp32 both): ' + json.dumps(agree))
    sk = time_sklearn(a.sklearn_N, D, K, weights, means, cov) if a.sklearn_N > 0 else None
    if sk:
        say(f'scikit-learn on the host, N = {sk["N"]}, {sk["cores"]} cores (OMP_NUM_THREADS={sk["omp_num_threads"]}): E {sk["e_ms"]:.1f} ms + M {sk["m_ms"]:.1f} ms '
            f'= {sk["us_per_row_and_iteration"]:.2f} us per row and iteration; the kernels: {kt / N * 1e3:.4f} us')
    else:
        say('scikit-learn: not importable here, not measured')
    result = dict(N=N, D=D, K=K, copies=a.copies, flop_per_step=flop, median_ms=med, spread_ms=spread, windows_ms=times, kernels_ms=kt,
                  torch_ops_ms=tt, whole_iteration_ms=whole, agreement=agree, sklearn=sk, peak_tflops=PEAK_TFLOPS)
    print(json.dumps(result))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'bench.json'), 'w') as f:
            json.dump(result, f, indent=1)
        with open(os.path.join(a.out, 'bench.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
