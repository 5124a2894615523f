#!/usr/bin/env python
"""Value + gradient of the points3d term at the fitting batch's size: the one-way robust op (humor_amd/points_fit.py) against the unfused
op chain (FittingLoss(fused_points=False): chamfer both ways, two torch.median per sequence, ATen weighting, atomics in the backward).

One process, both paths warmed up, device-synchronised windows of at least --window seconds, the two paths ALTERNATED window by window;
prints the median of each path, the spread of its windows and the difference, then the agreement of the two paths' outputs at that size,
and one JSON line.  --trace-only runs a few evaluations of each path and nothing else (for a kernel trace in a run of its own).

usage: bench_points_fit.py [--B 32 --T 60 --n-obs 2048 --V 6890 --windows 5 --window 0.5 --robust bisquare] [--trace-only]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from humor_amd.configs import stage_weights               # noqa: E402
from humor_amd.fitting_loss import FittingLoss            # noqa: E402


def make_inputs(B, T, n_obs, V, dev, seed=0):
    """A cloud of noisy vertices of a random body-sized vertex set, with 10 % far outliers (seeded)."""
    g = torch.Generator().manual_seed(seed)
    pred = 0.5 * torch.randn(B, T, V, 3, generator=g)
    pick = torch.randint(0, V, (B, T, n_obs), generator=g)
    obs = torch.gather(pred, 2, pick.unsqueeze(-1).expand(B, T, n_obs, 3)) + 0.02 * torch.randn(B, T, n_obs, 3, generator=g)
    far = torch.rand(B, T, n_obs, generator=g) < 0.1
    obs = torch.where(far.unsqueeze(-1), torch.randn(B, T, n_obs, 3, generator=g), obs)
    return obs.to(dev).contiguous(), pred.to(dev).contiguous().requires_grad_(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=32)
    ap.add_argument('--T', type=int, default=60)
    ap.add_argument('--n-obs', type=int, default=2048)
    ap.add_argument('--V', type=int, default=6890)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5, help='least seconds per timed window')
    ap.add_argument('--robust', default='bisquare', choices=['none', 'bisquare'])
    ap.add_argument('--trace-only', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_points_fit.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    obs, pred = make_inputs(a.B, a.T, a.n_obs, a.V, dev)
    W = stage_weights([{'points3d': 1.0}] * 3)
    fl = {name: FittingLoss(W, robust_loss=a.robust, use_chamfer=True, fused_points=fp) for name, fp in (('op', True), ('chain', False))}

    def evaluate(name):
        pred.grad = None
        loss = fl[name].points3d_loss(obs, pred)
        loss.backward()
        return loss.detach(), pred.grad

    out = {}
    for name in fl:                                        # warm-up of both paths (code objects, allocator), and the outputs to compare
        for _ in range(3):
            loss, grad = evaluate(name)
        out[name] = (loss.clone(), grad.clone())
    torch.cuda.synchronize()
    if a.trace_only:
        return

    def window(name):
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(4):
                evaluate(name)
            n += 4
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= a.window:
                return dt / n * 1e3

    times = {name: [] for name in fl}
    for _ in range(a.windows):
        for name in fl:                                    # alternated: op, chain, op, chain, ...
            times[name].append(window(name))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    for k in fl:
        print(f'{k:5s}: median {med[k]:.3f} ms per value + gradient, windows {" ".join("%.3f" % t for t in times[k])} (spread {spread[k]:.3f} ms)')
    diff, noise = med['chain'] - med['op'], max(spread.values())
    print(f'chain - op = {diff:.3f} ms, largest spread {noise:.3f} ms: the op is ' + ('FASTER by more than the spread' if diff > noise else 'NOT faster by more than the spread'))
    (l1, g1), (l0, g0) = out['op'], out['chain']
    loss_rel = abs(l1.item() - l0.item()) / abs(l0.item())
    gerr, gtop = (g1 - g0).abs().max().item(), g0.abs().max().item()
    print(f'outputs: loss op {l1.item():.6f} chain {l0.item():.6f} (rel. diff {loss_rel:.2e}); gradient max abs diff {gerr:.3e} of largest entry {gtop:.3e}')
    print(json.dumps(dict(B=a.B, T=a.T, n_obs=a.n_obs, V=a.V, robust=a.robust, op_ms=med['op'], chain_ms=med['chain'], op_spread_ms=spread['op'],
                          chain_spread_ms=spread['chain'], faster_by_more_than_spread=bool(diff > noise), loss_rel_diff=loss_rel,
                          grad_max_abs_diff=gerr, grad_largest=gtop)))


if __name__ == '__main__':
    main()
