"""The points3d data term of a point-cloud fit as ONE op: ``robust_points_loss(obs, pred)`` = 0.5 * sum of the robustly weighted squared
distances from every observed point to its nearest predicted vertex (FittingLoss.points3d_loss, humor/fitting/fitting_loss.py:378-396, with
the per-sequence bisquare weighting of fitting_utils.py:192-249), differentiable w.r.t. ``pred``.  humor_amd/csrc/points_fit.hip: one-way
search (the chamfer kernel), robust scale by radix selection instead of two sorts, weights and value; a deterministic backward without
floating-point atomics.  GPU tensors only (no CPU fallback).

The gradient of a point that sits exactly ON its vertex is 0 here (w * 0, the limit of the smooth objective); the op chain's sqrt backward
gives NaN there."""
import ctypes as C

import torch

from . import _lib

ROBUST = {'none': 0, 'bisquare': 1}
MAX_VERTS = 150 * 1024 // 12          # the backward keeps V * 3 fp32 accumulators in LDS (ha_points_fit_backward)
MAX_FRAMES = 65535


def usable(obs, pred, robust_loss, lib):
    """True when the op can evaluate the term for these tensors (FittingLoss falls back to the op chain otherwise)."""
    if robust_loss not in ROBUST or obs.dim() != 4 or pred.dim() != 4:
        return False
    if obs.dtype != torch.float32 or pred.dtype != torch.float32 or obs.requires_grad:
        return False
    if not ((obs.is_cuda and pred.is_cuda) or (lib is not None and lib.emulator and not obs.is_cuda and not pred.is_cuda)):
        return False
    B, T, n_obs, _ = obs.shape
    return pred.shape[2] <= MAX_VERTS and B * T <= MAX_FRAMES and n_obs >= 1 and T * n_obs < 2 ** 30


class PointsFit(torch.autograd.Function):
    """(pred [B,T,V,3]) -> (loss, d2, idx, weight, med_d2, sigma); only the loss carries a gradient."""

    @staticmethod
    def forward(ctx, pred, obs, lib, robust, tune):
        B, T, n_obs, _ = obs.shape
        V = pred.shape[2]
        pred, obs = pred.detach().contiguous(), obs.detach().contiguous()
        dev = pred.device
        new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        d2, weight, loss = new(B, T * n_obs), new(B, T * n_obs), new(B)
        idx = torch.empty(B, T * n_obs, dtype=torch.int32, device=dev)
        med_d2, sigma = (new(B), new(B)) if robust else (None, None)
        nbytes = C.c_int64(0)
        lib.call('ha_points_fit_workspace', B, T, n_obs, V, C.byref(nbytes))
        ws = torch.empty(max(int(nbytes.value), 4), dtype=torch.uint8, device=dev)
        lib.call('ha_points_fit_forward', B, T, n_obs, _lib.ptr(obs), V, _lib.ptr(pred), robust, float(tune), _lib.ptr(d2), _lib.ptr(idx),
                 _lib.ptr(weight), _lib.ptr(med_d2), _lib.ptr(sigma), _lib.ptr(loss), _lib.ptr(ws), _lib.stream_ptr(pred))
        ctx.lib, ctx.dims = lib, (B, T, n_obs, V)
        ctx.save_for_backward(obs, pred, idx, weight)
        if not robust:
            med_d2, sigma = new(0), new(0)
        ctx.mark_non_differentiable(d2, idx, weight, med_d2, sigma)
        return loss.sum(), d2, idx, weight, med_d2, sigma          # (the sequences' values in index order)

    @staticmethod
    def backward(ctx, g, *_):
        obs, pred, idx, weight = ctx.saved_tensors
        B, T, n_obs, V = ctx.dims
        g = g.detach().to(dtype=torch.float32).contiguous()
        g_pred = torch.empty_like(pred)
        ctx.lib.call('ha_points_fit_backward', B, T, n_obs, _lib.ptr(obs), V, _lib.ptr(pred), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(g),
                     _lib.ptr(g_pred), None, _lib.stream_ptr(pred))
        return g_pred, None, None, None, None


def robust_points_loss(obs, pred, robust_loss='bisquare', tuning_const=4.6851, _lib_override=None, return_parts=False):
    """obs [B,T,n_obs,3] (no gradient), pred [B,T,V,3] -> scalar loss; with return_parts also (d2, idx, weight, med_d2, sigma):
    d2 / idx / weight [B, T*n_obs], med_d2 / sigma [B] (None with robust_loss='none')."""
    lib = _lib_override if _lib_override is not None else _lib.get_lib()
    if robust_loss not in ROBUST:
        raise ValueError("robust_points_loss: robust_loss must be 'none' or 'bisquare' (the op chain of FittingLoss covers 'gm')")
    if not ((obs.is_cuda and pred.is_cuda) or lib.emulator):
        raise _lib.HumorAmdError('humor_amd.robust_points_loss runs on the GPU only (no CPU fallback)')
    if obs.requires_grad:
        raise ValueError('robust_points_loss: the observations carry no gradient in this op')
    if obs.dim() != 4 or pred.dim() != 4 or obs.shape[:2] != pred.shape[:2] or obs.shape[3] != 3 or pred.shape[3] != 3:
        raise ValueError('robust_points_loss: obs [B,T,n_obs,3] and pred [B,T,V,3] expected')
    if pred.shape[2] > MAX_VERTS:
        raise _lib.HumorAmdError(f'robust_points_loss: at most {MAX_VERTS} vertices (LDS accumulators of the backward)')
    loss, d2, idx, weight, med_d2, sigma = PointsFit.apply(pred.float(), obs.float(), lib, ROBUST[robust_loss], tuning_const)
    if not return_parts:
        return loss
    if robust_loss == 'none':
        med_d2 = sigma = None
    return loss, d2, idx, weight, med_d2, sigma
