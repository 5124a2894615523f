"""Checks of the layout passes folded into the batched GEMM (ha_tune_set "gemm_fold", humor_amd/csrc/rollout.hip): the row-major store
epilogue that replaces mlp_out_kernel (y of ha_mlp_forward without a tail, g_x of ha_mlp_backward) and the forward prior_io_kernel
(prior_mu / prior_var of a roll-out), and the row-major A operand that replaces transpose_in_kernel in front of a narrow first layer.
Emulator tier on CPU, gfx950 build on the GPU.

The bar (set by the issue that introduced the knob): gemm_fold 1 and gemm_fold 0 run the same MFMAs in the same order, the same expf and
the same GroupNorm code, so every output is BITWISE equal between the two -- y, g_x, prior_mu, prior_var and the roll-out's gradients --
and a destination filled with NaN keeps its NaN in every word behind the last row (a store to a row >= N or a column >= C of the last row
lands there).  The spare words behind a destination cover the rest of its last 32-row tile (every line a store without its row guard could
reach) plus one line, so that a broken guard fails an assertion instead of writing outside the allocation."""
import ctypes as C

import torch

import gemm_split_checks as GC
import rollout_checks as RC
from humor_amd import _lib
from humor_amd import mlp as M


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class fold:
    """with fold(lib, v): the knob set to v, back to the default (1) afterwards."""

    def __init__(self, lib, v):
        self.lib, self.v = lib, v

    def __enter__(self):
        self.lib.call('ha_tune_set', b'gemm_fold', self.v)

    def __exit__(self, *a):
        self.lib.call('ha_tune_set', b'gemm_fold', 1)


def mlp_raw(lib, device, f, x, g_y, tail=M.TAIL_NONE):
    """ha_mlp_forward / ha_mlp_backward called directly into NaN-filled destinations with spare lines behind them.
    Returns the whole buffers (y, g_x) and the count of valid words in each."""
    N = x.shape[0]
    x, g_y = x.to(device).contiguous(), g_y.to(device).contiguous()
    n = C.c_int64()
    lib.call('ha_mlp_workspace', f.ptr, N, C.byref(n))
    ws = torch.full((n.value,), float('nan'), dtype=torch.float32, device=device)
    out_w = f.out_dim if tail == M.TAIL_NONE else f.out_dim // 2
    spare = -(-N // 32) * 32 - N + 1          # lines up to the end of the last row tile, and one more
    y = torch.full(((N + spare) * out_w,), float('nan'), dtype=torch.float32, device=device)
    g_x = torch.full(((N + spare) * f.in_dim,), float('nan'), dtype=torch.float32, device=device)
    lib.call('ha_mlp_forward', f.ptr, N, _lib.ptr(x), tail, _lib.ptr(y), _lib.ptr(ws), _lib.stream_ptr(x))
    lib.call('ha_mlp_backward', f.ptr, N, _lib.ptr(g_y), tail, _lib.ptr(ws), _lib.ptr(g_x), _lib.stream_ptr(x))
    return y.cpu(), N * out_w, g_x.cpu(), N * f.in_dim


def check_mlp_net(lib, device, dims, act, N, seed=0, tail=M.TAIL_NONE, verbose=True):
    """One network of gemm_split_checks.NETS: y and g_x with the layout passes folded in against the separate launches."""
    lin, gns = GC.make_net(dims, act, seed)
    f = M.FusedMLP(lib, device.index or 0 if device.type == 'cuda' else 0, lin, act=act, slope=GC.SLOPE, gns=gns)
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(N, dims[0], generator=g)
    out_w = dims[-1] if tail == M.TAIL_NONE else dims[-1] // 2
    g_y = torch.randn(N, out_w, generator=g)
    with fold(lib, 0):
        y0, ny, gx0, ngx = mlp_raw(lib, device, f, x, g_y, tail)
    with fold(lib, 1):
        y1, _, gx1, _ = mlp_raw(lib, device, f, x, g_y, tail)
    if verbose:
        print(f'{act} {dims} N={N} tail={tail}: y bitwise {same_bits(y0[:ny], y1[:ny])} g_x bitwise {same_bits(gx0[:ngx], gx1[:ngx])} | NaN words left behind '
              f'y {int(torch.isnan(y1[ny:]).sum())}/{y1.numel() - ny} g_x {int(torch.isnan(gx1[ngx:]).sum())}/{gx1.numel() - ngx}')
    assert torch.isfinite(y0[:ny]).all() and torch.isfinite(gx0[:ngx]).all(), 'the separate layout passes left words unwritten'
    assert same_bits(y0[:ny], y1[:ny]), 'y: the row-major store epilogue changed bits'
    assert same_bits(gx0[:ngx], gx1[:ngx]), 'g_x: the row-major store epilogue changed bits'
    assert torch.isnan(y1[ny:]).all(), 'y: a store went beyond row N / column C'
    assert torch.isnan(gx1[ngx:]).all(), 'g_x: a store went beyond row N / column in_dim'


def rollout_raw(lib, device, hm, past, z, want_grads=True):
    """ha_humor_rollout_forward into NaN-filled prior_mu / prior_var with spare words behind them, then the adjoint of a fixed objective."""
    B, S = z.shape[0], z.shape[1]
    handle = hm._net_handle(device)
    n = C.c_int64()
    lib.call('ha_humor_rollout_workspace', handle.ptr, B, S, C.byref(n))
    nan = lambda k: torch.full((k,), float('nan'), dtype=torch.float32, device=device)
    stash, world = nan(n.value), nan(B * S * 348)
    spare = -(-B // 32) * 32 - B + 1          # sequences up to the end of the last row tile, and one more
    pm, pv = nan((B + spare) * S * 48), nan((B + spare) * S * 48)
    past, z = past.to(device).contiguous(), z.to(device).contiguous()
    lib.call('ha_humor_rollout_forward', handle.ptr, B, S, _lib.ptr(past), _lib.ptr(z), _lib.ptr(world), _lib.ptr(pm), _lib.ptr(pv), _lib.ptr(stash),
             _lib.stream_ptr(past))
    out = [world.cpu(), pm.cpu(), pv.cpu()]
    if want_grads:
        g = torch.Generator().manual_seed(B * 100 + S)
        gw = torch.randn(B * S * 348, generator=g).to(device)
        gm, gv = torch.randn(B * S * 48, generator=g).to(device), torch.randn(B * S * 48, generator=g).to(device)
        g_past, g_z = nan(B * 339), nan(B * S * 48)
        lib.call('ha_humor_rollout_backward_ex', handle.ptr, B, S, _lib.ptr(z), _lib.ptr(gw), _lib.ptr(gm), _lib.ptr(gv), _lib.ptr(stash), _lib.ptr(g_past),
                 _lib.ptr(g_z), None, _lib.stream_ptr(z))
        out += [g_past.cpu(), g_z.cpu()]
    return out


def check_prior(lib, device, B, S, seed=0, want_grads=True):
    """The prior-shaped case: 96 outputs (mean | log-variance) over S > 1 steps of B sequences, B not a multiple of 32.  prior_mu / prior_var
    from the last prior layer's epilogue against prior_io_kernel's, and the adjoint that reads the same stash."""
    assert S > 1 and B % 32 != 0
    hm, sd = RC.make_model(lib, device, seed=seed, contractive=True)
    g = torch.Generator().manual_seed(seed + 5)
    past, z = RC.canonical_state(B, g), torch.randn(B, S, 48, generator=g)
    with fold(lib, 0):
        r0 = rollout_raw(lib, device, hm, past, z, want_grads)
    with fold(lib, 1):
        r1 = rollout_raw(lib, device, hm, past, z, want_grads)
    n = B * S * 48
    names = ['world', 'prior_mu', 'prior_var', 'g_past_in0', 'g_z']
    for name, a, b in zip(names, r0, r1):
        k = n if name in ('prior_mu', 'prior_var') else a.numel()
        print(f'roll-out {B} x {S} {name}: bitwise {same_bits(a[:k], b[:k])}, finite {bool(torch.isfinite(a[:k]).all())}')
        assert torch.isfinite(a[:k]).all(), name + ': words left unwritten'
        assert same_bits(a[:k], b[:k]), name + ': gemm_fold 1 and 0 differ'
    for name, b in (('prior_mu', r1[1]), ('prior_var', r1[2])):
        assert torch.isnan(b[n:]).all(), name + ': a store went beyond sequence B'
    if S > 12:      # (a long chain amplifies fp32 rounding: the flat bar below is for short ones, the long ones are tests/rollout_checks.py's)
        return
    # and against the oracle, so that "equal" is not "equally wrong"
    w64, (pm64, pv64) = RC.H.roll_out({k: v.double() for k, v in sd.items()}, past.double(), z.double())
    assert (r1[1][:n].double().reshape(B, S, 48) - pm64).abs().max().item() < RC.FWD_TOL
    assert ((r1[2][:n].double().reshape(B, S, 48) - pv64).abs() / pv64.abs().clamp(min=1.0)).max().item() < RC.FWD_TOL
