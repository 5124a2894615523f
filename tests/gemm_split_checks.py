"""Checks of the batched GEMM's short-chain forms (prior_gemm_kernel<RM, KS, TN>: K split over 2 / 4 waves, one column tile per wave)
through the ha_mlp_* entry points, against an fp64 host evaluation of the same network.  Emulator tier on CPU, gfx950 build on the GPU.

A network is [in, hidden.., out] with either LeakyReLU(0.2) (epilogues 4 forward / 5 adjoint, 0 for the last layer and the input
gradient) or GroupNorm(16) + ReLU (epilogues 1 / 3, 0 likewise).  Which form each of its launches takes under the default policy
(ha_tune_set gemm_ks 2; plan_prior_gemm in humor_amd/csrc/rollout.hip) at a few row tiles (at 1888 rows the policy also weighs how many
waves would share a SIMD, and pins what the plain form runs with more than 512 waves), with K the layer's input width:
    K < 256 (32, 96, 126)        KS 1           256 <= K < 512 (339)    KS 2           K >= 512 (512, 1024)    KS 4
    epilogue 0 / 4 / 5           TN 1 (one 32-column tile per wave)     epilogue 1 / 3          TN 2 (the GroupNorm group stays in the wave)
gemm_ks 0 runs every launch in the plain form (KS 1, TN 2): the code path the split forms are measured against.

The bar (set by the issue that introduced the forms): against the fp64 result, the largest error of the default-policy run is at most
twice the largest error of the plain-form run on the same input -- a split shortens the accumulation chains, the factor two covers
single-entry luck.  Launches that the policy leaves unsplit (K < 256) or pins must reproduce the plain form bit for bit."""
import torch
import torch.nn as nn

from humor_amd import mlp as M

SLOPE = 0.2


def make_net(dims, act, seed):
    g = torch.Generator().manual_seed(seed)
    lin = []
    for i in range(len(dims) - 1):
        w = torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5
        b = 0.1 * torch.randn(dims[i + 1], generator=g)
        lin.append((w, b))
    gns = None
    if act == 'gn_relu':
        gns = [(1.0 + 0.2 * torch.randn(dims[i], generator=g), 0.1 * torch.randn(dims[i], generator=g)) for i in range(1, len(dims) - 1)]
    return lin, gns


def reference(lin, gns, x, w):
    """fp64 forward and input gradient of sum(y * w) on the host."""
    x = x.double().requires_grad_(True)
    h = x
    for i, (W, b) in enumerate(lin):
        h = h @ W.double().t() + b.double()
        if i + 1 < len(lin):
            if gns is None:
                h = nn.functional.leaky_relu(h, SLOPE)
            else:
                h = torch.relu(nn.functional.group_norm(h, 16, gns[i][0].double(), gns[i][1].double(), eps=1e-5))
    gx = torch.autograd.grad((h * w.double()).sum(), x)[0]
    return h.detach(), gx


def run(lib, device, f, x, w, ks):
    lib.call('ha_tune_set', b'gemm_ks', ks)
    try:
        xd = x.to(device).requires_grad_(True)
        y = f(xd)
        gx = torch.autograd.grad((y * w.to(device)).sum(), xd)[0]
        return y.detach().cpu(), gx.cpu()
    finally:
        lib.call('ha_tune_set', b'gemm_ks', 2)


def launch_unsplit(K, n_out, nrt):
    """Rules (b) and (c) of the policy: a launch keeps every output bit of the plain form if its K has fewer than four 64-channel slices
    (a wave keeps at least two slices when it splits; TN = 1 alone reorders nothing), or if the plain form already runs it with more than
    512 waves or two row tiles per wave (pinned: same instantiation, same grid)."""
    nslices, ncb = -(-K // 64), -(-(-(-n_out // 32)) // 8)
    return nslices < 4 or ncb * nrt * 4 > 512 or (nrt // 2) * ncb >= 512


def check_net(lib, device, dims, act, N, seed=0, verbose=True):
    """Returns the four errors (plain y, policy y, plain gx, policy gx)."""
    lin, gns = make_net(dims, act, seed)
    f = M.FusedMLP(lib, device.index or 0 if device.type == 'cuda' else 0, lin, act=act, slope=SLOPE, gns=gns)
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(N, dims[0], generator=g)
    w = torch.randn(N, dims[-1], generator=g)
    y_ref, gx_ref = reference(lin, gns, x, w)
    y0, gx0 = run(lib, device, f, x, w, 0)
    y2, gx2 = run(lib, device, f, x, w, 2)
    y2b, gx2b = run(lib, device, f, x, w, 2)
    nrt = -(-N // 32)
    import gemm_forms_checks as GF      # (imports this module)
    GF.assert_launch_unsplit_agrees(lib, dims, act, N)      # the Python restatement below against plan_prior_gemm itself
    fwd_same = all(launch_unsplit(dims[i], dims[i + 1], nrt) for i in range(len(dims) - 1))
    bwd_same = fwd_same and all(launch_unsplit(dims[i + 1], dims[i], nrt) for i in range(len(dims) - 1))      # (the adjoint reads the forward's stash)
    err = lambda a, r: (a.double() - r).abs().max().item()
    e = (err(y0, y_ref), err(y2, y_ref), err(gx0, gx_ref), err(gx2, gx_ref))
    if verbose:
        print(f'{act} {dims} N={N}: max err vs fp64  y plain {e[0]:.3e} policy {e[1]:.3e} | gx plain {e[2]:.3e} policy {e[3]:.3e}'
              f' | bitwise equal to plain: y {torch.equal(y0, y2)} (must: {fwd_same}) gx {torch.equal(gx0, gx2)} (must: {bwd_same})')
    assert torch.isfinite(y2).all() and torch.isfinite(gx2).all()
    assert torch.equal(y2, y2b) and torch.equal(gx2, gx2b), 'two runs of the same launch differ: the partial tiles must be added in fixed order'
    assert e[1] <= 2.0 * e[0], f'forward: policy form {e[1]:.3e} > 2 x plain form {e[0]:.3e}'
    assert e[3] <= 2.0 * e[2], f'adjoint: policy form {e[3]:.3e} > 2 x plain form {e[2]:.3e}'
    if fwd_same:
        assert torch.equal(y0, y2), 'forward: an unsplit launch (TN = 1 or pinned) changed bits'
    if bwd_same:
        assert torch.equal(gx0, gx2), 'adjoint: an unsplit launch (TN = 1 or pinned) changed bits'
    return e


# (dims, act): every (TN, KS) form behind every epilogue it serves, ragged K tails (339, 96, 126) and odd tile counts (126 -> 4 tiles of
# which the last is partial, 339 -> 11, 96 -> 3, 32 -> 1).  The forms named are those of a small batch (a few row tiles); a single-layer
# network's adjoint is the transposed product (K = the output width).
NETS = [
    ((32, 126), 'leaky_relu'),                # epi 0, TN 1 KS 1 both ways: K = 32 is one ragged slice, K = 126 -> 128 two
    ((126, 96), 'leaky_relu'),                # epi 0, TN 1 KS 1 both ways, 3 tiles / 4 tiles
    ((96, 1024), 'leaky_relu'),               # epi 0, TN 1 KS 1 (K = 64 + 32) | adjoint TN 1 KS 4, 3 tiles
    ((339, 1024), 'leaky_relu'),              # epi 0, TN 1 KS 2: K = 5 x 64 + 19, the tail rides with the last part | adjoint KS 4, 11 tiles
    ((512, 126), 'leaky_relu'),               # epi 0, TN 1 KS 4, 4 tiles (the last 30 columns wide)
    ((512, 32), 'leaky_relu'),                # epi 0, TN 1 KS 4, a single tile
    ((32, 512, 126), 'leaky_relu'),           # epi 4 KS 1 | epi 0 KS 4 | adjoint: epi 5 at K = 128 (KS 1), epi 0 at K = 512 (the VPoser decoder's shapes)
    ((512, 512, 512), 'leaky_relu'),          # epi 4 and epi 5 behind TN 1 KS 4
    ((339, 96, 339), 'leaky_relu'),           # epi 4 and epi 5 behind TN 1 KS 2 (3 tiles), epi 0 at K = 96 with 11 tiles
    ((512, 512, 48), 'gn_relu'),              # epi 1 behind TN 2 KS 4 (32-channel groups); adjoint epi 3 at K = 48
    ((339, 512, 1024, 32), 'gn_relu'),        # epi 1 behind TN 2 KS 2 and KS 4 (64-channel groups); epi 3 behind KS 1 and KS 4
]


def check_all(lib, device, N, nets=NETS):
    for dims, act in nets:
        check_net(lib, device, dims, act, N, seed=len(dims) + dims[0])
