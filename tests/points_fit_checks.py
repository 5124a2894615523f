"""The points3d op (humor_amd/points_fit.py, csrc/points_fit.hip) against a CPU yardstick built from the SAME inputs:
oracle.chamfer_restated.nnsearch for d2 / idx (pinned bit for bit to the compiled reference), humor_amd.fitting_loss.robust_std /
apply_robust_weighting on sqrt(d2) for the median, sigma and the weights (pinned bit for bit to the reference by
test_robust_weighting_matches_reference), and an fp64 accumulation of the fp32 per-point terms, and of w (pred - obs) per vertex, for
the loss and the gradient.

Bars: idx, d2, med_d2 bit-exact (search / pure selection); sigma relative 1e-6 and exactly 0 where the yardstick's is 0 (one sqrt, one
subtraction, one division from the selected values); weights absolute 2e-6 (the bisquare weight is continuous at norm = 1: no element is
left out); loss relative 2e-6 against the fp64 sum (twice log2(N) 2^-24, the worst case of a pairwise fp32 sum of N <= 2^17 non-negative
terms); g_pred max-abs error <= 1e-5 of the largest entry (the bar of chamfer_checks.py)."""
import numpy as np
import torch

from humor_amd.fitting_loss import apply_robust_weighting, robust_std
from humor_amd.points_fit import robust_points_loss
from oracle import chamfer_restated as CR

TUNE = 4.6851


# --------------------------------------------------------------------------------------------------------------------------------
# inputs (CPU tensors)
# --------------------------------------------------------------------------------------------------------------------------------
def make_case(B, T, n_obs, V, seed, outliers=0.15):
    """A cloud of noisy vertices with a share of far outliers (so that the bisquare weights cover 0 .. 1)."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, T, V, 3, generator=g)
    pick = torch.randint(0, V, (B, T, n_obs), generator=g)
    obs = torch.gather(pred, 2, pick.unsqueeze(-1).expand(B, T, n_obs, 3)) + 0.05 * torch.randn(B, T, n_obs, 3, generator=g)
    far = torch.rand(B, T, n_obs, generator=g) < outliers
    obs = torch.where(far.unsqueeze(-1), 2.0 * torch.randn(B, T, n_obs, 3, generator=g), obs)
    return obs.contiguous(), pred.contiguous()


def make_tie_case(B, T, n_obs, V, seed):
    """chamfer_checks.make_clouds per frame: duplicated vertices (the lowest index wins) and queries exactly ON a vertex (d2 = 0)."""
    from chamfer_checks import make_clouds
    x1, x2 = make_clouds(B * T, n_obs, V, seed)
    return x1.reshape(B, T, n_obs, 3).contiguous(), x2.reshape(B, T, V, 3).contiguous()


def make_mad0_case():
    """Vertices on small integer coordinates, more than half of the observations at vertex + (0.25, 0, 0) (d2 = 0.0625 exactly), the rest
    farther away: the median absolute deviation is 0."""
    B, T, n_obs = 2, 2, 45
    grid = torch.tensor([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], dtype=torch.float32)       # V = 27
    V = grid.shape[0]
    g = torch.Generator().manual_seed(11)
    pick = torch.randint(0, V, (B, T, n_obs), generator=g)
    off = torch.tensor([0.25, 0.0, 0.0]).expand(B, T, n_obs, 3).clone()
    off[:, :, 30:] = torch.tensor([0.25, 0.25, 0.125])          # one third: d2 = 0.140625
    obs = grid[pick] + off
    return obs.contiguous(), grid.expand(B, T, V, 3).contiguous()


def make_narrow_case():
    """One vertex at the origin (two more far away); d2 = 1 + 2 j^2 2^-23 exactly, j <= 11: every distance in one binade, the bit patterns
    differ in the last byte only (every radix pass but the last sees ONE occupied bin), with heavy duplicates at the median rank."""
    B, T, n_obs = 2, 1, 150
    g = torch.Generator().manual_seed(12)
    j = torch.randint(0, 12, (B, T, n_obs), generator=g)
    j[:, :, :60] = 5                                            # 40 % duplicates, around the median rank
    obs = torch.zeros(B, T, n_obs, 3)
    obs[..., 0] = 1.0
    obs[..., 1] = (2.0 * j.float()) * 2.0 ** -12                  # y^2 = j^2 2^-22, exact
    pred = torch.tensor([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0], [0.0, -100.0, 0.0]]).expand(B, T, 3, 3).contiguous()
    return obs.contiguous(), pred


# --------------------------------------------------------------------------------------------------------------------------------
# yardstick
# --------------------------------------------------------------------------------------------------------------------------------
def yardstick(obs, pred, robust='bisquare', tune=TUNE):
    """CPU.  dict(d2, idx, weight [B,N]; med_d2, sigma [B] or None; loss (fp64 scalar), loss_b [B] fp64, g_pred [B,T,V,3] fp64)."""
    B, T, n_obs, _ = obs.shape
    V = pred.shape[2]
    d2n, idxn = CR.nnsearch(obs.reshape(B * T, n_obs, 3).numpy(), pred.reshape(B * T, V, 3).numpy())
    d2 = torch.from_numpy(d2n).reshape(B, T * n_obs)
    idx = torch.from_numpy(idxn).reshape(B, T * n_obs)
    r = d2.sqrt()
    weighted, w = apply_robust_weighting(r, robust, tune)              # fp32 terms w * r^2
    out = dict(d2=d2, idx=idx, weight=w, med_d2=None, sigma=None)
    if robust != 'none':
        out['med_d2'] = torch.median(d2, dim=-1)[0]
        out['sigma'] = robust_std(r).reshape(B)
    out['loss_b'] = 0.5 * weighted.double().sum(-1)
    out['loss'] = out['loss_b'].sum()
    near = torch.gather(pred.reshape(B * T, V, 3), 1, idx.reshape(B * T, n_obs, 1).long().expand(B * T, n_obs, 3))
    contrib = w.reshape(B * T, n_obs, 1) * (near - obs.reshape(B * T, n_obs, 3))          # fp32, as the kernel forms them
    g = torch.zeros(B * T, V, 3, dtype=torch.float64)
    g.scatter_add_(1, idx.reshape(B * T, n_obs, 1).long().expand(B * T, n_obs, 3), contrib.double())
    out['g_pred'] = g.reshape(B, T, V, 3)
    return out


def run_op(lib, device, obs, pred, robust='bisquare', tune=TUNE):
    p = pred.clone().to(device).requires_grad_(True)
    loss, d2, idx, w, med_d2, sigma = robust_points_loss(obs.to(device), p, robust, tune, _lib_override=lib, return_parts=True)
    g, = torch.autograd.grad(loss, p)
    cpu = lambda t: None if t is None else t.detach().cpu()
    return dict(loss=cpu(loss), d2=cpu(d2), idx=cpu(idx), weight=cpu(w), med_d2=cpu(med_d2), sigma=cpu(sigma), g_pred=cpu(g))


def _eq_bits(a, b):
    return np.array_equal(a.numpy(), b.numpy(), equal_nan=True)


def compare(got, ref, robust='bisquare', skip_rows=()):
    """Every bar of the module docstring; prints each figure before it asserts.  `skip_rows`: sequences whose yardstick is NaN (their sigma /
    weights must be NaN too; they are left out of the loss and gradient bars, which are then taken over the other sequences)."""
    B = ref['d2'].shape[0]
    rows = [b for b in range(B) if b not in skip_rows]
    fig = {}
    assert got['idx'].dtype == torch.int32 and _eq_bits(got['idx'], ref['idx']), 'nearest-vertex indices differ'
    assert _eq_bits(got['d2'], ref['d2']), 'squared distances differ'
    if robust != 'none':
        assert _eq_bits(got['med_d2'], ref['med_d2']), ('med_d2', got['med_d2'], ref['med_d2'])
        for b in range(B):
            s, s0 = float(got['sigma'][b]), float(ref['sigma'][b])
            if b in skip_rows:
                assert np.isnan(s) and np.isnan(s0), (b, s, s0)
            elif s0 == 0.0:
                assert s == 0.0, (b, s)
            else:
                fig['sigma_rel'] = max(fig.get('sigma_rel', 0.0), abs(s - s0) / abs(s0))
        print('sigma rel. error', fig.get('sigma_rel', 0.0))
        assert fig.get('sigma_rel', 0.0) <= 1e-6, fig
    else:
        assert got['med_d2'] is None and got['sigma'] is None
    for b in skip_rows:
        assert bool(torch.isnan(got['weight'][b]).all()) and bool(torch.isnan(ref['weight'][b]).all()), b
    if rows:
        fig['weight_abs'] = float((got['weight'][rows] - ref['weight'][rows]).abs().max())
        print('weights max abs error', fig['weight_abs'])
        assert fig['weight_abs'] <= 2e-6, fig
    if skip_rows:
        assert np.isnan(float(got['loss'])), got['loss']
    else:
        lref = float(ref['loss'])
        fig['loss_rel'] = abs(float(got['loss']) - lref) / abs(lref) if lref != 0.0 else abs(float(got['loss']))
        print('loss', float(got['loss']), 'yardstick', lref, 'rel. error', fig['loss_rel'])
        assert abs(float(got['loss']) - lref) <= 2e-6 * abs(lref), fig
    if rows:
        g, g0 = got['g_pred'][rows].double(), ref['g_pred'][rows]
        top = float(g0.abs().max())
        fig['grad_err'] = float((g - g0).abs().max())
        fig['grad_top'] = top
        print('g_pred max abs error', fig['grad_err'], 'largest entry', top)
        assert bool(torch.isfinite(got['g_pred'][rows]).all()), 'non-finite gradient'
        assert fig['grad_err'] <= 1e-5 * top, fig
    return fig


def check_case(lib, device, obs, pred, robust='bisquare', ref=None):
    ref = yardstick(obs, pred, robust) if ref is None else ref
    return compare(run_op(lib, device, obs, pred, robust), ref, robust), ref


# --------------------------------------------------------------------------------------------------------------------------------
# special cases
# --------------------------------------------------------------------------------------------------------------------------------
def check_zero_distance_gradient(lib, device):
    """(2, 3, 70, 130) with the tie constructions: a query exactly on a (duplicated) vertex has d2 = 0, picks the LOWER index, and its
    gradient contribution is finite and exactly 0 -- the frames' vertex 5 / 0 receive only the other observations' addends (bar above)."""
    obs, pred = make_tie_case(2, 3, 70, 130, seed=3)
    fig, ref = check_case(lib, device, obs, pred)
    d2 = ref['d2'].reshape(2, 3, 70)
    idx = ref['idx'].reshape(2, 3, 70)
    assert bool((d2[:, :, 3] == 0).all()) and bool((d2[:, :, 4] == 0).all()) and bool((idx[:, :, 3] == 5).all()) and bool((idx[:, :, 4] == 0).all())
    return fig


def check_mad_zero(lib, device):
    obs, pred = make_mad0_case()
    ref = yardstick(obs, pred)
    # the PyTorch chain on the CPU first: sigma 0, every weight 0, loss 0, gradient 0, nothing NaN
    assert bool((ref['sigma'] == 0).all()) and bool((ref['weight'] == 0).all()) and float(ref['loss']) == 0.0 and float(ref['g_pred'].abs().max()) == 0.0
    assert bool((ref['med_d2'] == 0.0625).all())
    got = run_op(lib, device, obs, pred)
    compare(got, ref)
    assert bool((got['sigma'] == 0).all()) and bool((got['weight'] == 0).all()) and float(got['loss']) == 0.0
    assert float(got['g_pred'].abs().max()) == 0.0
    assert not any(bool(torch.isnan(got[k]).any()) for k in ('d2', 'weight', 'med_d2', 'sigma', 'loss', 'g_pred'))


def check_narrow_range(lib, device):
    obs, pred = make_narrow_case()
    ref = yardstick(obs, pred)
    bits = ref['d2'].view(torch.int32)
    assert int((bits >> 8).unique().numel()) == 1 and int(bits.unique().numel()) > 4          # one binade, last byte only
    assert bool((ref['idx'] == 0).all()) and bool((ref['sigma'] > 0).all())
    return compare(run_op(lib, device, obs, pred), ref)


def check_nan_sequence(lib, device):
    """One NaN coordinate in sequence 1 of 3: that sequence's sigma and the loss are NaN, the other sequences' outputs are unaffected."""
    obs, pred = make_case(3, 2, 40, 50, seed=5)
    obs[1, 1, 7, 2] = float('nan')
    ref = yardstick(obs, pred)
    assert bool(torch.isnan(ref['sigma'][1])) and not bool(torch.isnan(ref['sigma'][[0, 2]]).any())
    got = run_op(lib, device, obs, pred)               # (a single call)
    return compare(got, ref, skip_rows=(1,))


def check_none(lib, device, shape=(2, 3, 70, 130), seed=6):
    """robust_loss='none': weights all 1, the loss / gradient bars, and central finite differences of the loss in three pred coordinates
    within 5 % (the bar of test_points3d_chamfer_term_through_the_optimizer)."""
    obs, pred = make_case(*shape, seed=seed, outliers=0.0)
    ref = yardstick(obs, pred, 'none')
    got = run_op(lib, device, obs, pred, 'none')
    assert bool((got['weight'] == 1).all())
    fig = compare(got, ref, 'none')
    B, T, n_obs, V = shape
    idx = ref['idx'].reshape(B, T, n_obs)
    eps = 1e-3
    o = obs.to(device)
    for (b, t, i, c) in ((0, 0, 0, 0), (B - 1, T - 1, n_obs // 2, 1), (0, T // 2, n_obs - 1, 2)):
        v = int(idx[b, t, i])                          # a vertex some observation is matched to
        vals = []
        for sgn in (1.0, -1.0):
            p = pred.clone()
            p[b, t, v, c] += sgn * eps
            vals.append(float(robust_points_loss(o, p.to(device), 'none', _lib_override=lib)))
        fd = (vals[0] - vals[1]) / (2 * eps)
        ga = float(got['g_pred'][b, t, v, c])
        print('finite difference', (b, t, v, c), fd, 'gradient', ga)
        assert abs(fd - ga) <= 0.05 * max(1.0, abs(fd)), (b, t, v, c, fd, ga)
    return fig


def check_determinism(lib, device, shape, seed=7):
    obs, pred = make_case(*shape, seed=seed)
    a, b = run_op(lib, device, obs, pred), run_op(lib, device, obs, pred)
    assert torch.equal(a['loss'], b['loss']) and torch.equal(a['g_pred'], b['g_pred'])
    assert bool(torch.isfinite(a['g_pred']).all())


# --------------------------------------------------------------------------------------------------------------------------------
# dispatch of FittingLoss.points3d_loss
# --------------------------------------------------------------------------------------------------------------------------------
def _fitting_loss(lib, robust, fused_points=True, weights=None):
    from humor_amd.configs import stage_weights
    from humor_amd.fitting_loss import FittingLoss
    return FittingLoss(stage_weights([weights or {'points3d': 1.0}] * 3), robust_loss=robust, use_chamfer=True, _lib_override=lib,
                       fused_points=fused_points)


def check_fallbacks(lib, device, monkeypatch):
    """'gm', observations that require a gradient and a body beyond the LDS bound take today's op chain: the call succeeds, equals the
    result with fused_points=False and never reaches the new op; 'bisquare' / 'none' on plain inputs do reach it."""
    from humor_amd import points_fit
    calls = []
    real = points_fit.robust_points_loss

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(points_fit, 'robust_points_loss', spy)
    obs, pred = make_case(2, 3, 70, 130, seed=8)
    obs, pred = obs.to(device), pred.to(device)

    def both(robust, obs_grad=False):
        out = []
        for fp in (True, False):
            o = obs.clone().requires_grad_(obs_grad)
            p = pred.clone().requires_grad_(True)
            loss = _fitting_loss(lib, robust, fp).points3d_loss(o, p)
            out.append((loss.detach(), torch.autograd.grad(loss, p)[0]))
        return out

    for robust in ('bisquare', 'none'):
        n0 = len(calls)
        (l1, g1), (l0, g0) = both(robust)
        assert len(calls) == n0 + 1, 'the op was not taken'
        assert abs(float(l1) - float(l0)) <= 1e-5 * abs(float(l0)), (robust, float(l1), float(l0))
    n0 = len(calls)
    # (the same code path twice: equal values; the chain's gradient comes from float atomics, so its bits may differ from call to call)
    same = lambda a, b: float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    for kw in (dict(robust='gm'), dict(robust='bisquare', obs_grad=True)):
        (l1, g1), (l0, g0) = both(**kw)
        assert torch.equal(l1, l0) and same(g1, g0), kw
    monkeypatch.setattr(points_fit, 'MAX_VERTS', 100)           # a stubbed bound instead of a huge model (V = 130 here)
    (l1, g1), (l0, g0) = both('bisquare')
    assert torch.equal(l1, l0) and same(g1, g0)
    assert len(calls) == n0, 'a fallback case reached the op'
