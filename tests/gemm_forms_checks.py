"""Checks of every form of the batched GEMM (prior_gemm_kernel<RM, KS, TN>, humor_amd/csrc/rollout.hip) behind every epilogue it serves, each
form FORCED through the knobs (ha_tune_set gemm_rm / gemm_ks / gemm_fold) and CONFIRMED through the read-only plan query ha_debug_gemm_plan
before the run, against an fp64 host evaluation of the same network.  Emulator tier on CPU, gfx950 build on the GPU.

A form is written RM KS TN as one number (212 = two row tiles per wave, no K split, a pair of column tiles), an epilogue by its number in
GemmTask (0 raw; 1 GroupNorm + ReLU; 3 its adjoint; 4 LeakyReLU; 5 its adjoint).  A network [in, hidden.., out] of ha_mlp_* is one launch
per layer and direction: forward layer l has K = dims[l] and dims[l + 1] columns behind epilogue 4 / 1 (0 for the last layer), its adjoint
K = dims[l + 1] and dims[l] columns behind 5 / 3 (0 for the first layer).  CASES lists, per entry, the (form, epilogue) of every launch in
launch order; check_case asserts the list against the hook, so an entry whose launches the policy moves elsewhere fails instead of
silently testing something else, and REQUIRED is what the union of the table must be.

What a case asserts (bars set by the issue that introduced this module, none of them measured on the code under test):
  * outputs finite, two runs bitwise equal, every word behind row N / column C of y and g_x still NaN;
  * a single-layer network (epilogue 0 alone): per element |y - y64| <= (K + 2) 2^-24 (|x| |W|^T + |b|), the textbook bound of a length-K
    fp32 dot product plus the bias addition, evaluated in fp64; the same for g_x with W transposed;
  * a multi-layer network: tests/mlp_checks.py's bars (2e-5 forward, 1e-4 gradient, relative to max(1, |ref|_max)), and
    tests/gemm_split_checks.py's rule against the plain form (112 = gemm_rm 1 + gemm_ks 0) on the same input: at most twice its error;
  * bitwise: RM 2 == RM 1 at equal KS / TN (gemm_rm 2 against the plain form), TN 1 == TN 2 at KS 1 (an entry whose launches all have
    KS 1 against the plain form), gemm_fold 1 == gemm_fold 0 under every forced form, and a destination that is 4- but not 8-byte aligned
    (single-float stores) == the aligned one (float pairs)."""
import ctypes as C

import torch

import gemm_fold_checks as FC
import gemm_split_checks as GC
import rollout_checks as RC
from humor_amd import mlp as M

GN, LR = 'gn_relu', 'leaky_relu'
PRIOR_DIMS = (339, 1024, 1024, 1024, 1024, 96)      # HuMoR's prior network (GroupNorm(16) + ReLU), mean | log-variance out


# ------------------------------------------------------------------------------------------------------------------------------------
# the plan query
# ------------------------------------------------------------------------------------------------------------------------------------
def plan(lib, ntiles, nslices, nrt, epi):
    """(RM, KS, TN, column blocks) of plan_prior_gemm for one launch under the live knobs."""
    out = (C.c_int * 4)()
    fn = lib._dll.ha_debug_gemm_plan
    fn.restype, fn.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)]
    rc = fn(int(ntiles), int(nslices), int(nrt), int(epi), out)
    assert rc == 0, f'ha_debug_gemm_plan({ntiles}, {nslices}, {nrt}, {epi}) -> {rc}'
    return tuple(out)


def form(lib, ntiles, nslices, nrt, epi):
    rm, ks, tn, _ = plan(lib, ntiles, nslices, nrt, epi)
    return rm * 100 + ks * 10 + tn


def launches(dims, act, N, direction='both'):
    """(ntiles, nslices, nrt, epi) of every batched GEMM launch of ha_mlp_forward ('fwd'), ha_mlp_backward ('bwd') or both, in launch order."""
    n, nrt = len(dims) - 1, -(-N // 32)
    hid_f, hid_b = (4, 5) if act == LR else (1, 3)
    fwd = [(-(-dims[l + 1] // 32), -(-dims[l] // 64), nrt, 0 if l + 1 == n else hid_f) for l in range(n)]
    bwd = [(-(-dims[l] // 32), -(-dims[l + 1] // 64), nrt, 0 if l == 0 else hid_b) for l in range(n - 1, -1, -1)]
    return {'fwd': fwd, 'bwd': bwd, 'both': fwd + bwd}[direction]


def forms(lib, dims, act, N, direction='both'):
    """[(form, epilogue)] the hook reports for the launches of the network under the live knobs."""
    return [(form(lib, *q), q[3]) for q in launches(dims, act, N, direction)]


class knobs:
    """with knobs(lib, rm=.., ks=.., fold=..): the three GEMM knobs set, back to their defaults (0, 2, 1) afterwards."""
    DEFAULT = dict(gemm_rm=0, gemm_ks=2, gemm_fold=1)

    def __init__(self, lib, rm=0, ks=2, fold=1):
        self.lib, self.v = lib, dict(gemm_rm=rm, gemm_ks=ks, gemm_fold=fold)

    def __enter__(self):
        for k, v in self.v.items():
            self.lib.call('ha_tune_set', k.encode(), v)
        return self

    def __exit__(self, *a):
        for k, v in self.DEFAULT.items():
            self.lib.call('ha_tune_set', k.encode(), v)


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
def case(name, dims, act, N, rm, ks, claims, misalign=False, slow=False):
    return dict(name=name, dims=dims, act=act, N=N, rm=rm, ks=ks, claims=claims, misalign=misalign, slow=slow)


# Edges (what each entry is in the table for, besides its cells):
#   rows      1 / 32 / 45 / 64 / 70 under RM 2: one group with one live tile; two tiles, the second with 13 live rows; a full group; three tiles =
#             a last group of ONE live tile (the clamped second tile is computed and dropped) with 6 live rows
#   ragged K  19, 96, 126, 339; odd tile counts 339 -> 11, 96 -> 3, 32 -> 1; 126: the last tile is 30 columns wide
#   epilogue 0: slab only (every entry's gemm_fold 0 run), plain row-major store (gemm_fold 1), row-major A operand (in_dim 19 / 32 / 48 / 64),
#             single-float stores: odd line width (19, 339) and, with misalign, an even width (126, 96, 32) behind a 4-byte aligned pointer
#   GroupNorm groups of 32 channels (512 wide) and of 64 (1024 wide: r2_gn64, p_gn64 -- the only 1024-wide entries of the CPU tier)
#   big rows: 122 / 142 behind epilogues 0 / 4 / 5 exist only where TN 1 would put two waves on a SIMD (more than 1024 waves) and TN 2 does not:
#             17 row tiles x 16 column tiles x KS 4, 65 row tiles x 8 column tiles x KS 2 (the smallest launches with that property)
CASES = [
    # ---- RM 2 (gemm_rm 2; the K split is built for RM 1 only, so gemm_ks does not matter) ----
    case('r2_1row', (32, 126), LR, 1, 2, 2, [(212, 0), (212, 0)], misalign=True),
    case('r2_32rows', (64, 96), LR, 32, 2, 2, [(212, 0), (212, 0)], misalign=True),
    case('r2_64rows', (126, 96), LR, 64, 2, 2, [(212, 0), (212, 0)]),
    case('r2_70rows_a19', (19, 512, 126), LR, 70, 2, 2, [(212, 4), (212, 0), (212, 5), (212, 0)], misalign=True),
    case('r2_70rows_k339', (339, 96, 339), LR, 70, 2, 2, [(212, 4), (212, 0), (212, 5), (212, 0)]),
    case('r2_45rows_gn32', (48, 512, 32), GN, 45, 2, 2, [(212, 1), (212, 0), (212, 3), (212, 0)], misalign=True),
    case('r2_70rows_gn32', (339, 512, 339), GN, 70, 2, 2, [(212, 1), (212, 0), (212, 3), (212, 0)]),
    case('r2_70rows_gn64', (48, 1024, 32), GN, 70, 2, 2, [(212, 1), (212, 0), (212, 3), (212, 0)]),
    # ---- the plain form (gemm_ks 0) ----
    case('plain_lr', (32, 512, 126), LR, 45, 0, 0, [(112, 4), (112, 0), (112, 5), (112, 0)]),
    case('plain_gn', (48, 512, 32), GN, 33, 1, 0, [(112, 1), (112, 0), (112, 3), (112, 0)]),
    # ---- the policy's short-chain forms at a few row tiles (gemm_ks 2) ----
    case('p_111', (32, 126), LR, 33, 0, 2, [(111, 0), (111, 0)], misalign=True),
    case('p_111_k96', (126, 96), LR, 1, 0, 2, [(111, 0), (111, 0)]),
    case('p_121', (339, 126), LR, 45, 0, 2, [(121, 0), (111, 0)]),
    case('p_111_141', (32, 512, 126), LR, 33, 0, 2, [(111, 4), (141, 0), (111, 5), (141, 0)]),
    case('p_121_lr', (339, 96, 339), LR, 45, 0, 2, [(121, 4), (111, 0), (121, 5), (111, 0)]),
    case('p_141_lr', (512, 512, 512), LR, 33, 1, 2, [(141, 4), (141, 0), (141, 5), (141, 0)]),
    case('p_122_gn', (339, 512, 339), GN, 33, 0, 2, [(122, 1), (141, 0), (122, 3), (141, 0)]),
    case('p_142_gn', (512, 512, 512), GN, 64, 0, 2, [(142, 1), (141, 0), (142, 3), (141, 0)]),
    case('p_gn64', (512, 1024, 32), GN, 33, 0, 2, [(142, 1), (141, 0), (112, 3), (141, 0)]),
    # ---- the forced split (gemm_ks 3: the deepest split everywhere, TN 1 wherever the epilogue allows) ----
    case('f_lr', (339, 512, 339), LR, 40, 0, 3, [(121, 4), (141, 0), (121, 5), (141, 0)]),
    case('f_gn', (512, 512, 48), GN, 45, 0, 3, [(142, 1), (141, 0), (112, 3), (141, 0)]),
    case('f_k19', (19, 339), LR, 32, 0, 3, [(111, 0), (121, 0)]),
    # ---- TN 2 with a K split behind the epilogues that would allow TN 1: the policy takes it where TN 1 needs a second round of waves ----
    case('big_142', (512, 512, 512), LR, 530, 0, 2, [(142, 4), (142, 0), (142, 5), (142, 0)]),
    case('big_122', (256, 256, 256), LR, 2050, 0, 2, [(122, 4), (122, 0), (122, 5), (122, 0)]),
]

REQUIRED = {(f, e) for f in (212, 112, 122, 142) for e in (0, 1, 3, 4, 5)} | {(f, e) for f in (111, 121, 141) for e in (0, 4, 5)}
# the roll-out entries (check_rollout_case): the prior's launches under gemm_rm 2, among them the mean | exp(log-variance) store
ROLLOUT_CASES = [dict(B=5, S=3), dict(B=70, S=3)]
ROLLOUT_CLAIMS = [(212, 1)] * 4 + [(212, 0)] + [(212, 3)] * 4 + [(212, 0)]


def claimed():
    s = set(ROLLOUT_CLAIMS)
    for c in CASES:
        s |= set(c['claims'])
    return s


# ------------------------------------------------------------------------------------------------------------------------------------
# one case
# ------------------------------------------------------------------------------------------------------------------------------------
def mlp_raw_at(lib, device, f, x, g_y, off):
    """gemm_fold_checks.mlp_raw with y and g_x `off` floats into their NaN-filled buffers (off = 1: 4- but not 8-byte aligned destinations).
    Returns (y, valid words, g_x, valid words) like mlp_raw; the words in front of a destination must still be NaN."""
    if off == 0:
        return FC.mlp_raw(lib, device, f, x, g_y)
    from humor_amd import _lib
    N = x.shape[0]
    x, g_y = x.to(device).contiguous(), g_y.to(device).contiguous()
    n = C.c_int64()
    lib.call('ha_mlp_workspace', f.ptr, N, C.byref(n))
    nan = lambda k: torch.full((k,), float('nan'), dtype=torch.float32, device=device)
    ws = nan(n.value)
    spare = -(-N // 32) * 32 - N + 1
    y, g_x = nan(off + (N + spare) * f.out_dim), nan(off + (N + spare) * f.in_dim)
    assert _lib.ptr(y).value % 8 == 0 and _lib.ptr(g_x).value % 8 == 0
    lib.call('ha_mlp_forward', f.ptr, N, _lib.ptr(x), M.TAIL_NONE, C.c_void_p(_lib.ptr(y).value + 4 * off), _lib.ptr(ws), _lib.stream_ptr(x))
    lib.call('ha_mlp_backward', f.ptr, N, _lib.ptr(g_y), M.TAIL_NONE, _lib.ptr(ws), C.c_void_p(_lib.ptr(g_x).value + 4 * off), _lib.stream_ptr(x))
    y, g_x = y.cpu(), g_x.cpu()
    assert torch.isnan(y[:off]).all() and torch.isnan(g_x[:off]).all(), 'a store went in front of the destination'
    return y[off:], N * f.out_dim, g_x[off:], N * f.in_dim


def _err(a, r):
    return (a.double() - r).abs().max().item()


def check_case(lib, device, c, verbose=True):
    dims, act, N = c['dims'], c['act'], c['N']
    seed = len(dims) + dims[0] + N
    lin, gns = GC.make_net(dims, act, seed)
    f = M.FusedMLP(lib, device.index or 0 if device.type == 'cuda' else 0, lin, act=act, slope=GC.SLOPE, gns=gns)
    g = torch.Generator().manual_seed(seed + 100)
    x, w = torch.randn(N, dims[0], generator=g), torch.randn(N, dims[-1], generator=g)
    y64, gx64 = GC.reference(lin, gns, x, w)
    ny, ngx = N * dims[-1], N * dims[0]

    def run(rm, ks, fold, off=0, claims=None):
        with knobs(lib, rm, ks, fold):
            if claims is not None:      # what will run, asked before it runs
                got = forms(lib, dims, act, N)
                assert got == claims, f"{c['name']}: the table claims {claims}, plan_prior_gemm gives {got} (gemm_rm {rm} gemm_ks {ks})"
            y, n1, gx, n2 = mlp_raw_at(lib, device, f, x, w, off)
        assert (n1, n2) == (ny, ngx)
        assert torch.isnan(y[ny:]).all(), f"{c['name']}: y: a store went beyond row N / column C (rm {rm} ks {ks} fold {fold} off {off})"
        assert torch.isnan(gx[ngx:]).all(), f"{c['name']}: g_x: a store went beyond row N / column in_dim (rm {rm} ks {ks} fold {fold} off {off})"
        return y[:ny].reshape(N, -1), gx[:ngx].reshape(N, -1)

    y, gx = run(c['rm'], c['ks'], 1, claims=c['claims'])
    yb, gxb = run(c['rm'], c['ks'], 1)
    y0, gx0 = run(c['rm'], c['ks'], 0)
    plain = [(112, e) for _, e in c['claims']]
    yp, gxp = (y, gx) if c['claims'] == plain else run(1, 0, 1, claims=plain)
    e = (_err(yp, y64), _err(y, y64), _err(gxp, gx64), _err(gx, gx64))
    same = FC.same_bits(y, yp), FC.same_bits(gx, gxp)
    if verbose:
        print(f"{c['name']:>16} {act} {dims} N={N} rm {c['rm']} ks {c['ks']} {sorted(set(c['claims']))}: max err vs fp64  y plain {e[0]:.3e} forced {e[1]:.3e}"
              f" | gx plain {e[2]:.3e} forced {e[3]:.3e} | bitwise equal to plain: y {same[0]} gx {same[1]}")
    assert torch.isfinite(y).all() and torch.isfinite(gx).all(), 'words left unwritten'
    assert FC.same_bits(y, yb) and FC.same_bits(gx, gxb), 'two runs of the same launches differ'
    assert FC.same_bits(y, y0) and FC.same_bits(gx, gx0), 'gemm_fold 1 and gemm_fold 0 differ under a forced form'
    if c['misalign']:
        ym, gxm = run(c['rm'], c['ks'], 1, off=1)
        assert FC.same_bits(y, ym) and FC.same_bits(gx, gxm), 'single-float stores (4-byte aligned destination) differ from float pairs'
    # ---- against fp64 ----
    if len(dims) == 2:
        W, b = lin[0][0].double(), lin[0][1].double()
        u = 2.0 ** -24
        bar_y = (dims[0] + 2) * u * (x.double().abs() @ W.abs().t() + b.abs())
        bar_g = (dims[1] + 2) * u * (w.double().abs() @ W.abs())
        for name, got, ref, bar in (('y', y, y64, bar_y), ('g_x', gx, gx64, bar_g), ('y plain', yp, y64, bar_y), ('g_x plain', gxp, gx64, bar_g)):
            over = ((got.double() - ref).abs() - bar).max().item()
            worst = ((got.double() - ref).abs() / bar.clamp(min=1e-300)).max().item()
            if verbose:
                print(f"{'':>16} {name}: largest |error| / bound {worst:.3f}")
            assert over <= 0.0, f"{c['name']} {name}: an element is {worst:.2f} x its rounding bound"
    else:
        for name, got, ref, tol in (('y', y, y64, 2e-5), ('g_x', gx, gx64, 1e-4)):
            s = max(1.0, ref.abs().max().item())
            assert _err(got, ref) <= tol * s, f"{c['name']} {name}: max err {_err(got, ref):.3e} (scale {s:.3g})"
        assert e[1] <= 2.0 * e[0], f"{c['name']}: forward: forced form {e[1]:.3e} > 2 x plain form {e[0]:.3e}"
        assert e[3] <= 2.0 * e[2], f"{c['name']}: adjoint: forced form {e[3]:.3e} > 2 x plain form {e[2]:.3e}"
    # ---- bitwise against the plain form: RM 2 == RM 1 at equal KS / TN, TN 1 == TN 2 at KS 1 ----
    if all(fm // 10 % 10 == 1 for fm, _ in c['claims']):
        assert same[0], f"{c['name']}: forward: a launch without a K split changed bits against the plain form"
        assert same[1], f"{c['name']}: adjoint: a launch without a K split changed bits against the plain form"
    return e


def check_rollout_case(lib, device, B, S, seed=0, verbose=True):
    """The prior-shaped store (mean | expf(log-variance), rm_S = S > 1 steps interleaved) behind RM 2: a roll-out under gemm_rm 2 against the same
    under gemm_rm 1 + gemm_ks 0 and under gemm_fold 0, bit for bit; two runs; NaN behind sequence B; prior_mu / prior_var against the fp64 oracle."""
    hm, sd = RC.make_model(lib, device, seed=seed, contractive=True)
    g = torch.Generator().manual_seed(seed + 5)
    past, z = RC.canonical_state(B, g), torch.randn(B, S, 48, generator=g)
    N = 32 * S * -(-B // 32)
    with knobs(lib, 2, 2, 1):
        got = forms(lib, PRIOR_DIMS, GN, N)
        assert got == ROLLOUT_CLAIMS, f'roll-out {B} x {S}: the table claims {ROLLOUT_CLAIMS}, plan_prior_gemm gives {got}'
        r2 = FC.rollout_raw(lib, device, hm, past, z)
        r2b = FC.rollout_raw(lib, device, hm, past, z)
    with knobs(lib, 2, 2, 0):
        r2f = FC.rollout_raw(lib, device, hm, past, z)
    with knobs(lib, 1, 0, 1):
        assert all(fm == 112 for fm, _ in forms(lib, PRIOR_DIMS, GN, N))
        r1 = FC.rollout_raw(lib, device, hm, past, z)
    n = B * S * 48
    for name, a, b, c0, d in zip(['world', 'prior_mu', 'prior_var', 'g_past_in0', 'g_z'], r2, r2b, r2f, r1):
        k = n if name in ('prior_mu', 'prior_var') else a.numel()
        if verbose:
            print(f'roll-out {B} x {S} under gemm_rm 2, {name}: finite {bool(torch.isfinite(a[:k]).all())} | bitwise: second run {FC.same_bits(a[:k], b[:k])}'
                  f' gemm_fold 0 {FC.same_bits(a[:k], c0[:k])} gemm_rm 1 {FC.same_bits(a[:k], d[:k])}')
        assert torch.isfinite(a[:k]).all(), name + ': words left unwritten'
        assert FC.same_bits(a[:k], b[:k]), name + ': two runs differ'
        assert FC.same_bits(a[:k], c0[:k]), name + ': gemm_fold 1 and 0 differ under gemm_rm 2'
        assert FC.same_bits(a[:k], d[:k]), name + ': gemm_rm 2 and gemm_rm 1 differ'
        assert torch.isnan(a[k:]).all(), name + ': a store went beyond sequence B'
    w64, (pm64, pv64) = RC.H.roll_out({k: v.double() for k, v in sd.items()}, past.double(), z.double())
    e_m = (r2[1][:n].double().reshape(B, S, 48) - pm64).abs().max().item()
    e_v = ((r2[2][:n].double().reshape(B, S, 48) - pv64).abs() / pv64.abs().clamp(min=1.0)).max().item()
    if verbose:
        print(f'roll-out {B} x {S} under gemm_rm 2 against fp64: prior_mu {e_m:.3e} prior_var {e_v:.3e}')
    assert e_m < RC.FWD_TOL and e_v < RC.FWD_TOL


# ------------------------------------------------------------------------------------------------------------------------------------
# input gradient of a GroupNorm + ReLU network at a flat bar, with the reference's ReLU kinks decided on the reference side
# ------------------------------------------------------------------------------------------------------------------------------------
KINK_TAU = 4e-6      # rollout_checks.kink_aware_grad_check's floor: a GroupNorm output (O(1), behind a K = 1024 fp32 product) this close to zero has
                     # no sign an fp32 evaluation could be held to -- its rounding error alone is a few 1e-7 to 1e-6


def gn_relu_grad64(lin, gns, x, w, force=None, tau=KINK_TAU):
    """fp64 forward and input gradient of sum(y * w) like gemm_split_checks.reference (GroupNorm(16) + ReLU), plus the units whose GroupNorm
    output lies within tau of the kink [(layer, row, channel)].  force: {(layer, row, channel): bool} puts those units on / off."""
    x = x.double().requires_grad_(True)
    h, near = x, []
    for i, (W, b) in enumerate(lin):
        h = h @ W.double().t() + b.double()
        if i + 1 < len(lin):
            y = torch.nn.functional.group_norm(h, 16, gns[i][0].double(), gns[i][1].double(), eps=1e-5)
            mask = y > 0
            near += [(i, r, c) for r, c in (y.detach().abs() < tau).nonzero().tolist()]
            for (l, r, c), on in (force or {}).items():
                if l == i:
                    mask[r, c] = on
            h = y * mask.to(y.dtype)
    gx = torch.autograd.grad((h * w.double()).sum(), x)[0]
    return h.detach(), gx, near


def assert_grad_kink_aware(lin, gns, x, w, gx, tol, what, max_units=6, verbose=True):
    """Every row of gx within tol x max(1, |reference|_max) of the fp64 gradient.  The derivative of ReLU does not exist at 0: a row that misses
    the bar on the reference's own branch passes only if the REFERENCE has units within KINK_TAU of their kink in that row (at most max_units)
    and the kernel's gradient meets the same bar for one on / off assignment of exactly those units.  Rows are independent."""
    import itertools
    y64, gx64, near = gn_relu_grad64(lin, gns, x, w)
    s = max(1.0, gx64.abs().max().item())
    e = (gx.double() - gx64).abs().amax(1) / s
    moved = []
    for r in (e > tol).nonzero().flatten().tolist():
        units = [(l, c) for l, rr, c in near if rr == r]
        assert 0 < len(units) <= max_units, f'{what}: row {r} is {e[r].item():.3e} from the reference and has {len(units)} units within {KINK_TAU} of a ReLU kink'
        best = None
        for bits_ in itertools.product((False, True), repeat=len(units)):
            _, g1, _ = gn_relu_grad64(lin, gns, x[r:r + 1], w[r:r + 1], force={(l, 0, c): on for (l, c), on in zip(units, bits_)})
            e1 = (gx[r:r + 1].double() - g1).abs().max().item() / s
            best = e1 if best is None else min(best, e1)
        moved.append((r, len(units), e[r].item(), best))
        assert best <= tol, f'{what}: row {r} is {e[r].item():.3e} from the reference, {best:.3e} on the closest branch of its {len(units)} kink units'
    if verbose and moved:
        print(f'{what}: rows judged on another ReLU branch of the reference (row, units at the kink, error on the natural branch, on the closest): {moved}')
    return max([e[r].item() for r in range(len(e)) if e[r] <= tol] + [m[3] for m in moved])


# ------------------------------------------------------------------------------------------------------------------------------------
# the policy's documented decisions (the sixteen GEMM launches of one 32 x 60 evaluation; RM 2 at C5 size)
# ------------------------------------------------------------------------------------------------------------------------------------
VPOSER_DEC, VPOSER_ENC = (32, 512, 512, 126), (63, 512, 512, 32)
SIXTEEN = [
    # (network, act, rows, direction, forms in launch order)
    (VPOSER_DEC, LR, 32, 'bwd', [111, 141, 141]),       # VPoser adjoint 126 -> 512, 512 -> 512, 512 -> 32
    (VPOSER_DEC, LR, 32, 'fwd', [111, 141, 141]),       # VPoser decode 32 -> 512, 512 -> 512, 512 -> 126
    (PRIOR_DIMS, GN, 1888, 'fwd', [112, 112, 112, 112, 141]),
    (PRIOR_DIMS, GN, 1888, 'bwd', [112, 112, 112, 112, 122]),
]


def check_policy(lib):
    with knobs(lib):
        for dims, act, N, d, want in SIXTEEN:
            got = [fm for fm, _ in forms(lib, dims, act, N, d)]
            assert got == want, f'{dims} at {N} rows, {d}: DESIGN.md section 7 lists {want}, plan_prior_gemm gives {got}'
        assert sum(len(s[4]) for s in SIXTEEN) == 16
        # RM 2 at C5 size (256 sequences: 8 x 119 = 952 row tiles of the prior, 30 720 frames = 960 of VPoser) for every launch of two or
        # more column blocks of 256; a launch of ONE column block (96, 126 or 32 columns) reaches (row tiles / 2) x column blocks >= 512
        # only from 1024 row tiles on and stays in the plain form, pinned
        for dims, act, nrt in ((PRIOR_DIMS, GN, 952), (VPOSER_DEC, LR, 960), (VPOSER_ENC, LR, 960)):
            for q in launches(dims, act, 32 * nrt):
                ncb = -(-q[0] // 8)
                want = 212 if ncb >= 2 else 112
                assert form(lib, *q) == want, f'{dims} launch {q}: expected {want}, plan_prior_gemm gives {form(lib, *q)}'
                thr = 2 * -(-512 // ncb)         # the first row-tile count with (nrt / 2) x ncb >= 512
                assert plan(lib, q[0], q[1], thr, q[3])[0] == 2 and plan(lib, q[0], q[1], thr - 1, q[3])[0] == 1, (dims, q, thr)
        # the thresholds the text names: VPoser's hidden layers from 16 384 rows on, the 1024-wide products from 8 192
        assert plan(lib, 16, 8, 512, 4)[0] == 2 and plan(lib, 16, 8, 511, 4)[0] == 1
        assert plan(lib, 32, 16, 256, 1)[0] == 2 and plan(lib, 32, 16, 255, 1)[0] == 1
    # the knobs override the size rule
    with knobs(lib, rm=1):
        assert plan(lib, 32, 16, 952, 1)[0] == 1
    with knobs(lib, rm=2):
        assert plan(lib, 1, 1, 1, 0)[:3] == (2, 1, 2)


def assert_launch_unsplit_agrees(lib, dims, act, N):
    """gemm_split_checks.launch_unsplit restates rules (b) / (c) of the policy in Python; here it is held to the hook on every launch of the
    network it is asked about (gemm_split_checks.check_net calls this): unsplit <=> KS 1 under the default knobs."""
    with knobs(lib):
        nrt = -(-N // 32)
        for l in range(len(dims) - 1):
            for K, n_out, epi in ((dims[l], dims[l + 1], 0 if l + 2 == len(dims) else (4 if act == LR else 1)),
                                  (dims[l + 1], dims[l], 0 if l == 0 else (5 if act == LR else 3))):
                ks = plan(lib, -(-n_out // 32), -(-K // 64), nrt, epi)[1]
                assert GC.launch_unsplit(K, n_out, nrt) == (ks == 1), \
                    f'launch_unsplit({K}, {n_out}, {nrt}) = {GC.launch_unsplit(K, n_out, nrt)}, plan_prior_gemm gives KS {ks} ({dims} {act} epilogue {epi})'


def check_launch_unsplit_agrees(lib, rows=(32, 33, 45, 1888)):
    """... at every size the tiers call check_net with (32 / 33 rows on the emulator, 32 / 1888 on the GPU) without running a network."""
    for dims, act in GC.NETS:
        for N in rows:
            assert_launch_unsplit_agrees(lib, dims, act, N)
