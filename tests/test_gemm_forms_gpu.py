"""GPU tier of the batched GEMM's forms x epilogues (tests/gemm_forms_checks.py): the whole case table on the gfx950 build, and the sizes at
which plan_prior_gemm ITSELF picks two row tiles per wave -- VPoser at 30 720 / 16 400 frames, the posterior encoder at 30 464 / 8 200 rows,
the 256 x 120 stage-3 closure -- against fp64 on a row subset and, bit for bit on every row, against the same call under gemm_rm 1."""
import copy

import pytest
import torch

import fitting_checks as FIT
import gemm_fold_checks as FC
import gemm_forms_checks as GF
import mlp_checks as MC
import rollout_checks as RC
from humor_amd import mlp as M
from humor_amd import synth
from oracle import humor_restated as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('c', GF.CASES, ids=lambda c: c['name'])
def test_gemm_form_against_fp64(gpu_lib, dev, c):
    GF.check_case(gpu_lib, dev, c)


@pytest.mark.parametrize('B,S', [(5, 3), (70, 3)])
def test_gemm_rm2_prior_shaped_store(gpu_lib, dev, B, S):
    """mean | exp(log-variance) over S steps behind RM 2 (70 x 3: three row tiles per step, a row group of two tiles straddles a step
    boundary), behind the persistent (B <= 32) and the pipelined roll-out."""
    GF.check_rollout_case(gpu_lib, dev, B, S, seed=B + S)


def test_gemm_rm2_prior_shaped_store_launch_chain(gpu_lib, dev):
    gpu_lib.call('ha_tune_set', b'rollout_persist', 0)
    try:
        GF.check_rollout_case(gpu_lib, dev, 70, 3, seed=11)
    finally:
        gpu_lib.call('ha_tune_set', b'rollout_persist', 1)


def test_gemm_policy_documented_decisions(gpu_lib):
    """The gfx950 build answers the plan query like the emulator build (same source): DESIGN.md section 7's forms, RM 2 at C5 size."""
    GF.check_policy(gpu_lib)
    GF.check_launch_unsplit_agrees(gpu_lib)


# ------------------------------------------------------------------------------------------------------------------------------------
# the sizes at which the policy picks RM 2
# ------------------------------------------------------------------------------------------------------------------------------------
def subset(N):
    """Rows judged against fp64 (rows are independent): the first tile, the last two tiles, every 97th row."""
    nrt = -(-N // 32)
    return torch.tensor(sorted(set(range(32)) | set(range((nrt - 2) * 32, N)) | set(range(0, N, 97))))


def three_runs(lib, fn):
    """fn() under the default knobs, under gemm_ks 0 (the policy's RM, no K split) and under gemm_rm 1 + gemm_ks 0 (the plain form)."""
    out = []
    for rm, ks in ((0, 2), (0, 0), (1, 0)):
        with GF.knobs(lib, rm, ks, 1):
            out.append(fn())
    return out


def hidden_forms(lib, dims, act, N):
    """Forms of the launches that produce a hidden-width output (forward layers but the last, adjoint launches but the first layer's)."""
    n = len(dims) - 1
    fm = [f for f, _ in GF.forms(lib, dims, act, N)]
    return fm[:n - 1] + fm[n:2 * n - 1]


@pytest.mark.parametrize('N', [30720, 16400])
def test_vposer_rows_where_the_policy_picks_rm2(gpu_lib, dev, N):
    """RealShapedVPoser decode (6-D tail) and encode through FusedVPoser at 960 row tiles, and at 513 (odd, 16 live rows in the last)."""
    vp = MC.RealShapedVPoser(3).eval()
    fv = M.FusedVPoser(vp, gpu_lib, 0)
    vp64 = copy.deepcopy(vp).double()
    g = torch.Generator().manual_seed(N)
    z, wz = torch.randn(N, vp.latentD, generator=g), torch.randn(N, 63, generator=g)
    p, wp = 0.4 * torch.randn(N, 63, generator=g), torch.randn(N, vp.latentD, generator=g)
    for dims in (GF.VPOSER_DEC, GF.VPOSER_ENC):
        with GF.knobs(gpu_lib):
            hf = hidden_forms(gpu_lib, dims, GF.LR, N)
        assert hf == [212] * 4, f'{dims} at {N} rows: the hidden layers were expected in the RM 2 form, plan_prior_gemm gives {hf}'
        with GF.knobs(gpu_lib, 1, 0):
            assert hidden_forms(gpu_lib, dims, GF.LR, N) == [112] * 4

    def run(f, x, w):
        def once():
            xd = x.to(dev).requires_grad_(True)
            y = f(xd)
            gx = torch.autograd.grad((y * w.to(dev)).sum(), xd)[0]
            return y.detach().cpu(), gx.cpu()
        return three_runs(gpu_lib, once)

    rows = subset(N)
    for name, f, f64, x, w, tol in (('decode', fv.decode_aa, lambda t: H.rot_to_aa(vp64.decode(t).reshape(-1, 3, 3)).reshape(t.shape[0], -1), z, wz, (2e-5, 1e-4)),
                                    ('encode', fv.encode_mean, lambda t: vp64.encode(t).mean, p, wp, (2e-5, 1e-4))):
        (y, gx), (y_k0, gx_k0), (y_r1, gx_r1) = run(f, x, w)
        xs = x[rows].double().requires_grad_(True)
        y64 = f64(xs)
        gx64 = torch.autograd.grad((y64 * w[rows].double()).sum(), xs)[0]
        y64 = y64.detach()
        e = [(a[rows].double() - r).abs().max().item() for a, r in ((y, y64), (gx, gx64), (y_k0, y64), (gx_k0, gx64))]
        print(f'VPoser {name} N={N}: against fp64 on {len(rows)} rows  y {e[0]:.3e} g {e[1]:.3e} (gemm_ks 0: {e[2]:.3e} {e[3]:.3e}; scales {y64.abs().max().item():.3g} '
              f'{gx64.abs().max().item():.3g}) | RM 2 bitwise equal to RM 1: y {FC.same_bits(y_k0, y_r1)} g {FC.same_bits(gx_k0, gx_r1)}')
        assert torch.isfinite(y).all() and torch.isfinite(gx).all()
        for a, ga in ((y, gx), (y_k0, gx_k0)):
            MC._cmp(a[rows], y64, tol[0], f'{name} N={N}')
            MC._cmp(ga[rows], gx64, tol[1], f'{name} grad N={N}')
        assert FC.same_bits(y_k0, y_r1), f'{name}: RM 2 and RM 1 differ'
        assert FC.same_bits(gx_k0, gx_r1), f'{name} grad: RM 2 and RM 1 differ'


@pytest.mark.parametrize('N', [30464, 8200])
def test_posterior_rows_where_the_policy_picks_rm2(gpu_lib, dev, N):
    """HuMoR's posterior encoder (678 -> 4 x 1024 -> 96, GroupNorm groups of 64) through humor_mlp at 952 row tiles, and at 257 (odd, 8 live
    rows in the last)."""
    hm, _ = RC.make_model(None, torch.device('cpu'), seed=1, contractive=True)
    enc = hm.encoder
    f = M.humor_mlp(gpu_lib, 0, enc)
    enc64 = copy.deepcopy(enc).double()
    dims = (678, 1024, 1024, 1024, 1024, 96)
    with GF.knobs(gpu_lib):
        hf = hidden_forms(gpu_lib, dims, GF.GN, N)
    assert hf == [212] * 8, f'posterior encoder at {N} rows: the hidden layers were expected in the RM 2 form, plan_prior_gemm gives {hf}'
    g = torch.Generator().manual_seed(N)
    x = torch.cat([RC.canonical_state(N, g), RC.canonical_state(N, g)], 1)
    w = torch.randn(N, 96, generator=g)

    def once():
        xd = x.to(dev).requires_grad_(True)
        y = f(xd)
        gx = torch.autograd.grad((y * w.to(dev)).sum(), xd)[0]
        return y.detach().cpu(), gx.cpu()
    (y, gx), (y_k0, gx_k0), (y_r1, gx_r1) = three_runs(gpu_lib, once)
    rows = subset(N)
    xs = x[rows].double().requires_grad_(True)
    y64 = enc64(xs)
    gx64 = torch.autograd.grad((y64 * w[rows].double()).sum(), xs)[0]
    y64 = y64.detach()
    e = [(a[rows].double() - r).abs().max().item() for a, r in ((y, y64), (gx, gx64), (y_k0, y64), (gx_k0, gx64))]
    print(f'posterior encoder N={N}: against fp64 on {len(rows)} rows  y {e[0]:.3e} g {e[1]:.3e} (gemm_ks 0: {e[2]:.3e} {e[3]:.3e}; scales {y64.abs().max().item():.3g} '
          f'{gx64.abs().max().item():.3g}) | RM 2 bitwise equal to RM 1: y {FC.same_bits(y_k0, y_r1)} g {FC.same_bits(gx_k0, gx_r1)}')
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    # The gradient is held to the flat bar on every judged row; 409 rows x 4096 ReLU units have a few GroupNorm outputs within fp32 rounding of
    # zero (at 30 464 rows: unit 571 of the second layer in row 4365 is -4.6e-7 in fp64, and the reference's own gradient of that row moves by
    # 4.4e-3 with the unit's branch), so a row that misses it must meet it on another branch of exactly such units, decided on the reference side
    lin, gns, _ = enc.describe()
    lin, gns = [(l.weight.detach(), l.bias.detach()) for l in lin], [(n.weight.detach(), n.bias.detach()) for n in gns]
    y64b, gx64b, _ = GF.gn_relu_grad64(lin, gns, x[rows], w[rows])
    assert (y64b - y64).abs().max().item() < 1e-12 and (gx64b - gx64).abs().max().item() < 1e-12, 'the restated fp64 network is not the module'
    for a, ga in ((y, gx), (y_k0, gx_k0)):
        MC._cmp(a[rows], y64, 1e-4, f'posterior N={N}')
        worst = GF.assert_grad_kink_aware(lin, gns, x[rows], w[rows], ga[rows], 1e-3, f'posterior grad N={N}')
        print(f'posterior encoder N={N}: gradient against fp64, every row on a branch the reference cannot tell apart: {worst:.3e}')
    assert FC.same_bits(y_k0, y_r1), 'posterior: RM 2 and RM 1 differ'
    assert FC.same_bits(gx_k0, gx_r1), 'posterior grad: RM 2 and RM 1 differ'


def test_stage3_closure_256x120_rm2_equals_rm1(gpu_lib, dev, smplh_npz):
    """The C5-size stage-3 objective (256 sub-sequences of 120 frames: the prior at 952 row tiles, VPoser at 960) under gemm_ks 0 with the
    policy's RM 2 and with gemm_rm 1: loss and every gradient finite and bit for bit the same, no error word from the persistent roll-out."""
    from oracle import closure_cases as CC
    B, T = 256, 120
    case = CC.make_case('rgb', B, T, seed=5)
    with GF.knobs(gpu_lib, 0, 0):
        assert [f for f, _ in GF.forms(gpu_lib, GF.PRIOR_DIMS, GF.GN, 32 * 952)] == [212] * 4 + [112] + [212] * 5
    res = {}
    for rm in (0, 1):
        with GF.knobs(gpu_lib, rm, 0):
            opt = FIT.build(gpu_lib, dev, 'rgb', B, T, smplh_npz, state_dict=synth.contractive_state_dict(0))
            res[rm] = {k: v.detach().cpu().clone() for k, v in FIT.eval_stage(opt, case, 2, dev).items()}
            av, err, _ = opt.motion_prior.persistent_rollout_status(dev)
            assert err == 0, (av, hex(err))
        del opt
    print('256 x 120 stage-3 closure: loss', res[0]['loss'].item(), '| bitwise equal under gemm_rm 1:',
          {k: FC.same_bits(res[0][k], res[1][k]) for k in res[0]})
    for k in res[0]:
        assert torch.isfinite(res[0][k]).all(), k
        assert FC.same_bits(res[0][k], res[1][k]), f'{k}: RM 2 and RM 1 differ'
