"""GPU tier: the points3d op (csrc/points_fit.hip) against the CPU yardstick of points_fit_checks.py, through FittingLoss against the
unfused op chain at the dense body's size, and inside a captured closure."""
import pytest
import torch

import points_fit_checks as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (3, 5, 257, 1030), (2, 2, 64, 1), (1, 2, 130, 3), (1, 1, 2600, 5)])
def test_op_matches_yardstick(gpu_lib, dev, shape):
    """N = 1; N odd with V across the 1024-candidate LDS chunk and a ragged tail; up to 64 lanes of one wave on the same vertex
    (ordered in-wave accumulation over multiplicities 1 .. 64 and over wave steps); more observations per frame than five staged groups of
    the backward (512 each) with a ragged sixth, and N past one four-key trip of the select passes (2048) with a ragged tail."""
    PC.check_case(gpu_lib, dev, *PC.make_case(*shape, seed=sum(shape)))


def test_ties_and_zero_distance(gpu_lib, dev):
    PC.check_zero_distance_gradient(gpu_lib, dev)


def test_mad_zero(gpu_lib, dev):
    PC.check_mad_zero(gpu_lib, dev)


def test_narrow_range(gpu_lib, dev):
    PC.check_narrow_range(gpu_lib, dev)


def test_nan_sequence(gpu_lib, dev):
    PC.check_nan_sequence(gpu_lib, dev)


def test_no_robust_weights(gpu_lib, dev):
    PC.check_none(gpu_lib, dev)


def test_determinism_at_the_dense_body_size(gpu_lib, dev):
    PC.check_determinism(gpu_lib, dev, (2, 3, 700, 6890))


def test_fallbacks(gpu_lib, dev, monkeypatch):
    PC.check_fallbacks(gpu_lib, dev, monkeypatch)


# --------------------------------------------------------------------------------------------------------------------------------
# the dense synthetic SMPL+H body (V = 6890) through MotionOptimizer / FittingLoss
# --------------------------------------------------------------------------------------------------------------------------------
WEIGHTS_ALL = {'joints3d': 1.0, 'verts3d': 1.0, 'joints3d_smooth': 0.1, 'points3d': 1.0}


def _optimizer(dev, smplh_npz, B, T, weights, robust='bisquare', **kw):
    from humor_amd import synth
    from humor_amd.body_model import BodyModel
    from humor_amd.configs import stage_weights
    from humor_amd.humor_model import HumorModel
    from humor_amd.motion_optimizer import MotionOptimizer
    bm = BodyModel(smplh_npz, num_betas=16, batch_size=B * T, use_vtx_selector=False)
    hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', latent_size=48, model_data_config='smpl+joints+contacts', steps_in=1)
    hm.load_state_dict(synth.humor_state_dict(seed=0))
    hm = hm.to(dev).eval()
    w, mu, cov = synth.make_gmm(seed=0)
    opt = MotionOptimizer(dev, bm, 16, B, T, ['points3d'], stage_weights([weights] * 3), synth.SynthVPoser(seed=0).to(dev).eval(), hm,
                          {'gmm': (w.to(dev), mu.to(dev), cov.to(dev))}, robust_loss_type=robust, use_chamfer=True, **kw)
    g = torch.Generator().manual_seed(0)
    opt.trans = (0.1 * torch.randn(B, T, 3, generator=g)).to(dev).requires_grad_(True)
    opt.root_orient = (torch.tensor([0.3, 0.1, -0.2]) + 0.1 * torch.randn(B, T, 3, generator=g)).to(dev).requires_grad_(True)
    return opt


def _observations(opt, dev, B, T, n_obs, seed=1):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        pred, _ = opt.smpl_results(opt.trans, opt.root_orient, opt.latent2pose(opt.latent_pose), opt.betas)
    pick = torch.randint(0, 6890, (B, T, n_obs), generator=g).to(dev)
    noise = lambda ref, s: ref + s * torch.randn(ref.shape, generator=g).to(dev)
    cloud = noise(torch.gather(pred['points3d'], 2, pick.unsqueeze(-1).expand(B, T, n_obs, 3)), 0.02)      # (no query on a vertex)
    return {'points3d': cloud, 'joints3d': noise(pred['joints3d'], 0.05), 'verts3d': noise(pred['verts3d'], 0.05)}, pred


@pytest.fixture(scope='module')
def body(gpu_lib, dev, smplh_npz):
    B, T, n_obs = 2, 2, 700
    opt = _optimizer(dev, smplh_npz, B, T, WEIGHTS_ALL)
    obs, pred = _observations(opt, dev, B, T, n_obs)
    return opt, obs, pred


@pytest.mark.parametrize('robust', ['bisquare', 'none'])
def test_dense_body_matches_yardstick(gpu_lib, dev, body, robust):
    opt, obs, pred = body
    PC.check_case(gpu_lib, dev, obs['points3d'].cpu(), pred['points3d'].cpu().contiguous(), robust)


@pytest.mark.parametrize('robust', ['none', 'bisquare'])
@pytest.mark.parametrize('kind', ['root', 'smpl'])
def test_dense_body_objective_equals_unfused_chain(gpu_lib, dev, body, kind, robust):
    """joints3d, verts3d, joints3d_smooth and points3d all weighted: the op as an addend of the fused loss kernel against the term-by-term
    evaluation with the chamfer / median op chain (fused_points=False).  Loss to 1e-5 relative (the bar of that path), gradients w.r.t.
    trans / root_orient to 1e-4 of their largest entry (the project's flat gradient bar)."""
    opt, obs, _ = body
    fl = opt.fitting_loss
    res = []
    try:
        fl.robust_loss = robust
        for fp in (True, False):
            fl.fused_points = fp
            pred, _ = opt.smpl_results(opt.trans, opt.root_orient, opt.latent2pose(opt.latent_pose), opt.betas)
            loss, stats = fl.root_fit(obs, pred) if kind == 'root' else fl.smpl_fit(obs, pred, opt.seq_len)
            assert 'points3d' in stats and 'joints3d' in stats and 'verts3d' in stats and (kind == 'root' or 'joints3d_smooth' in stats)
            res.append((loss.item(), torch.autograd.grad(loss, [opt.trans, opt.root_orient])))
    finally:
        fl.robust_loss, fl.fused_points = 'bisquare', True
    (l1, g1), (l0, g0) = res
    print(kind, robust, 'loss', l1, l0)
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l1, l0)
    for a, b, name in zip(g1, g0, ('trans', 'root_orient')):
        e, top = (a - b).abs().max().item(), b.abs().max().item()
        print(kind, robust, name, 'max abs diff', e, 'largest entry', top)
        assert e <= 1e-4 * top, (name, e, top)


def test_points_only_objective_skips_the_fused_kernel(gpu_lib, dev, body, monkeypatch):
    from humor_amd import fit_kernels as FK
    from humor_amd.configs import stage_weights
    opt, obs, _ = body
    fl = opt.fitting_loss
    saved = fl.all_stage_loss_weights
    try:
        fl.all_stage_loss_weights = stage_weights([{'points3d': 1.0}] * 3)
        fl.set_stage(0)
        pred, _ = opt.smpl_results(opt.trans, opt.root_orient, opt.latent2pose(opt.latent_pose), opt.betas)
        with monkeypatch.context() as m:
            m.setattr(FK.FusedFit, 'apply', lambda *a, **k: pytest.fail('FusedFit launched for a points3d-only objective'))
            loss, stats = fl.root_fit(obs, pred)
        assert set(stats) == {'points3d'} and torch.isfinite(loss)
        fl.fused_points = False
        loss0, _ = fl.root_fit(obs, pred)
        assert abs(loss.item() - loss0.item()) <= 1e-5 * abs(loss0.item())
    finally:
        fl.all_stage_loss_weights, fl.fused_points = saved, True
        fl.set_stage(0)


def test_graphed_points_closure_equals_eager(gpu_lib, dev, smplh_npz):
    """The stage-1 closure of a point-cloud fit captured into a hipGraph and replayed twice against eager evaluation: the op makes no
    host reads, and since it is deterministic the loss and the gradients are the same bits."""
    B, T, n_obs = 2, 3, 70
    res = {}
    for graphs in (False, True):
        opt = _optimizer(dev, smplh_npz, B, T, {'points3d': 1.0}, use_graphs=graphs)
        obs, _ = _observations(opt, dev, B, T, n_obs)
        obs = {'points3d': obs['points3d']}
        opt.fitting_loss.set_stage(0)
        params = [opt.trans, opt.root_orient]
        ol = opt._local_obs(obs)
        closure = opt.make_closure(lambda: opt._stage1_objective(ol, False), params)
        out = []
        for _ in range(2):
            loss = closure()
            out.append((loss.detach().clone(), [p.grad.clone() for p in params]))
        torch.cuda.synchronize()
        assert getattr(opt, 'graph_failures', 0) == 0
        res[graphs] = out
    for (l0, g0), (l1, g1) in zip(res[False], res[True]):
        assert torch.isfinite(l0) and torch.equal(l0, l1), (l0, l1)
        for a, b in zip(g0, g1):
            assert torch.equal(a, b), (a - b).abs().max()
