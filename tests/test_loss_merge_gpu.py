"""GPU tier: the merged loss-side launches (ha_tune_set "loss_merge", default 1) against the one-launch-per-kernel form (0), bit for bit, and
against the references of the fit tests at their tolerances.  Allocations are poisoned (conftest), so an output a merged launch leaves
unwritten shows as NaN."""
import pytest
import torch

import fitloss_checks as FL
import fitting_checks as FC
import loss_merge_checks as LM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('B,T', LM.FIT_SHAPES)
@pytest.mark.parametrize('K', [1, 12])
def test_fit_loss_with_mixture_merged_equals_separate(gpu_lib, dev, B, T, K):
    print('worst relative gradient difference', LM.check_fit_loss(gpu_lib, dev, B, T, K, 'motion', seed=B + T))


@pytest.mark.parametrize('B,T', LM.FIT_SHAPES)
def test_fit_loss_without_mixture_merged_equals_separate(gpu_lib, dev, B, T):
    print('worst relative gradient difference', LM.check_fit_loss(gpu_lib, dev, B, T, 12, 'smpl', seed=B))


@pytest.mark.parametrize('kind', ['motion', 'smpl'])
def test_fit_loss_beyond_one_group_of_chunks(gpu_lib, dev, kind):
    LM.check_long_reduction(gpu_lib, dev, *LM.LONG_SHAPE)
    print('worst relative gradient difference', LM.check_fit_loss(gpu_lib, dev, *LM.LONG_SHAPE, 12, kind, seed=1))


def test_fit_loss_halo_and_standard_normal_prior(gpu_lib, dev):
    LM.check_fit_loss(gpu_lib, dev, 3, 5, 12, 'motion', halo=True, seed=2)
    LM.check_fit_loss(gpu_lib, dev, 3, 5, 12, 'motion', cond=False, seed=3)


@pytest.mark.parametrize('B,T', LM.POST_SHAPES)
@pytest.mark.parametrize('cam', [True, False])
def test_post_reduction_with_row_sum_merged_equals_separate(gpu_lib, dev, B, T, cam):
    for add1, add2 in ((True, True), (True, False), (False, False)):
        LM.check_post_backward(gpu_lib, dev, B, T, cam, add1, add2, seed=T)
    print('op chain: worst relative gradient difference', FL.check_rollout_post(gpu_lib, dev, B=B, S=T - 1, seed=T, cam=cam))


def test_stage3_closure_merged_equals_separate(gpu_lib, dev, smplh_npz):
    """MotionOptimizer's stage-3 closure at 2 x 8, eager and under hipGraph replay, with the variables changing in place between the
    evaluations: the loss and all nine gradients at loss_merge = 1 equal those at 0 bit for bit."""
    from oracle import closure_cases as CC
    B, T, reps = 2, 8, 2
    case = CC.make_case('rgb', B, T, seed=1)
    res = {}
    with LM.both_settings(gpu_lib) as settings:
        for merge in settings:
            for graphs in (False, True):
                opt = FC.build(gpu_lib, dev, 'rgb', B, T, smplh_npz)
                opt.use_graphs = graphs
                var = {k: v.clone().to(dev) for k, v in case['var'].items()}
                obs = {k: v.clone().to(dev) for k, v in case['obs'].items()}
                opt.fitting_loss.set_stage(2)
                opt.trans, opt.root_orient, opt.latent_pose = (var[k][:, :1].clone().requires_grad_(True) for k in ('trans', 'root_orient', 'latent_pose'))
                opt.betas = var['betas'].requires_grad_(True)
                opt.latent_motion = var['latent_motion'].requires_grad_(True)
                opt.trans_vel, opt.joints_vel, opt.root_orient_vel = (var[k].requires_grad_(True) for k in ('trans_vel', 'joints_vel', 'root_orient_vel'))
                opt.floor_plane = var['floor_plane'].requires_grad_(True)
                prior = [opt.trans_vel, opt.joints_vel, opt.root_orient_vel]
                params = [opt.trans, opt.root_orient, opt.latent_pose, opt.betas, opt.latent_motion] + prior + [opt.floor_plane]
                ol = opt._local_obs(obs)
                closure = opt.make_closure(lambda: opt._stage3_objective(ol, None, prior, False, 15, 1.0, 200.0, True, 'neutral'), params, None)
                out = []
                for _ in range(reps):
                    loss = closure()
                    out.append((loss.detach().clone(), [p.grad.clone() for p in params]))
                    with torch.no_grad():
                        opt.latent_motion.add_(0.01)
                        for p in params:
                            p.mul_(1.0 + 2.0 ** -20)
                    torch.cuda.synchronize()
                res[merge, graphs] = out
    for graphs in (False, True):
        for (l1, g1), (l0, g0) in zip(res[1, graphs], res[0, graphs]):
            assert bool(torch.isfinite(l1)) and LM.bits_equal(l1, l0), (graphs, l1.item(), l0.item())
            assert len(g1) == len(g0) == 9
            for i, (a, b) in enumerate(zip(g1, g0)):
                assert bool(torch.isfinite(a).all()) and LM.bits_equal(a, b), (graphs, i)
