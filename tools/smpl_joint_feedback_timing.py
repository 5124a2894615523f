"""One sampled roll-out of B sequences x S steps, with or without SMPL-joint feedback (HumorModel(model_use_smpl_joint_inputs=True,
smplh_path=...).roll_out(gender=, betas=)), timed with device events.  Both modes run the launch chain (ha_humor_rollout_sample /
ha_humor_rollout_smpl_joints); under `rocprofv3 --kernel-trace --stats` the kernel statistics give the launches per step of each mode
(calls / (roll-outs x S)) and the average time of the glue kernel (glue_fwd_kernel<3, true> / glue_fwd_fb_kernel).

    python tools/smpl_joint_feedback_timing.py --batch 1 --steps 300 --feedback 1 [--reps 5]

--grad 1: the given-z roll-out forward + backward instead (what a stage-3 closure spends in the motion prior), in ONE process for both the
plain prior on the launch chain (ha_tune_set rollout_persist 0: glue_fwd_kernel<3, true> / glue_bwd_kernel<3, true>) and the feedback prior
built with smpl_joint_gradients=True (glue_fwd_fb_kernel / glue_bwd_fb_kernel), so that one kernel trace holds all four glue kernels:

    python tools/smpl_joint_feedback_timing.py --batch 32 --steps 59 --grad 1 [--reps 10]

Synthetic body models and weights (humor_amd.synth), written to a temporary directory.
"""
import argparse
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from humor_amd import synth                          # noqa: E402
from humor_amd.humor_model import HumorModel         # noqa: E402

GENDERS = ['male', 'female', 'neutral']


def canonical_state(B, gen):
    from humor_amd.frames import _rodrigues_torch
    r = lambda *s: torch.randn(*s, generator=gen)
    trans = torch.cat([torch.zeros(B, 2), 0.9 + 0.1 * r(B, 1)], 1)
    R_root = _rodrigues_torch(0.3 * r(B, 3)).reshape(B, 9)
    R_body = _rodrigues_torch(0.3 * r(B * 21, 3)).reshape(B, 189)
    joints = 0.3 * r(B, 66)
    joints[:, :2] = 0
    return torch.cat([trans, 0.3 * r(B, 3), R_root, 0.3 * r(B, 3), R_body, joints, 0.3 * r(B, 66)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--feedback', type=int, default=1)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--grad', type=int, default=0)
    a = ap.parse_args()
    if a.grad:
        return main_grad(a)
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    B, S = a.batch, a.steps
    with tempfile.TemporaryDirectory() as td:
        kw = {}
        if a.feedback:
            for i, g in enumerate(GENDERS):
                os.makedirs(os.path.join(td, g))
                synth.write_smplh_npz(os.path.join(td, g, 'model.npz'), seed=i)
            kw = dict(model_use_smpl_joint_inputs=True, model_smpl_batch_size=B, smplh_path=td)
        hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', latent_size=48, model_data_config='smpl+joints+contacts', steps_in=1, **kw)
        hm.load_state_dict(synth.contractive_state_dict(0))
        hm = hm.to(dev).eval()
        gen = torch.Generator().manual_seed(0)
        past = canonical_state(B, gen).to(dev)
        eps = torch.randn(B, S, 48, generator=gen).to(dev)
        betas = (0.5 * torch.randn(B, 1, 16, generator=gen)).to(dev)
        gender = [GENDERS[i % 3] for i in range(B)]
        fb = dict(gender=gender, betas=betas) if a.feedback else {}

        def once():
            with torch.no_grad():
                return hm.roll_out(past, None, S, eps_seq=eps, return_world=True, **fb)
        world = once()                                  # warm-up: code objects, body-model upload
        torch.cuda.synchronize()
        assert torch.isfinite(world).all()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(a.reps):
            t0.record()
            once()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1))
    times.sort()
    print(f'feedback={a.feedback} B={B} S={S} roll-outs={a.reps + 1} ms per roll-out: min {times[0]:.3f} median {times[len(times) // 2]:.3f} '
          f'max {times[-1]:.3f} ({1e3 * times[len(times) // 2] / S:.2f} us per step)')


def main_grad(a):
    assert torch.cuda.is_available(), 'needs a GPU'
    from humor_amd import _lib
    dev = torch.device('cuda:0')
    B, S = a.batch, a.steps
    gen = torch.Generator().manual_seed(0)
    past = canonical_state(B, gen).to(dev).requires_grad_(True)
    z = torch.randn(B, S, 48, generator=gen).to(dev).requires_grad_(True)
    betas = (0.5 * torch.randn(B, 1, 16, generator=gen)).to(dev).requires_grad_(True)
    gw, gm = torch.randn(B, S, 348, generator=gen).to(dev), torch.randn(B, S, 48, generator=gen).to(dev)
    gender = [GENDERS[i % 3] for i in range(B)]
    _lib.get_lib().call('ha_tune_set', b'rollout_persist', 0)       # the plain prior on the launch chain, as the feedback prior always is
    with tempfile.TemporaryDirectory() as td:
        for i, g in enumerate(GENDERS):
            os.makedirs(os.path.join(td, g))
            synth.write_smplh_npz(os.path.join(td, g, 'model.npz'), seed=i)
        for feedback in (0, 1):
            kw = dict(model_use_smpl_joint_inputs=True, model_smpl_batch_size=B, smplh_path=td, smpl_joint_gradients=True) if feedback else {}
            hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', latent_size=48, model_data_config='smpl+joints+contacts', steps_in=1, **kw)
            hm.load_state_dict(synth.contractive_state_dict(0))
            hm = hm.to(dev).eval()
            for p in hm.parameters():
                p.requires_grad_(False)
            fb = dict(gender=gender, betas=betas) if feedback else {}
            wrt = [past, z] + ([betas] if feedback else [])

            def once():
                world, (pm, pv) = hm.roll_out(past, None, S, z_seq=z, return_prior=True, return_world=True, **fb)
                return torch.autograd.grad((world * gw).sum() + (pm * gm).sum() + (pv * gm).sum(), wrt)
            g = once()
            torch.cuda.synchronize()
            assert all(torch.isfinite(t).all() for t in g)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            times = []
            for _ in range(a.reps):
                t0.record()
                once()
                t1.record()
                torch.cuda.synchronize()
                times.append(t0.elapsed_time(t1))
            times.sort()
            print(f'grad feedback={feedback} B={B} S={S} evaluations={a.reps + 1} ms per forward + backward (launch chain): min {times[0]:.3f} '
                  f'median {times[len(times) // 2]:.3f} max {times[-1]:.3f}')


if __name__ == '__main__':
    main()
