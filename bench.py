#!/usr/bin/env python
"""bench.py -- headline benchmark of the HuMoR test-time-optimisation hot path on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W` (N>1 launched through torch.distributed.run, one rank
per GPU over RCCL) prints ONE JSON line from rank 0.

Workload = BASELINE.json config C4 (`metric`: batch=32 seq=60): fit_rgb_demo_use_split-shaped problem -- 2D OpenPose
keypoint observations, floor optimisation, overlapping 60-frame sub-sequences (overlap 10) with the overlap-consistency
terms, 32 sub-sequences per GPU.  With N GPUs the job is ONE video of 32*N coupled sub-sequences sharded contiguously
(weak scaling): replicated L-BFGS variables, closure evaluated on the local slice, differentiable halo all-gather for the
overlap terms and one packed all-reduce of [flat gradient | loss] per closure (humor_amd/distributed.py).

One "step" = one evaluation of the stage-3 fitting closure (objective forward + backward + gradient all-reduce): VPoser
decode, 3 SMPL evaluations (64-vertex subset kernels), HuMoR roll-out (59 steps, prior + decoder) with its adjoint, all loss terms -- the
deterministic unit of "fitting-iter/sec" (an L-BFGS outer iteration is ~25 of these).  Inputs are resident in HBM.
`value` = closure evaluations per second x (global batch / 32), i.e. aggregate 32x60-batch closure evaluations per second.
A plain run does only what `value` needs: set-up (at N=1 the one-off graph-vs-eager probe that picks the timed closure mode),
W warm-up and K timed closure evaluations, the result line.  `--dump-outputs DIR` writes what the last timed evaluation returned
to its caller -- `loss.npy` (float64) and `grad_<variable>.npy` (float32) for every optimisation variable -- for output-for-output
comparison of two builds (the inputs are seeded: identical from run to run).
With `--full` the side measurements below are taken as well (the `--no-*` options switch single ones off):
`smpl_verts_per_sec` (dense 6890-vertex SMPL forward, N=1920), the `roofline` of the streaming LBS kernel
(HIP events on the launch stream), `lbfgs` (REAL torch.optim.LBFGS outer iterations of every stage / stage-3 phase through
MotionOptimizer.run: outer iterations/s, closure evaluations per outer iteration, and the whole-fit time they imply for the
reference's 30/80/70 schedule), `strong` (N>1: the same 32-sequence job sharded over the N GPUs, next to the weak-scaling
headline), `rccl` (collective timings; at N=1 a world-size-1 RCCL group exercises the sharded code path on the one GPU) and
`cpu_baseline` (oracle restatement of the reference closure on the host cores, best of a thread-count sweep).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

B_SEQ, T_SEQ, OVERLAP = 32, 60, 10      # BASELINE.json metric: batch=32 seq=60 ; fit_rgb_demo_use_split.cfg overlap 10
HBM_PEAK_GBS = 8000.0                   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
V, J = 6890, 52
# algorithmic HBM bytes per frame of the LBS skinning kernel = read v_posed (V*12) + A (J*48), write verts (V*12)
SKIN_BYTES_PER_FRAME = V * 12 * 2 + J * 48
# HBM traffic of one ha_lbs_skin launch comes from rocprofv3 PMC passes (separate --pmc FETCH_SIZE / WRITE_SIZE runs of tools/skin_once.py
# via tools/pmc_lbs.sh, launches cycling over 4 operand sets like the timed launches here; FETCH_SIZE doubled per MI355X_MICROARCH.md
# 'HBM', WRITE_SIZE as reported; calibrated in the same passes on a device copy).  Counters cannot be read inside bench.py, so the
# summary tool leaves a machine-readable record next to its SUMMARY.txt -- profiles/<run>/traffic.json, with a fingerprint of the
# kernel's source -- and bench.py reads the newest record at run time: a record whose fingerprint no longer matches the kernel is
# reported as stale (traffic = null), never silently reused.


def lbs_kernel_fingerprint():
    """sha1 of the source text of lbs_skin_wave_kernel (humor_amd/csrc/smpl.hip): what a PMC record is valid for."""
    import hashlib
    lines = open(os.path.join(ROOT, 'humor_amd', 'csrc', 'smpl.hip')).read().split('\n')
    start = next(i for i, l in enumerate(lines) if 'void lbs_skin_wave_kernel(' in l)
    while start > 0 and not lines[start - 1].startswith('}') and lines[start - 1].strip():
        start -= 1
    end = next(i for i in range(start + 1, len(lines)) if lines[i] == '}')
    return hashlib.sha1('\n'.join(lines[start:end + 1]).encode()).hexdigest()[:16]


def pmc_traffic(frames):
    """(HBM bytes per launch at `frames` frames, source note) from the newest profiles/*/traffic.json that has this size."""
    import glob
    fp = lbs_kernel_fingerprint()
    for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', '*', 'traffic.json')), reverse=True):
        try:
            rec = json.load(open(f))
        except Exception:
            continue
        for e in rec.get('launches', []):
            if int(e.get('frames', -1)) == frames:
                rel = os.path.relpath(f, ROOT)
                if rec.get('kernel_fingerprint') != fp:
                    return None, f'STALE: {rel} was measured on another version of lbs_skin_wave_kernel (re-run tools/pmc_lbs.sh)'
                return int(e['hbm_bytes']), f'{rel}: {rec.get("how", "")}'
    return None, 'no PMC record for this size under profiles/*/traffic.json'


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--full', action='store_true', help='also take every side measurement (rooflines, scaling companions, L-BFGS profile, '
                    'RCCL figures, C5 sizes, CPU baseline + parity); a plain run times the headline closure only')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the loss and the gradients of the last timed closure evaluation as DIR/<name>.npy')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--eager', action='store_true', help='do not capture the closure into a hipGraph')
    ap.add_argument('--no-c5', action='store_true', help='skip the BASELINE C5-size (256x120) kernel rooflines appended at N=1')
    ap.add_argument('--graph', dest='auto', action='store_false', help='always replay the captured hipGraph (default at N=1: time graph replay against eager launches once and keep the faster)')
    ap.add_argument('--scaling', choices=['weak', 'strong', 'both'], default='both',
                    help='N>1: weak = 32 sub-sequences per GPU (the headline value), strong = 32 in total; both = time both')
    ap.add_argument('--no-c5-weak', action='store_true', help='skip the 32 x 120 per-GPU closure line (BASELINE config 5 shape, weak)')
    ap.add_argument('--no-lbfgs', action='store_true', help='skip the staged L-BFGS outer-iteration measurement (N=1)')
    ap.add_argument('--no-rccl-check', action='store_true', help='skip the world-size-1 RCCL self-check (N=1)')
    return ap.parse_args()


def seq_intervals(nseq, seq_len, overlap):
    s, out = 0, []
    for _ in range(nseq):
        out.append((s, s + seq_len))
        s += seq_len - overlap
    return torch.tensor(out)


def make_problem(B, T, seed, device):
    """Synthetic RGB observations for B overlapping sub-sequences + a plausible starting point for stage 3."""
    from humor_amd import synth
    g = torch.Generator().manual_seed(seed)
    root, body, trans = synth.smooth_pose_sequence(B, T, seed=seed, amp=0.25)
    root = root + torch.tensor([np.pi, 0.0, 0.0])            # camera looks down +z, body upright in the image (-y up)
    trans = torch.cat([0.3 * trans[:, :, :2], 4.0 + 0.2 * trans[:, :, 2:]], dim=2)
    xy = torch.rand(B, T, 25, 2, generator=g) * torch.tensor([1900.0, 1000.0])
    conf = torch.rand(B, T, 25, 1, generator=g)
    conf[:, :, [3, 17]] = 0.0
    obs = {'joints2d': torch.cat([xy, conf], 3).to(device),
           'floor_plane': torch.tensor([[0.0, -1.0, 0.0, -0.5]]).expand(B, 4).clone().to(device),
           'seq_interval': seq_intervals(B, T, OVERLAP).to(device)}
    init = {'trans': trans.to(device), 'root_orient': root.to(device),
            'latent_pose': (0.5 * torch.randn(B, T, 32, generator=g)).to(device),
            'betas': (0.5 * torch.randn(B, 16, generator=g)).to(device)}
    return obs, init


def loss_weights():
    from humor_amd.configs import RGB_WEIGHTS          # the per-stage weights of configs/fit_rgb_demo_use_split.cfg
    return RGB_WEIGHTS


def camera_matrix(B, device):
    from humor_amd.configs import camera_matrix as cm
    return cm(B).to(device)


def humor_weights():
    """Random-init HuMoR weights of the reference architecture, scaled to the well-conditioned regime of the parity fixtures
    (synth.contractive_state_dict: a default-init 59-step chain amplifies fp32 rounding ~1e4x, so no two fp32 evaluations -- the
    reference's included -- agree at full length).  Same shapes, same arithmetic, same timing; with these weights the `parity`
    field of the line (GPU closure vs the oracle closure at the SAME variables) is held to the flat 1e-4 / 1e-3 bars."""
    from humor_amd import synth
    return synth.contractive_state_dict(0)


def build_optimizer(dev, npz, B, shard=None, use_graphs=False, T=None):
    T = T_SEQ if T is None else T
    from humor_amd import synth
    from humor_amd.body_model import BodyModel
    from humor_amd.humor_model import HumorModel
    from humor_amd.motion_optimizer import MotionOptimizer
    bm = BodyModel(npz, num_betas=16, batch_size=B * T, use_vtx_selector=True)
    hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', latent_size=48, model_data_config='smpl+joints+contacts', steps_in=1)
    hm.load_state_dict(humor_weights())
    hm = hm.to(dev).eval()
    for p in hm.parameters():
        p.requires_grad_(False)
    w, mu, cov = synth.make_gmm(seed=0)
    return MotionOptimizer(dev, bm, 16, B, T, ['joints2d'], loss_weights(), synth.SynthVPoser(seed=0).to(dev).eval(), hm,
                           {'gmm': (w.to(dev), mu.to(dev), cov.to(dev))}, optim_floor=True, camera_matrix=camera_matrix(B, dev),
                           robust_loss_type='bisquare', joint2d_sigma=100, shard=shard, use_graphs=use_graphs)


class FitClosure:
    """Stage-3 closure of humor_amd.MotionOptimizer on this rank's share of the problem."""

    def __init__(self, dev, npz, world, rank, group, use_graphs=True, B_total=None, T=None):
        B = B_SEQ * world if B_total is None else B_total
        T = T_SEQ if T is None else T
        shard = None
        if group is not None or world > 1:
            from humor_amd.distributed import Shard
            shard = Shard(B, group)
        obs, init = make_problem(B, T, seed=100, device=dev)      # same problem on every rank (replicated variables)
        self.opt = build_optimizer(dev, npz, B, shard=shard, use_graphs=use_graphs, T=T)
        o = self.opt
        o.trans, o.root_orient, o.latent_pose, o.betas = init['trans'], init['root_orient'], init['latent_pose'], init['betas']
        o.fitting_loss.set_stage(2)
        o.floor_plane = (obs['floor_plane'][:, :3] * obs['floor_plane'][:, 3:]).clone().requires_grad_(True)
        self.params, self.prior_params = o.setup_stage3(data_fps=30)
        self.obs_local = o._local_obs(obs)
        self.og_w = o.fitting_loss.loss_weights['rgb_overlap_consist']

        # the closure exactly as MotionOptimizer.run builds it for the refine phase (whole-closure hipGraph when enabled)
        self.closure = o.make_closure(
            lambda: o._stage3_objective(self.obs_local, None, self.prior_params, False, 15, 1.0, self.og_w, True, 'neutral'),
            self.params, None)

    def step(self):
        self.last_loss = self.closure()
        return self.last_loss

    VAR_NAMES = ('latent_motion', 'betas', 'floor_plane', 'trans', 'root_orient', 'latent_pose', 'trans_vel', 'joints_vel', 'root_orient_vel')

    def outputs(self):
        """What the LAST evaluation returned to its caller (no new evaluation): the loss and every variable's gradient, on the host."""
        o = self.opt
        out = {'loss': np.asarray(float(self.last_loss.detach()), dtype=np.float64)}
        for k in self.VAR_NAMES:
            g = getattr(o, k).grad
            out['grad_' + k] = (g.detach().float().cpu().numpy() if g is not None else np.zeros(tuple(getattr(o, k).shape), np.float32))
        return out

    def snapshot(self):
        """One evaluation: the variables it was evaluated at, its loss and every gradient, on the host (parity vs the oracle)."""
        loss = float(self.step().detach())
        o = self.opt
        var = {k: getattr(o, k).detach().cpu().clone() for k in self.VAR_NAMES}
        grad = {k: (getattr(o, k).grad.detach().cpu().clone() if getattr(o, k).grad is not None else torch.zeros_like(var[k])) for k in self.VAR_NAMES}
        return {'loss': loss, 'var': var, 'grad': grad}

    def gradient_sensitivity(self, n=48, rtol=2e-4):
        """Per sub-sequence: does the GPU closure's OWN gradient move by >= rtol (relative to max(1, max|g|) of the tensor) when every
        variable is perturbed by one ulp (n random sign patterns)?  Such a sub-sequence has a ReLU(GroupNorm) unit within fp32
        rounding of its kink: no two fp32 evaluations of its gradient agree to 1e-3, whatever computes them."""
        o = self.opt
        params = [getattr(o, k) for k in self.VAR_NAMES]
        base_v = [p.detach().clone() for p in params]
        self.step()
        base_g = [(p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for p in params]
        B = params[0].shape[0]
        unstable = torch.zeros(B, dtype=torch.bool, device=params[0].device)
        gen = torch.Generator(device=params[0].device).manual_seed(11)
        for _ in range(n):
            with torch.no_grad():
                for p, v in zip(params, base_v):
                    sign = (torch.rand(v.shape, generator=gen, device=v.device) > 0.5).float() * 2 - 1
                    p.copy_(v * (1.0 + sign * 2.0 ** -23))
            self.step()
            for p, g0 in zip(params, base_g):
                g1 = p.grad if p.grad is not None else torch.zeros_like(p)
                dev = (g1 - g0).abs().reshape(B, -1).amax(dim=1) / max(1.0, g0.abs().max().item())
                unstable |= dev >= rtol
        with torch.no_grad():
            for p, v in zip(params, base_v):
                p.copy_(v)
        return unstable.cpu()


def closure_mode(args, fc):
    o = fc.opt
    graph = bool(o.use_graphs) and not getattr(o, 'graph_failures', 0)
    name = 'hipGraph replay (objective + backward captured once)' if graph else 'eager launches'
    note = getattr(fc, 'mode_note', None)
    return name + (' (%s)' % note if note else '')


def time_events(fn, iters, warm=2):
    """Average duration (ms) of fn() measured with HIP events on the current (launch) stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def skin_roofline(dev, npz, N=B_SEQ * T_SEQ, rotate=1):
    """The streaming LBS kernel alone (ha_lbs_skin) at N frames: algorithmic bytes / event-timed launch duration.
    Launched on torch's current stream, so the HIP events bracket exactly these launches.
    rotate = number of operand sets the launches cycle through.  At the metric's batch (N = 1920) one set is 159 MB read + 159 MB
    written: back-to-back launches on ONE set are partly served by the 256 MiB Infinity Cache (not an HBM figure); cycling through
    enough sets that > 256 MiB lie between two uses of a line makes every launch stream from / to HBM.  N = 30720 (C5) is
    cache-free with one set."""
    from humor_amd import _lib
    from humor_amd.body_model import BodyModel
    lib = _lib.get_lib()
    h = BodyModel(npz, num_betas=16)._handle_for(dev)
    sets = [(torch.randn(N * V * 3 + 4, device=dev), torch.randn(N, J, 12, device=dev), torch.randn(N, 3, device=dev),
             torch.empty(N, V, 3, device=dev)) for _ in range(rotate)]
    st = _lib.stream_ptr(sets[0][3])
    state = {'i': 0}

    def launch():
        vposed, A, transl, verts = sets[state['i'] % rotate]
        state['i'] += 1
        lib.call('ha_lbs_skin', h.ptr, N, _lib.ptr(vposed), _lib.ptr(A), _lib.ptr(transl), _lib.ptr(verts), st)
    # cache-free sizes: the first ~20 back-to-back launches ride a power-management transient (0.93 ms, then a hump up to 1.3 ms, then
    # a steady ~0.98 ms; tools/skin_jitter.py, profiles/r02_run20_skin_jitter.txt) -- the sustained figure is the one reported
    small = N <= 4096
    ms = time_events(launch, iters=(48 if rotate > 1 else 50) if small else 30, warm=(6 if rotate > 1 else 5) if small else 30)
    nbytes = SKIN_BYTES_PER_FRAME * N
    gbs = nbytes / (ms * 1e-3) / 1e9
    traffic, traffic_source = pmc_traffic(N)
    return {'kernel': 'lbs_skin (ha_lbs_skin)', 'bound': 'hbm', 'achieved': round(gbs, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
            'frac': round(gbs / HBM_PEAK_GBS, 4), 'traffic': traffic, 'traffic_source': traffic_source,
            'avg_launch_us': round(ms * 1e3, 2), 'operand_sets': rotate,
            'bytes_per_launch': nbytes, 'frames_per_launch': N}


def skin_ceilings(dev, npz, roof):
    """What the same bytes cost WITHOUT the skinning arithmetic, measured in the same run on the same rotating operand sets:
    (i) the kernel's own copy-only mode (ha_tune_set skin_variant 13: identical access geometry, weights still loaded, the LDS
    transposition kept, the bone gather and the blend dropped) and (ii) a plain device copy of the v_posed array (torch).  The 8 TB/s
    in `peak` is the HBM3E spec; these are what a read + write stream reaches on this box."""
    from humor_amd import _lib
    lib = _lib.get_lib()
    lib.call('ha_tune_set', b'skin_variant', 13)
    try:
        co = skin_roofline(dev, npz, rotate=roof['operand_sets'])
    finally:
        lib.call('ha_tune_set', b'skin_variant', -1)
    N = roof['frames_per_launch']
    srcs = [torch.randn(N * V * 3, device=dev) for _ in range(roof['operand_sets'])]
    dsts = [torch.empty(N * V * 3, device=dev) for _ in range(roof['operand_sets'])]
    st = {'i': 0}

    def cp():
        k = st['i'] % len(srcs)
        st['i'] += 1
        dsts[k].copy_(srcs[k])
    ms = time_events(cp, iters=48, warm=6)
    cp_gbs = 2 * N * V * 12 / (ms * 1e-3) / 1e9
    return {'kernel_copy_only_mode_gbs': co['achieved'], 'frac_of_kernel_copy_only_mode': round(roof['achieved'] / co['achieved'], 4),
            'device_copy_gbs': round(cp_gbs, 1), 'frac_of_device_copy': round(roof['achieved'] / cp_gbs, 4),
            'note': 'profiles/r04_lbs/README.txt: why the gap to the copy-only mode is the LDS return path (192 B of bone matrices per vertex), and the '
                    'weight-stationary / software-pipelined form that was tried and lost'}


def dense_smpl_ms(dev, npz):
    from humor_amd import synth
    from humor_amd.body_model import BodyModel
    N = B_SEQ * T_SEQ
    bm = BodyModel(npz, num_betas=16, use_vtx_selector=True)
    root, body, trans = synth.smooth_pose_sequence(B_SEQ, T_SEQ, seed=1)
    args = dict(root_orient=root.reshape(N, 3).to(dev), pose_body=body.reshape(N, 63).to(dev), trans=trans.reshape(N, 3).to(dev),
                betas=torch.randn(N, 16, device=dev))
    with torch.no_grad():
        ms_fwd = time_events(lambda: bm(**args), iters=10, warm=2)
    # forward + backward with a gradient on every vertex (point-cloud / mesh terms): dense MFMA adjoint behind ha_smpl_backward_dense
    gargs = {k: v.clone().requires_grad_(True) for k, v in args.items()}

    def fwd_bwd():
        for v in gargs.values():
            v.grad = None
        o = bm(**gargs)
        (o.v.sum() + o.Jtr.sum()).backward()
    return ms_fwd, time_events(fwd_bwd, iters=10, warm=2)


def rollout_c4_ms(dev):
    """HumorModel.roll_out alone at the metric's batch (32 sequences x 59 steps, prior + decoder): forward and forward + backward."""
    from humor_amd import synth
    from humor_amd.humor_model import HumorModel
    hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', latent_size=48, model_data_config='smpl+joints+contacts', steps_in=1)
    hm.load_state_dict(humor_weights())
    hm = hm.to(dev).eval()
    for p in hm.parameters():
        p.requires_grad_(False)
    S = T_SEQ - 1
    past = torch.randn(B_SEQ, 339, device=dev, requires_grad=True)
    z = torch.randn(B_SEQ, S, 48, device=dev, requires_grad=True)

    def fwd():
        with torch.no_grad():
            hm.roll_out(past, None, S, z_seq=z, return_prior=True)

    def fwd_bwd():
        past.grad = None
        z.grad = None
        out, (pm, pv) = hm.roll_out(past, None, S, z_seq=z, return_prior=True)
        (out['trans'].sum() + out['joints'].sum() + pm.sum()).backward()
    from humor_amd import _lib
    lib = _lib.get_lib()
    out = {}
    # default path (forward = ONE persistent launch, weights resident in the XCD teams' register files) and the launch chain beside it
    for name, knob in (('persistent_forward', 1), ('launch_chain', 0)):
        lib.call('ha_tune_set', b'rollout_persist', knob)
        try:
            tf, tb = time_events(fwd, iters=10, warm=2), time_events(fwd_bwd, iters=10, warm=2)
        finally:
            lib.call('ha_tune_set', b'rollout_persist', 1)
        out[name] = {'fwd_ms': round(tf, 3), 'fwd_bwd_ms': round(tb, 3), 'steps_per_sec_fwd': round(B_SEQ * S / (tf * 1e-3), 1),
                     'steps_per_sec_fwd_bwd': round(B_SEQ * S / (tb * 1e-3), 1)}
    res = dict(out['persistent_forward'])
    res.update(batch=B_SEQ, steps=S, launch_chain=out['launch_chain'])
    return res


def lbfgs_profile(dev, npz, k=5):
    """REAL outer iterations: MotionOptimizer.run on the C4 problem with k torch.optim.LBFGS.step calls (max_iter 20, strong-Wolfe)
    per stage and per stage-3 phase (tune-init on the first 15 frames / frozen-init / refine); wall time per phase from
    MotionOptimizer.stage_profile (a device synchronise at every phase boundary)."""
    from humor_amd.configs import NUM_ITER_RGB, STAGE3_TUNE_INIT_FREEZE
    totals = []
    for rep in range(2):
        # Two fits, each with a NEW MotionOptimizer (its own optimisers, histories and hipGraph captures); the SECOND one is reported: the
        # first also pays what a process pays once -- code-object loads, the caching allocator growing back after the 256 x 120 closure
        # measured before (empty_cache) -- and with 15 outer iterations per stage that one-off cost moved the stage-2 figure by 50 %
        # between two otherwise identical runs (profiles/r05_mid vs the steady-state A/B of tools/stage_lbfgs_n.py).
        opt = build_optimizer(dev, npz, B_SEQ, use_graphs='auto')      # MotionOptimizer's default: hipGraph replay for the short closures
        opt.stage3_tune_init_freeze_start, opt.stage3_tune_init_freeze_end = k, 2 * k
        opt.stage_profile = {}
        obs, _ = make_problem(B_SEQ, T_SEQ, seed=100, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        # (stages 1-2: 3 k iterations each -- their evaluations are 0.3 ms, and a phase's wall time includes the one-off capture of its graph)
        opt.run(obs, data_fps=30, lr=1.0, num_iter=[3 * k, 3 * k, 3 * k], lbfgs_max_iter=20)
        torch.cuda.synchronize()
        totals.append(time.perf_counter() - t0)
    total = totals[-1]
    prof = {n: v for n, v in opt.stage_profile.items() if not n.startswith('_')}
    out = {'k_outer_iters_per_phase': k, 'lbfgs_max_iter': 20, 'measured_run_seconds': round(total, 3), 'first_run_seconds': round(totals[0], 3), 'phases': {},
           'note': 'second of two fits in this process (new MotionOptimizer each); each phase includes the one-off hipGraph capture of its closure '
                   'where use_graphs=auto captures it (stages 1-2, tune-init) and the first step of its optimiser'}
    f0, f1 = STAGE3_TUNE_INIT_FREEZE
    sched = {'stage1': NUM_ITER_RGB[0], 'stage2': NUM_ITER_RGB[1], 'stage3_tune_init': f0, 'stage3_frozen_init': f1 - f0,
             'stage3_refine': NUM_ITER_RGB[2] - f1}
    whole = 0.0
    for name, n_full in sched.items():
        p = prof.get(name)
        if not p or not p['outer_iters']:
            continue
        rate = p['outer_iters'] / p['seconds']
        out['phases'][name] = {'outer_iters_per_sec': round(rate, 3), 'closure_evals_per_outer_iter': round(p['closure_evals'] / p['outer_iters'], 2),
                               'closure_evals_per_sec': round(p['closure_evals'] / p['seconds'], 2), 'ms_per_closure_eval': round(1e3 * p['seconds'] / max(1, p['closure_evals']), 3)}
        whole += n_full / rate
    s3 = [prof[n] for n in ('stage3_tune_init', 'stage3_frozen_init', 'stage3_refine') if n in prof]
    if s3:
        out['stage3_outer_iters_per_sec'] = round(sum(p['outer_iters'] for p in s3) / sum(p['seconds'] for p in s3), 3)
    out['whole_fit_seconds_for_30_80_70_schedule'] = round(whole, 2)
    out['whole_fit_outer_iters_per_sec'] = round(sum(sched.values()) / whole, 3) if whole > 0 else None
    return out


def rccl_selfcheck(dev, npz):
    """World-size-1 RCCL process group on the one GPU: init_process_group('nccl'), the sharded closure path (differentiable halo
    all-gather + packed gradient all-reduce) evaluated through it, and the two collectives timed with HIP events.  Catches
    import / ABI / device_id errors of the N>1 path that a 1-GPU box can discover."""
    import torch.distributed as dist
    out = {'backend': 'nccl (RCCL)', 'world_size': 1}
    try:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(29400 + os.getpid() % 500))
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
        fc = FitClosure(dev, npz, 1, 0, dist.group.WORLD, use_graphs=False)
        l0 = float(fc.step().detach())
        ref = FitClosure(dev, npz, 1, 0, None, use_graphs=False)
        l1 = float(ref.step().detach())
        out['sharded_closure_loss_rel_diff_vs_unsharded'] = abs(l0 - l1) / abs(l1)
        n = sum(p.numel() for p in fc.params) + 1
        packed = torch.zeros(n, device=dev)
        out['allreduce_packed_floats'] = n
        out['allreduce_us'] = round(1e3 * time_events(lambda: dist.all_reduce(packed), iters=50, warm=5), 2)
        halo = torch.zeros(T_SEQ * 43 * 3 + 16 + 3, device=dev)
        bufs = [torch.empty_like(halo)]
        out['allgather_halo_floats'] = halo.numel()
        out['allgather_us'] = round(1e3 * time_events(lambda: dist.all_gather(bufs, halo), iters=50, warm=5), 2)
        out['ok'] = out['sharded_closure_loss_rel_diff_vs_unsharded'] < 1e-5
        del fc, ref
    except Exception as e:                                   # report, never take the benchmark down
        out['ok'] = False
        out['error'] = '%s: %s' % (type(e).__name__, str(e)[:300])
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    torch.cuda.empty_cache()
    return out


def oracle_pin(ds):
    """Chain of custody of the CPU baseline on the timing box (/root/reference does not exist there): before it is timed, the
    restated closure must reproduce the loss the REFERENCE MotionOptimizer produced for the committed fixture
    tests/golden/closure_c4.npz (8 x 60, overlap 10; generated in the build container by oracle/make_golden_long.py)."""
    from humor_amd import synth
    from oracle import closure_cases as CC
    from oracle.closure_restated import RestatedFit
    gd = np.load(os.path.join(ROOT, 'tests', 'golden', 'closure_c4.npz'))
    B, T, ov = int(gd['B']), int(gd['T']), int(gd['ov'])
    case = CC.make_case(str(gd['kind']), B, T, seed=int(gd['seed']), ov=ov)
    fit = RestatedFit(ds, synth.contractive_state_dict(int(gd['weight_seed'])), synth.SynthVPoser(seed=0), synth.make_gmm(seed=0), CC.RGB_WEIGHTS,
                      B, T, True, CC.camera_matrix(B))
    var = {k: (v[:, :1] if k in ('trans', 'root_orient', 'latent_pose') else v).clone() for k, v in case['var'].items()}
    with torch.no_grad():
        loss = float(fit.objective(var, case['obs']))
    ref = float(gd['s2_loss'])
    rel = abs(loss - ref) / abs(ref)
    assert rel < 1e-4, f'oracle/closure_restated.py does not reproduce the reference fixture closure_c4.npz: {loss} vs {ref}'
    return {'fixture': 'tests/golden/closure_c4.npz (reference MotionOptimizer stage-3 objective, 8x60)', 'loss_rel': float('%.3g' % rel)}


def cpu_baseline(npz, gpu_eval=None):
    """oracle/closure_restated.py (restatement of the reference closure: dense smplx-style SMPL on the expanded B*T batch,
    Python roll-out loop) on the host cores, at the FULL C4 size (32 x 60), forward + backward.  The thread count is swept once
    ({16, 32, 64}: one timed evaluation each after a warm-up) and the best one is timed for the reported value."""
    from humor_amd import synth
    from oracle.closure_restated import RestatedFit
    avail = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else os.cpu_count()
    data = np.load(npz)

    class DS:
        pass
    ds = DS()
    for k in data.files:
        setattr(ds, k, data[k])
    cpu = torch.device('cpu')
    torch.set_num_threads(min(avail, 32))
    pin = oracle_pin(ds)
    obs, init = make_problem(B_SEQ, T_SEQ, seed=100, device=cpu)
    fit = RestatedFit(ds, humor_weights(), synth.SynthVPoser(seed=0), synth.make_gmm(seed=0), loss_weights(),
                      B_SEQ, T_SEQ, True, camera_matrix(B_SEQ, cpu))
    parity = None
    if gpu_eval is not None:
        # the oracle closure at EXACTLY the variables of one GPU closure evaluation of the timed workload: loss and every gradient,
        # per sub-sequence.  ReLU(GroupNorm) kinks: a sub-sequence with a unit within fp32 rounding of its kink has a gradient that
        # moves by 1e-3..1e-2 between two CORRECT fp32 evaluations (tests/rollout_checks.py); such sequences are found by
        # re-evaluating the oracle at 1-ulp perturbations of the variables and are reported separately.
        def oracle_eval(var):
            pv = {k: v.clone().requires_grad_(True) for k, v in var.items()}
            ploss = fit.objective(pv, obs)
            pg = torch.autograd.grad(ploss, list(pv.values()), allow_unused=True)
            return float(ploss), {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(pv.items(), pg)}

        def per_seq(a, b):      # max |a - b| per sub-sequence relative to max(1, max |b|) of the tensor
            return (a - b).abs().reshape(a.shape[0], -1).amax(dim=1) / max(1.0, b.abs().max().item())
        oloss, og = oracle_eval(gpu_eval['var'])
        flagged = torch.zeros(B_SEQ, dtype=torch.bool)
        for k in range(6):
            gp = torch.Generator().manual_seed(7 + k)
            pvar = {n: v * (1.0 + ((torch.rand(v.shape, generator=gp) > 0.5).float() * 2 - 1) * 2.0 ** -23) for n, v in gpu_eval['var'].items()}
            _, pg2 = oracle_eval(pvar)
            for n in og:
                flagged |= per_seq(pg2[n], og[n]) >= 2e-4
        by_oracle = int(flagged.sum())
        # (the bar applies to every sub-sequence the ORACLE's perturbations do not flag; sub-sequences whose own GPU gradient is unstable
        # are reported, not excused: a GPU-side bug that made gradients noisy must not clear itself)
        gpu_unstable = gpu_eval.get('gpu_unstable')
        worst_all, worst_stable, per = 0.0, 0.0, {}
        over = torch.zeros(B_SEQ, dtype=torch.bool)
        for n in og:
            e = per_seq(gpu_eval['grad'][n], og[n])
            per[n] = float('%.3g' % e.max().item())
            worst_all = max(worst_all, e.max().item())
            if (~flagged).any():
                worst_stable = max(worst_stable, e[~flagged].max().item())
            over |= e > 1e-3
        parity = {'loss_rel': float('%.3g' % (abs(gpu_eval['loss'] - oloss) / abs(oloss))),
                  'grad_rel_max': float('%.3g' % worst_stable), 'grad_rel_max_incl_kink_sequences': float('%.3g' % worst_all),
                  'kink_flagged_sequences': int(flagged.sum()), 'kink_flagged_by_oracle_perturbations': by_oracle,
                  'gpu_unstable_sequences_informational': int(gpu_unstable.sum()) if gpu_unstable is not None else None,
                  'gpu_unstable_not_oracle_flagged': int((gpu_unstable & ~flagged).sum()) if gpu_unstable is not None else None,
                  'unflagged_sequences_over_1e-3': int((over & ~flagged).sum()),
                  'sequences_within_1e-3': int((~over).sum()), 'sequences': B_SEQ,
                  'grad_rel_by_tensor_incl_kink_sequences': per, 'oracle_loss': oloss, 'gpu_loss': gpu_eval['loss'],
                  'what': 'GPU stage-3 closure of the timed workload (32x60) vs oracle/closure_restated.py at the same variables; gradient error per '
                          'sub-sequence relative to max(1, max|oracle gradient|) of the tensor; kink-flagged = sub-sequences whose ORACLE gradient moves >= 2e-4 '
                          'under 1-ulp perturbations of the variables (six perturbations, 4.8 s each; the GPU closure\'s own sensitivity under 48 perturbations is '
                          'reported as gpu_unstable_*, it excuses nothing): a ReLU(GroupNorm) unit within fp32 rounding of its kink, where no two fp32 evaluations agree to 1e-3 '
                          '(the set grows with the number of perturbations tried, tests/rollout_checks.py); bars: loss 1e-4, gradients 1e-3 on the unflagged '
                          'sub-sequences'}
    g = torch.Generator().manual_seed(3)
    var = {'trans': init['trans'][:, :1].clone(), 'root_orient': init['root_orient'][:, :1].clone(),
           'latent_pose': init['latent_pose'][:, :1].clone(), 'betas': init['betas'].clone(),
           'latent_motion': 0.5 * torch.randn(B_SEQ, T_SEQ - 1, 48, generator=g), 'trans_vel': 0.1 * torch.randn(B_SEQ, 1, 3, generator=g),
           'joints_vel': 0.1 * torch.randn(B_SEQ, 1, 22, 3, generator=g), 'root_orient_vel': 0.1 * torch.randn(B_SEQ, 1, 3, generator=g),
           'floor_plane': torch.tensor([[0.0, 0.5, 0.0]]).expand(B_SEQ, 3).clone()}
    var = {k: v.requires_grad_(True) for k, v in var.items()}

    def step():
        loss = fit.objective(var, obs)
        torch.autograd.grad(loss, list(var.values()), allow_unused=True)
    # measured once on the 256-core box (profiles/r02_*): 32 threads 4.9 s, 64: 6.7 s, 128: 13.5 s, 256: 656 s per evaluation --
    # torch's intra-op pool degrades badly when oversubscribed, so the sweep stays at the low end and stops once it gets slower
    sweep = {}
    for n in sorted({min(avail, c) for c in (16, 32, 64)}):
        torch.set_num_threads(n)
        if not sweep:
            step()                 # warm-up (allocator, first-touch)
        t0 = time.time()
        step()
        sweep[n] = time.time() - t0
        if len(sweep) > 1 and sweep[n] > 1.3 * min(sweep.values()):
            break
    ncores = min(sweep, key=sweep.get)
    torch.set_num_threads(ncores)
    reps, t0 = 0, time.time()
    while reps < 2 or (time.time() - t0 < 12.0 and reps < 20):
        step()
        reps += 1
    dt = (time.time() - t0) / reps
    return {'value': round(1.0 / dt, 4), 'unit': 'closure-evals/s', 'cores': ncores, 'kind': 'port', 'pin': pin, 'parity': parity,
            'thread_sweep_seconds_per_eval': {str(k): round(v, 3) for k, v in sweep.items()},
            'sample': f'full C4 batch 32x60, {reps} timed stage-3 closure evaluations (fwd+bwd), {dt * 1e3:.0f} ms each, at the best thread count '
                      f'of a one-evaluation sweep over {sorted(sweep)} threads ({avail} cores visible); '
                      f'oracle/closure_restated.py = reference closure restated (5 dense 6890-vertex SMPL calls on the expanded B*T batch, '
                      f'59-step Python roll-out loop, VPoser, all loss terms), torch CPU'}


def dump_outputs(outdir, arrays):
    os.makedirs(outdir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(outdir, name + '.npy'), a)


def self_launch(args):
    """`python bench.py --gpus N` without a launcher (WORLD_SIZE unset): start the N ranks ourselves, one per GPU, exactly as the
    driver's torch.distributed.run command line would, and relay rank 0's JSON line."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(args))
    # the contract is ONE JSON line on stdout: libraries that print to the C-level stdout (RCCL's version banner) are sent to
    # stderr for the duration of the run; fd 1 is restored for the final line only
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    try:
        line = run(args)
    finally:
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        os.dup2(saved_stdout, 1)
        os.close(saved_stdout)
    if line is not None:
        print(line, flush=True)


def run(args):
    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local = int(os.environ.get('LOCAL_RANK', 0))
    assert world == args.gpus, f'--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks'
    dist = None
    # validation aid for 1-GPU boxes: HUMOR_AMD_BENCH_BACKEND=gloo HUMOR_AMD_BENCH_ONE_GPU=1 runs all ranks on cuda:0 with host-
    # staged collectives (exercises the sharded code path; the numbers mean nothing).  Default: one GPU per rank over RCCL.
    backend = os.environ.get('HUMOR_AMD_BENCH_BACKEND', 'nccl')
    dev = torch.device('cuda:0' if os.environ.get('HUMOR_AMD_BENCH_ONE_GPU') == '1' else f'cuda:{local}')
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if backend == 'nccl':
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from humor_amd import synth
    tmp = tempfile.mkdtemp(prefix='humor_amd_bench_')
    npz = synth.write_smplh_npz(os.path.join(tmp, f'model_{rank}.npz'), seed=0)
    # Closure mode.  hipGraph replay pays ~1.5 us of node hand-off per kernel, eager launches pay host time that the roll-out's
    # long launches partly hide; which one wins depends on the host CPU, so at N=1 both are timed on a throw-away instance
    # each (separate instances: an eager evaluation next to a live capture runs 10-20 % slower) and the faster is benchmarked.
    # N>1 always runs eagerly: capturing RCCL collectives cannot be exercised in the 1-GPU development environment, and a
    # rank-divergent capture failure would dead-lock the job.
    mode_note = None
    if world > 1 or args.eager:
        use_graphs = False
    elif not args.auto:
        use_graphs = True
    else:
        def probe(f, n=12):
            for _ in range(4):
                f.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                f.step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n
        f_graph = FitClosure(dev, npz, 1, 0, None, use_graphs=True)
        t_graph = probe(f_graph)
        del f_graph
        torch.cuda.empty_cache()
        fc = FitClosure(dev, npz, 1, 0, None, use_graphs=False)
        t_eager = probe(fc)
        use_graphs = t_graph < t_eager
        mode_note = 'picked by a one-off timing on separate instances: hipGraph replay %.2f ms vs eager %.2f ms per closure' % (
            1e3 * t_graph, 1e3 * t_eager)
        if use_graphs:
            del fc
            torch.cuda.empty_cache()
            fc = None
    if not (world == 1 and not args.eager and args.auto and not use_graphs):
        fc = FitClosure(dev, npz, world, rank, None, use_graphs=use_graphs)
    fc.mode_note = mode_note

    def timed(f):
        """W untimed + exactly K timed closure evaluations, bracketed by barrier + synchronise; MAX over ranks (seconds)."""
        for _ in range(args.warmup):
            f.step()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            f.step()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        d = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([d], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            d = t.item()
        return d
    dt = timed(fc)
    if args.dump_outputs and rank == 0:
        # read before anything else evaluates a closure (a sharded closure's gradients live in an arena the next evaluation zero-fills)
        dump_outputs(args.dump_outputs, fc.outputs())
    roof_early = None
    if rank == 0 and args.full:
        # the roofline kernel at the metric's batch, measured right behind the headline timing: behind the 256 x 120 closure / the C5 sizes the
        # chip sits in a power-management transient (MI355X_MICROARCH.md, DVFS give-back; profiles/r02_run20_skin_jitter.txt) that cost this
        # HBM-bound kernel 5-10 % in the round-5 runs (0.59-0.62 measured there against 0.63-0.65 of the rounds that measured it first)
        roof_early = skin_roofline(dev, npz, rotate=4)
        roof_early['cache_warm_single_set'] = {k: v for k, v in skin_roofline(dev, npz, rotate=1).items() if k in ('achieved', 'frac', 'avg_launch_us')}
        roof_early['ceilings'] = skin_ceilings(dev, npz, roof_early)
        roof_early['measured'] = 'right behind the headline closure timing, before the 32 x 120 / 256 x 120 closures'
    # Two more jobs beside the headline (SCALE runs: make the curves unambiguous).
    #   strong  -- the ONE 32-sequence job BASELINE.json / north_star name ("batch=32 sub-seqs of 60 frames sharded over 8 MI355X": 4 per GPU
    #              at N = 8).  Chain-bound: a rank's closure is a 59-step dependent chain whatever its share is.
    #   c5_weak -- BASELINE config 5's shape per GPU: 32 sub-sequences x 120 frames on every rank (256 x 120 at N = 8).
    strong = None
    if args.full and world > 1 and args.scaling in ('strong', 'both') and B_SEQ >= world:
        del fc
        torch.cuda.empty_cache()
        fc = FitClosure(dev, npz, world, rank, None, use_graphs=False, B_total=B_SEQ)
        fc.mode_note = None
        dts = timed(fc)
        strong = {'scaling': 'strong', 'global_batch': B_SEQ, 'sequences_per_gpu': [B_SEQ // world + (1 if r < B_SEQ % world else 0) for r in range(world)],
                  'value': round(args.steps / dts, 3), 'unit': 'closure-evals/s of the one 32x60 job', 'ms_per_step': round(dts / args.steps * 1e3, 4)}
    elif world == 1:
        strong = {'scaling': 'strong', 'global_batch': B_SEQ, 'sequences_per_gpu': [B_SEQ], 'value': round(args.steps / dt, 3),
                  'unit': 'closure-evals/s of the one 32x60 job', 'ms_per_step': round(dt / args.steps * 1e3, 4), 'note': 'N = 1: the same run as `value`'}
    c5_weak = None
    if args.full and not args.no_c5_weak:
        keep = fc
        f5 = FitClosure(dev, npz, world, rank, None, use_graphs=False, T=120)
        f5.mode_note = None
        dt5 = timed(f5)
        del f5
        torch.cuda.empty_cache()
        fc = keep
        c5_weak = {'scaling': 'weak', 'workload': f'32 sub-sequences x 120 frames per GPU ({B_SEQ * world} x 120 in all; BASELINE config 5 is 256 x 120 = N 8)',
                   'value': round(args.steps * world / dt5, 3), 'unit': 'closure-evals/s (32x120-batch equivalents)', 'ms_per_step': round(dt5 / args.steps * 1e3, 4)}
    c5_full = None
    if args.full and world == 1 and not args.no_c5_weak:
        # BASELINE config 5 as it stands (256 sub-sequences x 120 frames) as ONE stage-3 closure on one GPU: the roll-out runs on the
        # pipelined persistent kernels (rollout_pipe.inc), SMPL / losses on 30 720 frames
        try:
            keep = fc
            f5 = FitClosure(dev, npz, 1, 0, None, use_graphs=False, B_total=256, T=120)
            f5.mode_note = None
            k5 = max(2, min(args.steps, 5))
            for _ in range(2):
                f5.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k5):
                f5.step()
            torch.cuda.synchronize()
            dtf = (time.perf_counter() - t0) / k5
            del f5
            torch.cuda.empty_cache()
            fc = keep
            c5_full = {'workload': '256 sub-sequences x 120 frames, one stage-3 closure (fwd+bwd) on ONE GPU', 'steps': k5,
                       'ms_per_step': round(dtf * 1e3, 3), 'value': round(1.0 / dtf, 3), 'unit': 'closure-evals/s (256x120 batch)',
                       'sub_sequence_frames_per_sec': round(256 * 120 / dtf, 1)}
        except Exception as e:                               # report, never take the benchmark down
            c5_full = {'error': '%s: %s' % (type(e).__name__, str(e)[:300])}
            torch.cuda.empty_cache()
    coll = None
    if args.full and dist is not None:
        n = sum(p.numel() for p in fc.params) + 1
        packed = torch.zeros(n, device=dev)
        halo = torch.zeros(T_SEQ * 43 * 3 + 16 + 3, device=dev)
        bufs = [torch.empty_like(halo) for _ in range(world)]
        coll = {'backend': backend, 'allreduce_packed_floats': n,
                'allreduce_us': round(1e3 * time_events(lambda: dist.all_reduce(packed), iters=50, warm=5), 2),
                'allgather_halo_floats': halo.numel(),
                'allgather_us': round(1e3 * time_events(lambda: dist.all_gather(bufs, halo), iters=50, warm=5), 2),
                'collectives_per_closure': '1 differentiable halo all-gather (+ its all-reduce in backward) + 1 packed [gradient | loss] all-reduce'}

    if rank == 0:
        res = {
            'metric': 'fitting closure evaluations/s (stage-3 objective fwd+bwd), batch=32 seq=60 per GPU',
            'value': round(args.steps * world / dt, 3), 'unit': 'closure-evals/s (32x60-batch equivalents)',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(dt / args.steps * 1e3, 4), 'higher_is_better': True, 'scaling': 'weak',
            'strong_value': strong['value'] if strong is not None else None,
            'strong_ms_per_step': strong['ms_per_step'] if strong is not None else None,
            'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            # BASELINE.json config 4 / north_star name the STRONG job (one batch of 32 sub-sequences sharded over the GPUs): a reader of a
            # SCALE file must take `strong_value` for that curve; `value` (the contract's whole-job aggregate) is the WEAK job
            'north_star_job': 'strong',
            'config': {'workload': f'strong_value (STRONG, the job BASELINE.json config 4 names): the ONE 32 x 60 job, {B_SEQ} sub-sequences sharded '
                                   f'{B_SEQ // world if world <= B_SEQ else 0} per GPU; value (WEAK): the same shape with 32 overlapping sub-sequences x 60 '
                                   f'frames PER GPU (one coupled job of {B_SEQ * world} sub-sequences) -- at N = 1 the two are the same run.  Both: '
                                   'C4 fit_rgb_demo_use_split shape, joints2d + floor + overlap-consistency, SMPL+H 6890 verts / 52 joints / 16 betas, '
                                   'HuMoR 48-d latent, 59-step roll-out; step = one stage-3 closure (fwd+bwd).  c5_weak: 32 x 120 per GPU (BASELINE config 5 '
                                   'shape at N = 8); c5_full (N = 1 only): the whole 256 x 120 batch of config 5 as ONE closure on one GPU',
                       'global_batch': B_SEQ * world, 'strong_global_batch': B_SEQ, 'seq_len': T_SEQ,
                       'parallelism': f'dp{world} (sub-sequence sharding, replicated L-BFGS)'},
            'closure_mode': closure_mode(args, fc),
        }
        if strong is not None:
            res['strong'] = strong
    if rank == 0 and args.full:
        gpu_eval = fc.snapshot() if world == 1 and not args.no_cpu_baseline else None      # for the parity field (untimed)
        if gpu_eval is not None:
            gpu_eval['gpu_unstable'] = fc.gradient_sensitivity()
        ms_dense, ms_dense_fb = dense_smpl_ms(dev, npz)
        res.update({
            'smpl_verts_per_sec': round(B_SEQ * T_SEQ * V / (ms_dense * 1e-3), 1),
            'smpl_dense_fwd_ms': round(ms_dense, 4),
            'smpl_dense_fwd_bwd_ms': round(ms_dense_fb, 4),
            'smpl_verts_per_sec_fwd_bwd': round(B_SEQ * T_SEQ * V / (ms_dense_fb * 1e-3), 1),
            'rollout': rollout_c4_ms(dev),
            # the roofline kernel at the metric's batch, HBM figure: launches rotate over 4 operand sets (1.27 GB: > 256 MiB of other
            # lines between two uses of any line); the single-set (Infinity-Cache-assisted) figure of rounds 1-2 is kept beside it
            'roofline': roof_early,
        })
        if c5_weak is not None:
            res['c5_weak'] = c5_weak
        if c5_full is not None:
            res['c5_full'] = c5_full
        if coll is not None:
            res['rccl'] = coll
        if world == 1 and not args.no_lbfgs:
            del fc
            fc = None
            torch.cuda.empty_cache()
            res['lbfgs'] = lbfgs_profile(dev, npz)
            # the "fitting-iter/sec" of BASELINE.json's metric in L-BFGS outer iterations (whole 30/80/70 fit), next to `value`
            res['outer_iters_per_sec'] = res['lbfgs'].get('whole_fit_outer_iters_per_sec')
        if world == 1 and not args.no_rccl_check:
            res['rccl'] = rccl_selfcheck(dev, npz)
        if world == 1 and not args.no_c5:
            # the roofline kernel again at the C5 size: operands far beyond the Infinity Cache, i.e. the cache-free figure
            fc = None
            torch.cuda.empty_cache()
            res['roofline_c5'] = skin_roofline(dev, npz, N=256 * 120)
            res['roofline_c5']['note'] = ('cache-free size (5.2 GB per launch); at this size the kernel\'s own copy-only mode reaches 5.77 TB/s '
                                          'and a torch device copy 4.94 TB/s (profiles/r02_pmc_lbs/SUMMARY.txt)')
            res['roofline']['note'] = ('the metric\'s batch (32 x 60) on 4 rotating operand sets = streamed from / to HBM; cache_warm_single_set = the '
                                       'same launches on ONE 159 + 159 MB set (partly served by the 256 MiB Infinity Cache: the figure of rounds 1-2); '
                                       'roofline_c5 = the cache-free C5 size, sustained')
            # BASELINE config C5 (batch 256 x 120 frames): LBS GB/s, pose-blend and decoder/prior MLP fp32-MFMA utilisation
            sys.path.insert(0, os.path.join(ROOT, 'tools'))
            import bench_c5
            fc = None
            torch.cuda.empty_cache()
            res['c5_rooflines'] = bench_c5.measure(256, 120, dev)
        if not args.no_cpu_baseline and world == 1:      # the CPU baseline is timed on rank 0 of the 1-GPU run only
            res['cpu_baseline'] = cpu_baseline(npz, gpu_eval)
            res['parity'] = res['cpu_baseline'].pop('parity')
    if rank == 0:
        # the contract's keys first (a reader that truncates the line keeps them), the detailed side measurements after
        head = ['metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'north_star_job', 'strong_value',
                'strong_ms_per_step', 'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline', 'parity', 'outer_iters_per_sec', 'smpl_verts_per_sec', 'closure_mode',
                'strong', 'c5_weak', 'c5_full', 'rccl']
        res = {**{k: res[k] for k in head if k in res}, **{k: v for k, v in res.items() if k not in head}}
        line = json.dumps(res)
    else:
        line = None
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return line


if __name__ == '__main__':
    main()
