"""ha_tune_set("loss_merge"): the merged loss-side launches (ha_fit_loss with the init-state mixture inside its two launches and the LDS-staged
reduction; ha_rollout_post_backward's reduction with the row-sum task) against the one-launch-per-kernel form, bit for bit, and against the
references the fit tests use (term-by-term FittingLoss, the op chain of rollout_latent_motion) at those tests' tolerances."""
import contextlib
import ctypes as C

import torch

import fitloss_checks as FL
from humor_amd import _lib, synth
from humor_amd.fitting_loss import FittingLoss
from humor_amd.tables import OP_IGNORE_JOINTS, SMPLH_TO_OPENPOSE25

# (B, T): one sequence with S = 1 | 15 frames, fewer than 64 lanes | 260 frames: one trip of the 256-frame unrolled loop + a remainder,
# two staged chunks | 300 frames
FIT_SHAPES = [(1, 2), (3, 5), (2, 130), (5, 60)]
# 2100 frames: more than the 2048 whose partial sums the reduction fetches at once -- a second group, holding one short chunk
LONG_SHAPE = (3, 700)
# (B, T) of the post reduction: the above and T = 65 -- more frames than lanes, two staged chunks of 64 frames
POST_SHAPES = FIT_SHAPES + [(2, 65)]


def set_merge(lib, v):
    lib.call('ha_tune_set', b'loss_merge', int(v))


@contextlib.contextmanager
def both_settings(lib):
    """yields the two knob values in turn; the default (1) is back in place afterwards, whatever happens"""
    def gen():
        for v in (1, 0):
            set_merge(lib, v)
            yield v
    try:
        yield gen()
    finally:
        set_merge(lib, 1)


@contextlib.contextmanager
def recorded_buffers():
    """every floating-point tensor torch.empty hands out inside the block, in allocation order: the fused op's flat buffer (gradients of every
    input | terms | loss | mixture total | per-frame partials) and the mixture's lp, gpart, nll, g_x"""
    got, inner = [], torch.empty

    def empty(*a, **k):
        t = inner(*a, **k)
        if t.is_floating_point():
            got.append(t)
        return t
    torch.empty = empty
    try:
        yield got
    finally:
        torch.empty = inner


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_fit_loss(lib, device, B, T, K, kind, halo=False, cond=True, seed=0):
    """FusedFit at both knob values: loss, term values (the mixture's total among them), the gradient of every input and every buffer the op
    allocates (flat gradients + per-frame partials, lp, gpart, nll, g_x) bit for bit; then knob 1 against the term-by-term evaluation at the
    tolerances of fitloss_checks.check_fused_vs_terms.  kind 'motion' has the mixture, 'smpl' / 'root' have none."""
    w, mu, cov = synth.make_gmm(seed=0, ncomp=K)
    gmm = {'gmm': (w.to(device), mu.to(device), cov.to(device))}
    cam_f = torch.tensor([[1060.5, 1060.4]]).expand(B, 2).to(device)
    cam_c = torch.tensor([[951.3, 536.8]]).expand(B, 2).to(device)
    mk = lambda fused: FittingLoss([FL.ALL_ON] * 3, gmm, SMPLH_TO_OPENPOSE25, OP_IGNORE_JOINTS, cam_f, cam_c, 'bisquare', joints2d_sigma=100,
                                   fused=fused, _lib_override=lib)
    fused, terms = mk(True), mk(False)
    diff, obs = FL.make_inputs(B, T, device, seed=seed, halo=halo)
    res = {}
    with both_settings(lib) as settings:
        for v in settings:
            with recorded_buffers() as bufs:
                l, s, g = FL.evaluate(fused, kind, diff, obs, halo, cond)
            res[v] = (l, s, g, list(bufs))
    (l1, s1, g1, b1), (l0, s0, g0, b0) = res[1], res[0]
    assert bits_equal(l1, l0), (l1.item(), l0.item())
    assert set(s1) == set(s0)
    for k in s0:
        assert bits_equal(torch.as_tensor(s1[k]), torch.as_tensor(s0[k])), (k, float(s1[k]), float(s0[k]))
    for k in g0:
        assert bits_equal(g1[k], g0[k]), k
    assert len(b1) == len(b0) == (5 if kind == 'motion' else 1), (len(b1), len(b0))
    if kind != 'motion':             # flat = [gradients | terms NT | loss | mixture total | partials F * NT]: no mixture, nobody writes its total
        b1[0], b0[0] = (torch.cat([t[:-B * T * 17 - 1], t[-B * T * 17:]]) for t in (b1[0], b0[0]))
    for i, (p, q) in enumerate(zip(b1, b0)):
        assert bool(torch.isfinite(p).all()), ('a buffer of the merged launches was left partly unwritten', i, tuple(p.shape))
        assert bits_equal(p, q), ('buffer', i, tuple(p.shape))
    # the reference
    lr, sr, gr = FL.evaluate(terms, kind, diff, obs, halo, cond)
    assert abs(l1.item() - lr.item()) <= 2e-5 * abs(lr.item()), (l1.item(), lr.item())
    assert set(s1) == set(sr)
    for k in sr:
        assert abs(float(s1[k]) - float(sr[k])) <= 2e-5 * max(1.0, abs(float(sr[k]))), (k, float(s1[k]), float(sr[k]))
    worst = 0.0
    for k in gr:
        if gr[k] is None:
            assert g1[k] is None or float(g1[k].abs().max()) == 0.0, k
            continue
        e = (g1[k] - gr[k]).abs().max().item() / max(1.0, gr[k].abs().max().item())
        worst = max(worst, e)
        assert e <= 1e-4, (k, e)
    return worst


def check_post_backward(lib, device, B, T, cam, add1, add2, W=16, seed=0):
    """ha_rollout_post_backward with the row-sum task at both knob values: every gradient output and the row sums bit for bit; the row sums also
    against ha_seq_sum_add itself (bit for bit) and a float64 sum."""
    from oracle import lbs_restated as L
    S = T - 1
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: (sc * torch.randn(*s, generator=g))
    world = r(B, S, 348, sc=0.5)
    world[:, :, 6:15] = L.batch_rodrigues(r(B * S, 3, sc=1.5)).reshape(B, S, 9)
    world[:, :, 18:207] = L.batch_rodrigues(r(B * S * 21, 3, sc=0.8)).reshape(B, S, 189)
    ins = dict(world=world, trans0=r(B, 3), root0=r(B, 3, sc=0.8), pose0=r(B, 63, sc=0.4), joints0=r(B, 22, 3))
    if cam:
        ins.update(c2p_R=L.batch_rodrigues(r(B, 3)).reshape(B, 3, 3), c2p_t=r(B, 3))
    gin = dict(g_trans=r(B, T, 3), g_root_orient=r(B, T, 3), g_pose_body=r(B, T, 63), g_joints=r(B, T, 22, 3), g_contacts_conf=r(B, T, 22))
    if cam:
        gin.update(g_cam_trans=r(B, T, 3), g_cam_root_orient=r(B, T, 3))
    task = dict(sum_src=r(B, T, W), sum_add1=r(B, W) if add1 else None, sum_add2=r(B, W) if add2 else None)
    ins, gin, task = ({k: (None if v is None else v.contiguous().to(device)) for k, v in d.items()} for d in (ins, gin, task))
    new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)
    fwd = dict(trans=new(B, T, 3), root_orient=new(B, T, 3), pose_body=new(B, T, 63), joints=new(B, T, 22, 3), contacts_conf=new(B, T, 22),
               contacts=new(B, T, 22))
    if cam:
        fwd.update(cam_trans=new(B, T, 3), cam_root_orient=new(B, T, 3))
    st = _lib.stream_ptr(ins['world'])

    def args(**fields):
        a = _lib.RolloutPostArgs()
        a.B, a.S, a.sum_W = B, S, W
        for k, v in fields.items():
            if v is not None:
                setattr(a, k, v.data_ptr())
        return a
    lib.call('ha_rollout_post_forward', C.byref(args(**ins, **fwd)), st)
    res = {}
    with both_settings(lib) as settings:
        for v in settings:
            out = dict(g_world=new(B, S, 348), g_trans0=new(B, 3), g_root0=new(B, 3), g_pose0=new(B, 63), g_joints0=new(B, 22, 3),
                       partial=new(B * T, 15), sum_out=new(B, W))
            if cam:
                out.update(g_c2p_R=new(B, 3, 3), g_c2p_t=new(B, 3))
            lib.call('ha_rollout_post_backward', C.byref(args(**ins, **fwd, **gin, **task, **out)), st)
            res[v] = out
    for k in res[0]:
        assert bool(torch.isfinite(res[1][k]).all()), ('left partly unwritten', k)
        assert bits_equal(res[1][k], res[0][k]), k
    alone = new(B, W)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib.call('ha_seq_sum_add', B, T, W, p(task['sum_src']), p(task['sum_add1']), p(task['sum_add2']), p(alone), st)
    assert bits_equal(res[1]['sum_out'], alone)
    ref, mag = task['sum_src'].double().sum(1), task['sum_src'].double().abs().sum(1)
    for k in ('sum_add1', 'sum_add2'):
        if task[k] is not None:
            ref, mag = ref + task[k].double(), mag + task[k].double().abs()
    # at most T + 2 fp32 additions, each rounding by at most 2^-24 of a partial sum that the sum of the magnitudes bounds
    bound = (T + 2) * 2.0 ** -24 * mag
    assert bool(((res[1]['sum_out'].double() - ref).abs() <= bound).all())


def check_long_reduction(lib, device, B, T, seed=0):
    """ha_fit_loss with the pose-prior term alone (cheap frames, so that the host emulator can run thousands of them) at both knob values: the
    per-frame partial sums, the gradient, the term values and the loss bit for bit; the term against a float64 sum at the 2e-5 of the fit tests."""
    from humor_amd import fit_kernels as FK
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 32, generator=g).to(device)
    res = {}
    with both_settings(lib) as settings:
        for v in settings:
            out = {k: torch.empty(sh, dtype=torch.float32, device=device) for k, sh in
                   dict(terms=(FK.NT,), loss=(1,), partial=(B * T, FK.NT), g_latent_pose=(B, T, 32)).items()}
            a = _lib.FitArgs()
            a.B, a.T, a.dlp, a.nsteps, a.latent_pose = B, T, 32, 1.0, x.data_ptr()
            a.w[FK.POSE_PRIOR] = 0.3
            for k, t in out.items():
                setattr(a, k, t.data_ptr())
            lib.call('ha_fit_loss', C.byref(a), _lib.stream_ptr(x))
            res[v] = out
    for k in res[0]:
        assert bool(torch.isfinite(res[1][k]).all()), ('left partly unwritten', k)
        assert bits_equal(res[1][k], res[0][k]), k
    ref = float((x.double() ** 2).sum())
    got = float(res[1]['terms'][FK.POSE_PRIOR])
    assert abs(got - ref) <= 2e-5 * abs(ref), (got, ref)
    assert abs(float(res[1]['loss'][0]) - 0.3 * ref) <= 2e-5 * 0.3 * abs(ref)
