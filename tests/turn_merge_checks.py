"""ha_tune_set("turn_merge"): the short launches at the ends of the persistent roll-out kernels riding as block roles of ha_fit_pre_backward (the
dL/dz reduction), ha_rollout_post_backward (the prior adjoint's layout pass, the adjoint's exchange clear) and ha_fit_pre_forward (the forward's
exchange clear) -- knob 0 (each a launch of its own) against all bits on, bit for bit, and against references computed here in float64 /
by index arithmetic.  Allocations are poisoned on the GPU tier (conftest), so a word a role leaves unwritten shows as NaN."""
import contextlib
import ctypes as C

import torch

from humor_amd import _lib

ALL = _lib.TURN_DZ | _lib.TURN_POST | _lib.TURN_FWD_CLEAR
ZD, DZ_SLOTS = 48, 31
GUARD = 64                      # words behind a region that a clear must leave alone


def set_turn(lib, v):
    lib.call('ha_tune_set', b'turn_merge', int(v))


@contextlib.contextmanager
def knob_values(lib, values=(ALL, 0)):
    """yields the knob values in turn; the default (all bits) is back in place afterwards, whatever happens"""
    def gen():
        for v in values:
            set_turn(lib, v)
            yield v
    try:
        yield gen()
    finally:
        set_turn(lib, ALL)


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def launches(lib):
    n = C.c_ulonglong()
    lib.call('ha_debug_launch_count', C.byref(n))
    return n.value


def _stream(t):
    return _lib.stream_ptr(t)


def _rand(device, seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, sc=1.0: (sc * torch.randn(*s, generator=g)).to(device).contiguous()


def _fit_pre_inputs(r, B, device):
    ins = dict(floor=torch.tensor([[0.05, -1.0, 0.1]]).repeat(B, 1).to(device) * (1.0 + 0.1 * r(B, 1).abs()), trans0=r(B, 3), root0=r(B, 3, sc=0.5),
               pose0=r(B, 63, sc=0.3), jcam=r(B, 22, 3), trans_vel=r(B, 3), joints_vel=r(B, 22, 3), root_orient_vel=r(B, 3))
    return {k: v.contiguous() for k, v in ins.items()}


PRE_OUT = dict(past_in=(339,), trans_p=(3,), root_p=(3,), joints_p=(22, 3), c2p_R=(3, 3), c2p_t=(3,), root_height=(1,))
PRE_GRAD = dict(g_floor=(3,), g_trans0=(3,), g_root0=(3,), g_pose0=(63,), g_jcam=(22, 3), g_trans_vel=(3,), g_joints_vel=(22, 3), g_root_orient_vel=(3,))


def _region(device, words):
    """a region of `words` non-zero words with GUARD words behind it"""
    return torch.full((words + GUARD,), 0x5a5a5a5a, dtype=torch.int32, device=device)


def _check_cleared(buf, words, what):
    assert int((buf[:words] != 0).sum()) == 0, (what, 'words left uncleared', int((buf[:words] != 0).sum()))
    assert int((buf[words:] != 0x5a5a5a5a).sum()) == 0, (what, 'wrote behind the region')


def check_dz_in_fit_pre(lib, device, B, S, with_add, seed=0):
    """ha_fit_pre_backward with the dz task at knob 0 (a launch of its own in front) and all on (blocks of the launch): g_z and every fit_pre
    gradient bit for bit, the fit_pre gradients also against the call without a task, g_z against a float64 sum.  Launch counts 2 and 1."""
    r = _rand(device, seed)
    ins = _fit_pre_inputs(r, B, device)
    gin = dict(g_past_in=r(B, 339), g_trans_p=r(B, 3), g_root_p=r(B, 3), g_joints_p=r(B, 22, 3), g_c2p_R=r(B, 3, 3), g_c2p_t=r(B, 3), g_root_height=r(B, 1))
    part = r(S, DZ_SLOTS, 32, ZD)
    add = r(B, S, ZD) if with_add else None

    def run(task):
        o = {k: torch.empty((B,) + sh, dtype=torch.float32, device=device) for k, sh in PRE_GRAD.items()}
        g_z = torch.empty(B, S, ZD, dtype=torch.float32, device=device)
        a = _lib.FitPreArgs()
        a.B = B
        for k, v in dict(**ins, **gin, **o).items():
            setattr(a, k, v.data_ptr())
        if task:
            a.dz_part, a.dz_g_z, a.dz_B, a.dz_S, a.dz_slots = part.data_ptr(), g_z.data_ptr(), B, S, DZ_SLOTS
            if add is not None:
                a.dz_g_z_add = add.data_ptr()
        n0 = launches(lib)
        lib.call('ha_fit_pre_backward', C.byref(a), _stream(part))
        return o, g_z, launches(lib) - n0

    res = {}
    with knob_values(lib) as values:
        for v in values:
            res[v] = run(True)
    plain, _, n_plain = run(False)
    (o1, z1, n1), (o0, z0, n0) = res[ALL], res[0]
    assert (n_plain, n1, n0) == (1, 1, 2), (n_plain, n1, n0)
    assert bool(torch.isfinite(z1).all()), 'g_z left partly unwritten'
    assert bits_equal(z1, z0)
    for k in PRE_GRAD:
        assert bits_equal(o1[k], o0[k]) and bits_equal(o1[k], plain[k]), k
    # the reference: the slots of rows < B in float64; 31 + 1 fp32 additions, each rounding by at most 2^-24 of a partial sum that the sum of
    # the magnitudes bounds
    p64 = part[:, :, :B].double()
    ref, mag = p64.sum(1).permute(1, 0, 2), p64.abs().sum(1).permute(1, 0, 2)
    if add is not None:
        ref, mag = ref + add.double(), mag + add.double().abs()
    assert bool(((z1.double() - ref).abs() <= (DZ_SLOTS + 1) * 2.0 ** -24 * mag).all())


def _qoff(c):
    return (c // 4) * 128 + (c % 4)


def expected_slab(g_mu, g_var, pri_out, B, S, RT, pad):
    """the layout pass by index arithmetic: [S][RT][pad][32] quad-interleaved, g_mu | g_var * exp(log-variance) | zeros; rows >= B zero"""
    dev = pri_out.device
    out = torch.zeros(S, RT, pad * 32, dtype=torch.float32, device=dev)
    src = pri_out.reshape(S, RT, pad * 32)
    rows = torch.arange(B, device=dev)
    rt, rr = rows // 32, rows % 32
    for c in range(ZD):
        if g_mu is not None:
            out[:, rt, rr * 4 + _qoff(c)] = g_mu[:, :, c].t()
        if g_var is not None:
            # (the product in fp32, as the kernel forms it; exp may differ from the device's expf in the last bits: compared with a tolerance)
            out[:, rt, rr * 4 + _qoff(ZD + c)] = g_var[:, :, c].t() * torch.exp(src[:, rt, rr * 4 + _qoff(ZD + c)])
    return out.reshape(S, RT, pad, 32)


def check_post_merged(lib, device, B, S, with_sum, pad=104, clr_words=2500, cam=True, seed=0):
    """ha_rollout_post_backward with the layout and clear riders (and the row-sum task) at knob 0 and all on: every gradient output, the row
    sums, the reduction's outputs and the whole g_pri_all slab -- padding channels and rows >= B included -- bit for bit; the slab against index
    arithmetic (exact where it copies or zeroes, 4 ulp on the exp products); every word of the exchange region zero, none behind it touched.
    Launch counts: 2 with the riders on, 4 with them as launches of their own."""
    from oracle import lbs_restated as L
    T, W, RT = S + 1, 16, (B + 31) // 32
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
    task = dict(sum_src=r(B, T, W), sum_add1=r(B, W)) if with_sum else {}
    lay = dict(lay_g_mu=r(B, S, ZD), lay_g_var=r(B, S, ZD), lay_pri_out=r(S, RT, pad, 32, sc=0.7))
    ins, gin, task, lay = ({k: v.contiguous().to(device) for k, v in d.items()} for d in (ins, gin, task, lay))
    new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)
    fwd = dict(trans=new(B, T, 3), root_orient=new(B, T, 3), pose_body=new(B, T, 63), joints=new(B, T, 22, 3), contacts_conf=new(B, T, 22),
               contacts=new(B, T, 22))
    if cam:
        fwd.update(cam_trans=new(B, T, 3), cam_root_orient=new(B, T, 3))
    st = _stream(ins['world'])

    def args(**fields):
        a = _lib.RolloutPostArgs()
        a.B, a.S, a.sum_W = B, S, W
        for k, v in fields.items():
            setattr(a, k, v.data_ptr())
        return a
    lib.call('ha_rollout_post_forward', C.byref(args(**ins, **fwd)), st)
    res = {}
    with knob_values(lib) as values:
        for v in values:
            out = dict(g_world=new(B, S, 348), g_trans0=new(B, 3), g_root0=new(B, 3), g_pose0=new(B, 63), g_joints0=new(B, 22, 3), partial=new(B * T, 15))
            if with_sum:
                out['sum_out'] = new(B, W)
            if cam:
                out.update(g_c2p_R=new(B, 3, 3), g_c2p_t=new(B, 3))
            slab = torch.full((S, RT, pad, 32), float('nan'), dtype=torch.float32, device=device)
            xch = _region(device, clr_words)
            a = args(**ins, **fwd, **gin, **task, **lay, **out, lay_dst=slab)
            a.lay_step_stride, a.lay_RT, a.lay_pad = RT * pad * 32, RT, pad
            a.clr, a.clr_words = xch.data_ptr(), clr_words
            n0 = launches(lib)
            lib.call('ha_rollout_post_backward', C.byref(a), st)
            res[v] = (out, slab, xch, launches(lib) - n0)
    (o1, s1, x1, n1), (o0, s0, x0, n0) = res[ALL], res[0]
    assert (n1, n0) == (2, 4), (n1, n0)
    for k in o0:
        assert bool(torch.isfinite(o1[k]).all()), ('left partly unwritten', k)
        assert bits_equal(o1[k], o0[k]), k
    assert bool(torch.isfinite(s1).all()), 'the slab was left partly unwritten'
    assert bits_equal(s1, s0)
    for x, what in ((x1, 'riding'), (x0, 'own launch')):
        _check_cleared(x, clr_words, what)
    want = expected_slab(lay['lay_g_mu'], lay['lay_g_var'], lay['lay_pri_out'], B, S, RT, pad)
    var_ch = torch.zeros(pad, dtype=torch.bool, device=device)
    var_ch[ZD:2 * ZD] = True
    assert torch.equal(s1[:, :, ~var_ch], want[:, :, ~var_ch]), 'mean / padding channels or rows >= B'
    err = (s1[:, :, var_ch].double() - want[:, :, var_ch].double()).abs()
    assert bool((err <= 4 * 2.0 ** -23 * want[:, :, var_ch].double().abs()).all()), float(err.max())
    # the riders change nothing else: the same call without them
    plain = {k: torch.empty_like(v) for k, v in o0.items()}
    lib.call('ha_rollout_post_backward', C.byref(args(**ins, **fwd, **gin, **task, **plain)), st)
    for k in o0:
        assert bits_equal(o1[k], plain[k]), ('riders changed', k)


def check_fwd_clear(lib, device, B, clr_words=2500, seed=0):
    """ha_fit_pre_forward with the clear task at knob 0 and all on: the region zero, nothing behind it touched, every output bit for bit (also
    against the call without a task).  Launch counts 1 and 2."""
    r = _rand(device, seed)
    ins = _fit_pre_inputs(r, B, device)

    def run(task):
        o = {k: torch.empty((B,) + sh, dtype=torch.float32, device=device) for k, sh in PRE_OUT.items()}
        xch = _region(device, clr_words)
        a = _lib.FitPreArgs()
        a.B = B
        for k, v in dict(**ins, **o).items():
            setattr(a, k, v.data_ptr())
        if task:
            a.clr, a.clr_words = xch.data_ptr(), clr_words
        n0 = launches(lib)
        lib.call('ha_fit_pre_forward', C.byref(a), _stream(xch))
        return o, xch, launches(lib) - n0
    res = {}
    with knob_values(lib) as values:
        for v in values:
            res[v] = run(True)
    plain, _, n_plain = run(False)
    (o1, x1, n1), (o0, x0, n0) = res[ALL], res[0]
    assert (n_plain, n1, n0) == (1, 1, 2), (n_plain, n1, n0)
    _check_cleared(x1, clr_words, 'riding')
    _check_cleared(x0, clr_words, 'own launch')
    for k in PRE_OUT:
        assert bool(torch.isfinite(o1[k]).all()), ('left partly unwritten', k)
        assert bits_equal(o1[k], o0[k]) and bits_equal(o1[k], plain[k]), k


def check_task_argument_refusals(lib, device):
    """malformed rider tasks are refused by the host entry points before anything is launched"""
    import pytest
    r = _rand(device, 0)
    B = 2
    ins = _fit_pre_inputs(r, B, device)
    o = {k: torch.empty((B,) + sh, dtype=torch.float32, device=device) for k, sh in dict(**PRE_OUT, **PRE_GRAD).items()}
    buf = torch.zeros(4096, dtype=torch.float32, device=device)

    def pre(**extra):
        a = _lib.FitPreArgs()
        a.B = B
        for k, v in dict(**ins, **o).items():
            setattr(a, k, v.data_ptr())
        for k, v in extra.items():
            setattr(a, k, v)
        return a
    n0 = launches(lib)
    with pytest.raises(_lib.HumorAmdError, match='clr_words'):
        lib.call('ha_fit_pre_forward', C.byref(pre(clr=buf.data_ptr(), clr_words=0)), _stream(buf))
    with pytest.raises(_lib.HumorAmdError, match='dz task'):       # no g_z
        lib.call('ha_fit_pre_backward', C.byref(pre(dz_part=buf.data_ptr(), dz_B=B, dz_S=1, dz_slots=DZ_SLOTS)), _stream(buf))
    with pytest.raises(_lib.HumorAmdError, match='dz task'):       # a slot count the kernel is not built for
        lib.call('ha_fit_pre_backward', C.byref(pre(dz_part=buf.data_ptr(), dz_g_z=buf.data_ptr(), dz_B=B, dz_S=1, dz_slots=DZ_SLOTS - 1)), _stream(buf))
    with pytest.raises(_lib.HumorAmdError, match='dz task'):       # more rows than the partials hold
        lib.call('ha_fit_pre_backward', C.byref(pre(dz_part=buf.data_ptr(), dz_g_z=buf.data_ptr(), dz_B=33, dz_S=1, dz_slots=DZ_SLOTS)), _stream(buf))
    assert launches(lib) == n0, 'a refused call launched a kernel'


# ---- the roll-out entry points (a network: GPU tier; the emulator has no persistent kernels and refuses every flag) ---------------------------

def make_net(lib, device, seed=0):
    from humor_amd import synth
    from humor_amd.humor_model import HumorModel
    hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', latent_size=48, model_data_config='smpl+joints+contacts', steps_in=1, _lib_override=lib)
    hm.load_state_dict(synth.contractive_state_dict(seed))
    hm = hm.to(device).eval()
    for p in hm.parameters():
        p.requires_grad_(False)
    return hm, hm._net_handle(device)


def _rollout_buffers(lib, h, device, B, S, seed=0):
    r = _rand(device, seed)
    n = C.c_int64()
    lib.call('ha_humor_rollout_workspace', h.ptr, B, S, C.byref(n))
    past = torch.zeros(B, 339, device=device)
    eye = torch.eye(3, device=device).reshape(9)
    past[:, 6:15] = eye
    past[:, 18:207] = eye.repeat(21)
    past[:, 207:273] = r(B, 66, sc=0.3)
    return dict(past=past.contiguous(), z=r(B, S, ZD, sc=0.5), world=torch.empty(B, S, 348, device=device), pm=torch.empty(B, S, ZD, device=device),
                pv=torch.empty(B, S, ZD, device=device), stash=torch.empty(n.value, device=device), g_world=r(B, S, 348, sc=0.1),
                g_pm=r(B, S, ZD, sc=0.1), g_pv=r(B, S, ZD, sc=0.1), g_past=torch.empty(B, 339, device=device), g_z=torch.empty(B, S, ZD, device=device))


def _fwd(lib, h, b, B, S, flags=0):
    p = _lib.ptr
    lib.call('ha_humor_rollout_forward_fl', h.ptr, B, S, p(b['past']), p(b['z']), p(b['world']), p(b['pm']), p(b['pv']), p(b['stash']), flags, _stream(b['z']))


def _bwd(lib, h, b, B, S, flags=0):
    p = _lib.ptr
    lib.call('ha_humor_rollout_backward_fl', h.ptr, B, S, p(b['z']), p(b['g_world']), p(b['g_pm']), p(b['g_pv']), p(b['stash']), p(b['g_past']), p(b['g_z']),
             None, flags, _stream(b['z']))


def check_flag_refusals(lib, device, h, persistent, B=2, S=3):
    """A call flagged "cleared" / "laid out" for a workspace no launch has treated, and a call after partials were left unreduced and never picked
    up, return an error from the host entry point -- before any launch.  Without the persistent kernels every flag is refused."""
    import pytest
    b = _rollout_buffers(lib, h, device, B, S)
    n0 = launches(lib)
    with pytest.raises(_lib.HumorAmdError, match='HA_ROLL_CLEARED'):
        _fwd(lib, h, b, B, S, _lib.ROLL_CLEARED)
    assert launches(lib) == n0
    _fwd(lib, h, b, B, S)
    n0 = launches(lib)
    for fl, word in ((_lib.ROLL_CLEARED, 'HA_ROLL_CLEARED' if persistent else 'flags'), (_lib.ROLL_LAID_OUT, 'HA_ROLL_LAID_OUT' if persistent else 'flags'),
                     (8, 'unknown flag')):
        with pytest.raises(_lib.HumorAmdError, match=word):
            _bwd(lib, h, b, B, S, fl)
    if not persistent:
        with pytest.raises(_lib.HumorAmdError, match='flags'):
            _bwd(lib, h, b, B, S, _lib.ROLL_DEFER_DZ)
        assert launches(lib) == n0
        return
    assert launches(lib) == n0
    # a mark is good for one call: cleared once, claimed twice
    t = _lib.TurnTasks()
    lib.call('ha_humor_rollout_turn_tasks', h.ptr, B, S, _lib.ptr(b['stash']), 1, C.byref(t))
    assert t.flags == _lib.ROLL_CLEARED | _lib.ROLL_LAID_OUT | _lib.ROLL_DEFER_DZ and t.clr and t.lay_dst and t.dz_part and t.dz_slots == DZ_SLOTS
    # partials left unreduced and never picked up: the next entry point on the network says so, once
    _bwd(lib, h, b, B, S, _lib.ROLL_DEFER_DZ)
    n0 = launches(lib)
    with pytest.raises(_lib.HumorAmdError, match='unreduced'):
        _fwd(lib, h, b, B, S)
    assert launches(lib) == n0
    _fwd(lib, h, b, B, S)
    _bwd(lib, h, b, B, S)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(b['g_z']).all())


def check_entry_points_with_riders(lib, device, h, B, S, seed=0):
    """The roll-out entry points with every rider done by the neighbouring launches (the kernel-level form of what the stage-3 nodes do) against
    the plain calls: world, prior outputs, dL/dpast_in0 and dL/dz bit for bit; the persistent error word stays 0."""
    b = _rollout_buffers(lib, h, device, B, S, seed)
    r = _rand(device, seed + 1)
    add = r(B, S, ZD, sc=0.1)
    _fwd(lib, h, b, B, S)
    p = _lib.ptr
    lib.call('ha_humor_rollout_backward_fl', h.ptr, B, S, p(b['z']), p(b['g_world']), p(b['g_pm']), p(b['g_pv']), p(b['stash']), p(b['g_past']), p(b['g_z']),
             p(add), 0, _stream(add))
    ref = {k: b[k].clone() for k in ('world', 'pm', 'pv', 'g_past', 'g_z')}
    for k in ref:
        b[k].fill_(float('nan'))
    ins = _fit_pre_inputs(r, B, device)
    o = {k: torch.empty((B,) + sh, dtype=torch.float32, device=device) for k, sh in dict(**PRE_OUT, **PRE_GRAD).items()}

    def pre():
        a = _lib.FitPreArgs()
        a.B = B
        for k, v in dict(**ins, **o).items():
            setattr(a, k, v.data_ptr())
        return a
    st = _stream(add)
    t = _lib.TurnTasks()
    lib.call('ha_humor_rollout_turn_tasks', h.ptr, B, S, p(b['stash']), 0, C.byref(t))
    assert t.flags == _lib.ROLL_CLEARED
    a = pre()
    a.clr, a.clr_words = t.clr, t.clr_words
    lib.call('ha_fit_pre_forward', C.byref(a), st)
    _fwd(lib, h, b, B, S, _lib.ROLL_CLEARED)
    lib.call('ha_humor_rollout_turn_tasks', h.ptr, B, S, p(b['stash']), 1, C.byref(t))
    assert t.flags == _lib.ROLL_CLEARED | _lib.ROLL_LAID_OUT | _lib.ROLL_DEFER_DZ
    # the post launch on a problem of its own shape B x S (its outputs are not looked at here: check_post_merged does)
    from oracle import lbs_restated as L
    T = S + 1
    cpu = _rand(torch.device('cpu'), seed + 2)
    world = cpu(B, S, 348, sc=0.5)
    world[:, :, 6:15] = L.batch_rodrigues(cpu(B * S, 3, sc=1.5)).reshape(B, S, 9)
    world[:, :, 18:207] = L.batch_rodrigues(cpu(B * S * 21, 3, sc=0.8)).reshape(B, S, 189)
    new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=device)
    pa = _lib.RolloutPostArgs()
    pa.B, pa.S = B, S
    keep = dict(world=world.to(device), trans0=r(B, 3), root_orient=r(B, T, 3), contacts_conf=r(B, T, 22).sigmoid(), g_world=new(B, S, 348), g_trans0=new(B, 3),
                g_root0=new(B, 3), g_pose0=new(B, 63), g_joints0=new(B, 22, 3), partial=new(B * T, 15))
    for k, v in keep.items():
        setattr(pa, k, v.data_ptr())
    pa.lay_g_mu, pa.lay_g_var = b['g_pm'].data_ptr(), b['g_pv'].data_ptr()
    pa.lay_pri_out, pa.lay_dst, pa.lay_step_stride, pa.lay_RT, pa.lay_pad = t.lay_pri_out, t.lay_dst, t.lay_step_stride, t.lay_RT, t.lay_pad
    pa.clr, pa.clr_words = t.clr, t.clr_words
    lib.call('ha_rollout_post_backward', C.byref(pa), st)
    _bwd(lib, h, b, B, S, t.flags)
    a = pre()
    a.dz_part, a.dz_slots, a.dz_g_z, a.dz_g_z_add, a.dz_B, a.dz_S = t.dz_part, t.dz_slots, b['g_z'].data_ptr(), add.data_ptr(), B, S
    lib.call('ha_fit_pre_backward', C.byref(a), st)
    torch.cuda.synchronize()
    for k, v in ref.items():
        assert bool(torch.isfinite(b[k]).all()), k
        assert bits_equal(b[k], v), k
    avail, err, n = C.c_int(), C.c_uint(), C.c_int64()
    lib.call('ha_humor_persist_status', h.ptr, C.byref(avail), C.byref(err), C.byref(n))
    assert avail.value == 1 and err.value == 0, (avail.value, hex(err.value))


# ---- whole stage-3 closures (GPU tier) ---------------------------------------------------------------------------------------------------------

def run_closure(lib, dev, npz, B, T, graphs, reps=4, seed=1):
    """MotionOptimizer's stage-3 closure at B x T, `reps` evaluations with every variable changed in place between them.  Returns the loss and the
    nine gradients of each evaluation, and the library launches of the last eager evaluation (None under hipGraph replay)."""
    import fitting_checks as FC
    from oracle import closure_cases as CC
    case = CC.make_case('rgb', B, T, seed=seed)
    opt = FC.build(lib, dev, 'rgb', B, T, npz)
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
    out, count = [], None
    for _ in range(reps):
        n0 = launches(lib)
        loss = closure()
        if not graphs:
            count = launches(lib) - n0
        out.append((loss.detach().clone(), [p.grad.clone() for p in params]))
        with torch.no_grad():
            opt.latent_motion.add_(0.01)
            for p in params:
                p.mul_(1.0 + 2.0 ** -20)
        torch.cuda.synchronize()
        status = opt.motion_prior.persistent_rollout_status(dev)
        assert status[1] == 0, ('persistent error word', hex(status[1]))
    assert not getattr(opt, 'graph_failures', 0), 'the closure fell back to eager launches'
    return out, count


def assert_same_evaluations(got, want, what):
    assert len(got) == len(want)
    for i, ((l1, g1), (l0, g0)) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(l1)) and bits_equal(l1, l0), (what, i, l1.item(), l0.item())
        assert len(g1) == len(g0) == 9
        for j, (a, b) in enumerate(zip(g1, g0)):
            assert bool(torch.isfinite(a).all()) and bits_equal(a, b), (what, 'evaluation', i, 'gradient', j)
