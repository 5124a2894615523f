"""Shared checks of HumorModel(model_use_smpl_joint_inputs=True, smplh_path=...): the roll-out that feeds every step the SMPL+H joints of its
own prediction (reference humor_model.py:210-227, 894-954), forward only, through ha_humor_rollout_smpl_joints.  Run on the GPU
(test_smpl_joint_inputs_gpu.py) and on the host SIMT emulator (test_smpl_joint_inputs_emu.py).

Reference values: tests/golden/rollout_smpl_joints.npz, written by tools/make_golden_smpl_joint_inputs.py from the unmodified reference.  The
bar is the flat forward bar of the roll-out tests (rollout_checks.FWD_TOL = 1e-4 absolute); the generator measured how far the reference's
own outputs move under a 1e-7 relative perturbation of the initial state (stored per case, all below 1e-6), two orders below the bar.
"""
import atexit
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from humor_amd import synth
from humor_amd.humor_model import HumorModel
from rollout_checks import FWD_TOL, KEYS, world_of

GENDERS = ['male', 'female', 'neutral']
NAMES = KEYS[:-1]
DIMS = [3, 3, 9, 3, 189, 66, 66]
FIXTURE = 'rollout_smpl_joints.npz'
# case -> (input prefix, roll_out options)
CASES = {
    'b5_given': ('b5', dict(mode='given')),
    'b5_mean': ('b5', dict(mode='mean')),
    'b5_sampled': ('b5', dict(mode='sampled')),
    'b33_given': ('b33', dict(mode='given')),
    'b1_canon': ('b1', dict(mode='given', canon=True)),
}
_cache = {}


def smplh_root():
    """Directory with male|female|neutral/model.npz: the synthetic SMPL+H files of the fixture's seeds, written once per process."""
    if 'root' not in _cache:
        gd = golden(FIXTURE)
        root = tempfile.mkdtemp(prefix='smplh_genders_')
        atexit.register(shutil.rmtree, root, ignore_errors=True)
        for g, seed in zip(GENDERS, gd['gender_seeds']):
            os.makedirs(os.path.join(root, g))
            synth.write_smplh_npz(os.path.join(root, g, 'model.npz'), seed=int(seed))
        _cache['root'] = root
    return _cache['root']


def state_dict():
    return synth.humor_state_dict(int(golden(FIXTURE)['weight_seed']), **synth.CONTRACTIVE)


def make_model(lib, device, feedback=True, batch=64):
    kw = dict(model_use_smpl_joint_inputs=True, model_smpl_batch_size=batch, smplh_path=smplh_root()) if feedback else {}
    hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', latent_size=48, model_data_config='smpl+joints+contacts', steps_in=1,
                    _lib_override=lib, **kw)
    hm.load_state_dict(state_dict())
    return hm.to(device).eval()


def as_dict(past, device):
    d, o = {}, 0
    for k, n in zip(NAMES, DIMS):
        d[k] = past[:, o:o + n].unsqueeze(1).to(device)
        o += n
    return d


def fixture_inputs(prefix, rows=None, steps=None):
    gd = golden(FIXTURE)
    sl = slice(None) if rows is None else slice(0, rows)
    t = lambda k: torch.from_numpy(gd[f'{prefix}_{k}'][sl])
    past, betas, z = t('past'), t('betas'), t('z_in')
    eps = t('eps') if f'{prefix}_eps' in gd.files else None
    genders = [GENDERS[i] for i in gd[f'{prefix}_gender'][sl]]
    if steps is not None:
        z, eps = z[:, :steps], (None if eps is None else eps[:, :steps])
    return past, betas, z, eps, genders


def run(hm, device, past, S, genders, betas, z=None, eps=None, mode='given', canon=False):
    """-> world [B,S,348], prior_mu, prior_var, z (host tensors)."""
    kw = dict(return_prior=True, return_z=True, gender=genders, betas=None if betas is None else betas.to(device),
              canonicalize_input=canon, uncanonicalize_output=canon)
    if mode == 'given':
        kw['z_seq'] = z.to(device)
    elif mode == 'mean':
        kw['use_mean'] = True
    else:
        kw['eps_seq'] = eps.to(device)
    with torch.no_grad():
        out, (pm, pv) = hm.roll_out(None, as_dict(past, device), S, **kw)
    return world_of(out).cpu(), pm.cpu(), pv.cpu(), out['z'].cpu()


def check_fixture_case(lib, device, name, rows=None, steps=None):
    """World states, prior mean / variance and z over all steps against the reference's (optionally the first `rows` sequences and `steps`
    steps of the case: the sequences of a batch are independent and a step does not depend on later ones)."""
    gd = golden(FIXTURE)
    prefix, opt = CASES[name]
    past, betas, z, eps, genders = fixture_inputs(prefix, rows, steps)
    S = z.shape[1]
    hm = make_model(lib, device, batch=past.shape[0])
    world, pm, pv, z_out = run(hm, device, past, S, genders, betas, z=z, eps=eps, **opt)
    B = past.shape[0]
    figures = {}
    for key, got in (('world', world), ('prior_mu', pm), ('prior_var', pv), ('z', z_out)):
        ref = z.numpy() if (key == 'z' and opt['mode'] == 'given') else gd[f'{name}_{key}'][:B, :S]
        figures[key] = float(np.abs(got.numpy() - ref).max())
    print(f'{name} B={B} S={S}: max abs deviation from the reference {figures} (reference sensitivity {float(gd[name + "_dev"]):.1e})')
    assert torch.isfinite(world).all()
    for key, v in figures.items():
        assert v < FWD_TOL, (name, key, v)


def check_feedback_is_live(lib, device):
    """Step 1 is the plain roll-out's (the feedback enters with the second input); from step 2 on the two differ by more than 0.1."""
    past, betas, z, _, genders = fixture_inputs('b5')
    S = 4
    fb, _, _, _ = run(make_model(lib, device), device, past, S, genders, betas, z=z[:, :S])
    # the feedback runs on the launch chain: the plain roll-out it is compared with takes the same kernels
    lib.call('ha_tune_set', b'rollout_persist', 0)
    try:
        plain, _, _, _ = run(make_model(lib, device, feedback=False), device, past, S, None, None, z=z[:, :S])
    finally:
        lib.call('ha_tune_set', b'rollout_persist', 1)
    assert (fb[:, 0] - plain[:, 0]).abs().max().item() < 1e-6
    for t in range(1, S):
        assert (fb[:, t] - plain[:, t]).abs().max().item() > 0.1, t


def check_without_gender_is_plain(lib, device):
    """Flag on, gender / betas missing: the plain roll-out on the existing paths (humor_model.py:896)."""
    past, betas, z, _, genders = fixture_inputs('b5')
    S = 3
    hm = make_model(lib, device)
    plain, pm0, pv0, _ = run(make_model(lib, device, feedback=False), device, past, S, None, None, z=z[:, :S])
    for g, b in ((None, betas), (genders, None), (None, None)):
        w, pm, pv, _ = run(hm, device, past, S, g, b, z=z[:, :S])
        assert torch.equal(w, plain) and torch.equal(pm, pm0) and torch.equal(pv, pv0)


def check_batch_permutation(lib, device):
    past, betas, z, eps, genders = fixture_inputs('b5')
    S = 3
    perm = [3, 0, 4, 2, 1]
    hm = make_model(lib, device)
    for mode in ('given', 'sampled'):
        a = run(hm, device, past, S, genders, betas, z=z[:, :S], eps=eps[:, :S], mode=mode)
        b = run(hm, device, past[perm], S, [genders[i] for i in perm], betas[perm], z=z[perm][:, :S], eps=eps[perm][:, :S], mode=mode)
        for x, y in zip(a, b):
            assert (x[perm] - y).abs().max().item() < 1e-6, mode


def check_smpl_batch_size(lib, device):
    """A gender group above model_smpl_batch_size raises the reference's exception (humor_model.py:925); one that fits does not."""
    past, betas, z, _, genders = fixture_inputs('b5')       # two male, two female, one neutral
    with pytest.raises(Exception, match='SMPL model batch size not large enough to accomodate!'):
        run(make_model(lib, device, batch=1), device, past, 2, genders, betas, z=z[:, :2])
    run(make_model(lib, device, batch=2), device, past, 2, genders, betas, z=z[:, :2])


def check_gradient_is_refused(lib, device):
    past, betas, z, _, genders = fixture_inputs('b5', rows=2)
    hm = make_model(lib, device)
    kw = dict(gender=genders, betas=betas.to(device))
    p, zz = past.to(device), z[:, :2].to(device)
    with pytest.raises(NotImplementedError):
        hm.roll_out(p.clone().requires_grad_(True), None, 2, z_seq=zz, **kw)
    with pytest.raises(NotImplementedError):
        hm.roll_out(p, None, 2, z_seq=zz.clone().requires_grad_(True), **kw)
    with torch.no_grad():       # gradients switched off: served
        hm.roll_out(p.clone().requires_grad_(True), None, 2, z_seq=zz, **kw)


# ----------------------------------------------------------------------------------------------------
# no library needed
# ----------------------------------------------------------------------------------------------------
def check_constructor_and_state_dict():
    with pytest.raises(NotImplementedError, match='smplh_path'):
        HumorModel(in_rot_rep='mat', out_rot_rep='aa', model_use_smpl_joint_inputs=True)
    hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', model_use_smpl_joint_inputs=True, smplh_path='/nonexistent/never/probed')
    assert hm.use_smpl_joint_inputs and hm.ignore_keys == ['male_bm', 'female_bm', 'neutral_bm']
    sd = state_dict()
    for g in ('male_bm', 'female_bm', 'neutral_bm'):        # what a HuMoR-Qual checkpoint carries besides the networks
        sd[f'{g}.bm.shapedirs'] = torch.zeros(4, 3, 16)
        sd[f'{g}.bm.J_regressor'] = torch.zeros(52, 4)
    hm.load_state_dict(sd)
    assert torch.equal(hm.decoder.net[0].weight, sd['decoder.net.0.weight'])
    for combo in (dict(in_rot_rep='aa'), dict(steps_in=2), dict(out_rot_rep='6d'), dict(output_delta=False)):
        kw = dict(in_rot_rep='mat', out_rot_rep='aa', model_use_smpl_joint_inputs=True, smplh_path='/nonexistent/never/probed')
        kw.update(combo)
        m = HumorModel(**kw)
        with pytest.raises(NotImplementedError, match='released configuration'):
            m.roll_out(torch.zeros(1, m.steps_in, m.input_data_dim), None, 2, z_seq=torch.zeros(1, 2, 48), gender=['male'],
                       betas=torch.zeros(1, m.steps_in, 16))


def batch_data(B, T, steps_in=1, seed=0):
    """A data-loader batch as the reference's dataset hands it over: (data_in, data_out) with [B, T, steps, ...] entries, data_out also
    holding the global_* copies [B, T, ...]."""
    g = torch.Generator().manual_seed(seed)
    shapes = {'trans': (3,), 'trans_vel': (3,), 'root_orient': (9,), 'root_orient_vel': (3,), 'pose_body': (21, 9), 'joints': (22, 3),
              'joints_vel': (22, 3), 'contacts': (9,)}
    data_in = {k: torch.randn(B, T, steps_in, *s, generator=g) for k, s in shapes.items()}
    data_out = {k: torch.randn(B, T, 1, *s, generator=g) for k, s in shapes.items()}
    data_out.update({'global_' + k: torch.randn(B, T, *s, generator=g) for k, s in shapes.items()})
    return data_in, data_out


def check_prepare_input_structure():
    B, T = 2, 3
    hm = HumorModel(in_rot_rep='mat', out_rot_rep='aa', model_data_config='smpl+joints+contacts')
    data_in, data_out = batch_data(B, T)
    cpu = torch.device('cpu')
    x = hm.prepare_input(data_in, cpu)
    assert x.shape == (B, T, 1, 339)
    x2, d_in = hm.prepare_input(data_in, cpu, return_input_dict=True)
    assert torch.equal(x, x2) and list(d_in) == hm.data_names
    # return_global_dict without data_out has nothing to return (humor_model.py:310-314)
    assert torch.equal(hm.prepare_input(data_in, cpu, return_global_dict=True), x)
    r3 = hm.prepare_input(data_in, cpu, data_out=data_out)
    r4 = hm.prepare_input(data_in, cpu, data_out=data_out, return_input_dict=True)
    r4g = hm.prepare_input(data_in, cpu, data_out=data_out, return_global_dict=True)
    r5 = hm.prepare_input(data_in, cpu, data_out=data_out, return_input_dict=True, return_global_dict=True)
    assert [len(r) for r in (r3, r4, r4g, r5)] == [3, 4, 4, 5] and all(isinstance(r, tuple) for r in (r3, r4, r4g, r5))
    x_past, x_t, gt, d_in, glob = r5
    assert torch.equal(x_past, x) and x_t.shape == (B, T, 1, 339)
    assert torch.equal(x_t, torch.cat([data_out[k].reshape(B, T, 1, -1) for k in hm.data_names], 3))
    # the auxiliary output (contacts) is in the dictionaries, not in x_t
    assert list(gt) == hm.data_names + ['contacts'] and list(glob) == list(gt) and list(r4g[3]) == list(gt)
    assert 'contacts' not in d_in
    for k in gt:
        assert gt[k].shape == (B, T, 1, data_out[k][0, 0].numel())
        assert glob[k].shape == gt[k].shape
        assert torch.equal(glob[k], data_out['global_' + k].reshape(B, T, 1, -1))
    # steps_in > 1 folds the input steps; the global entries are expanded over the output steps (one here)
    hm2 = HumorModel(in_rot_rep='mat', out_rot_rep='aa', model_data_config='smpl+joints', steps_in=2)
    data_in2, data_out2 = batch_data(B, T, steps_in=2, seed=1)
    xp, xt, gt2, glob2 = hm2.prepare_input(data_in2, cpu, data_out=data_out2, return_global_dict=True)
    assert xp.shape == (B, T, 2, 339) and xt.shape == (B, T, 1, 339) and 'contacts' not in gt2 and list(glob2) == hm2.data_names
    # aux input names, when a model declares them, join the input dictionary only
    hm.aux_in_data_names = ['contacts']
    xa, da = hm.prepare_input(data_in, cpu, return_input_dict=True)
    assert torch.equal(xa, x) and list(da) == hm.data_names + ['contacts'] and da['contacts'].shape == (B, T, 1, 9)


def _reference():
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip('reference tree not present')
    return ref_loader.load()


def check_prepare_input_vs_reference():
    R = _reference()
    cpu = torch.device('cpu')
    for cfg, steps_in in (('smpl+joints+contacts', 1), ('smpl+joints', 2)):
        kw = dict(in_rot_rep='mat', out_rot_rep='aa', latent_size=48, model_data_config=cfg, steps_in=steps_in)
        ours, ref = HumorModel(**kw), R.humor_model.HumorModel(**kw)
        data_in, data_out = batch_data(2, 3, steps_in=steps_in, seed=5)
        for opts in (dict(), dict(return_input_dict=True), dict(data_out=data_out), dict(data_out=data_out, return_input_dict=True),
                     dict(data_out=data_out, return_global_dict=True), dict(data_out=data_out, return_input_dict=True, return_global_dict=True)):
            a, b = ours.prepare_input(data_in, cpu, **opts), ref.prepare_input(data_in, cpu, **opts)
            assert type(a) is type(b)
            a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
            assert len(a) == len(b)
            for x, y in zip(a, b):
                if isinstance(y, dict):
                    assert list(x) == list(y)
                    for k in y:
                        assert x[k].shape == y[k].shape and torch.equal(x[k], y[k]), (opts, k)
                else:
                    assert x.shape == y.shape and torch.equal(x, y), opts


def _reference_tool():
    _reference()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_golden_smpl_joint_inputs as tool
    return tool


def check_qual_sampling_sequence(lib, device):
    """The caller of the Qual sampling config (test_humor.py:210-224) at B = 2: prepare_input(..., data_out, input dict, global dict) ->
    first step -> roll_out(x_past, dict, S, gender=, betas=), against the reference doing the same (prior mean, so that both draw nothing)."""
    tool = _reference_tool()
    R = _reference()
    past, betas, _, _, genders = fixture_inputs('b5', rows=2)
    B, T, S = 2, 3, 3
    data_in, data_out = batch_data(B, T, seed=9)
    for k, v in as_dict(past, torch.device('cpu')).items():        # a valid state at step 0, whatever the later steps hold
        data_in[k][:, 0] = v.reshape(data_in[k][:, 0].shape)
    ref = tool.reference_model(R, smplh_root(), B)
    ours = make_model(lib, device, batch=B)
    outs = []
    for model, dev in ((ref, torch.device('cpu')), (ours, device)):
        with torch.no_grad(), tool.numpy_int_alias():
            x_past, _, gt, d_in, glob = model.prepare_input(data_in, dev, data_out=data_out, return_input_dict=True, return_global_dict=True)
            first = {k: v[:, 0, :, :].clone() for k, v in d_in.items()}
            pred = model.roll_out(x_past[:, 0, :, :], first, S, use_mean=True, gender=genders, betas=betas.to(dev))
        outs.append(torch.cat([pred[k] for k in KEYS], 2).cpu())
    assert (outs[0] - outs[1]).abs().max().item() < FWD_TOL


def check_fixture_regenerates():
    """One case of the committed fixture from the reference, live: the fixture is what the generator writes."""
    tool = _reference_tool()
    R = _reference()
    gd = golden(FIXTURE)
    past, betas, z, _, genders = fixture_inputs('b1')
    hm = tool.reference_model(R, smplh_root(), 1)
    world, pm, pv, _ = tool.run(hm, past, z.shape[1], genders, betas, z=z, canon=True)
    # the same arithmetic on another host may round differently; the generator's own bar on the reference's sensitivity bounds that
    for key, got in (('world', world), ('prior_mu', pm), ('prior_var', pv)):
        assert np.abs(got.numpy() - gd[f'b1_canon_{key}']).max() < tool.DEV_BAR, key
