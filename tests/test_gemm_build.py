"""CPU tier: static check of the compiled batched GEMM (prior_gemm_kernel<RM, KS, TN>, humor_amd/csrc/rollout.hip; hipcc cross-compiles
gfx950 without a GPU).  The epilogue holds its operands (gamma, beta, bias, hsrc) in registers next to the tile; the condition of the
change that put them there is that no instantiation spills and that the one-row-tile forms keep the register bracket of two waves per
SIMD, which the launches between 1024 and 2048 waves run at."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_batched_gemm_forms_have_no_scratch_and_keep_their_occupancy(tmp_path):
    src = os.path.join(ROOT, 'humor_amd', 'csrc', 'rollout.hip')
    out = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '--cuda-device-only', '-S',
                          '-Rpass-analysis=kernel-resource-usage', '-o', str(tmp_path / 'rollout.s'), src], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    forms = {}
    name = None
    for line in out.stderr.split('\n'):
        m = re.search(r'Function Name: _ZN2ha17prior_gemm_kernelILi(\d)ELi(\d)ELi(\d)EEEvNS_8GemmTaskE', line)
        if m:
            name = tuple(int(v) for v in m.groups())
            forms[name] = {}
        elif 'Function Name:' in line:
            name = None
        elif name is not None:
            for key in ('VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]'):
                m = re.search(re.escape(key) + r': (\d+)', line)
                if m:
                    forms[name][key] = int(m.group(1))
    print(forms)
    assert sorted(forms) == [(1, 1, 1), (1, 1, 2), (1, 2, 1), (1, 2, 2), (1, 4, 1), (1, 4, 2), (2, 1, 2)], sorted(forms)
    for f, r in forms.items():
        assert r['ScratchSize [bytes/lane]'] == 0, (f, r)
        if f[0] == 1:
            assert r['Occupancy [waves/SIMD]'] >= 2, (f, r)
