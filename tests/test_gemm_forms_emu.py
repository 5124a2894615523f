"""CPU tier (SIMT emulator) of the batched GEMM's forms x epilogues, each forced and confirmed through the plan query:
tests/gemm_forms_checks.py.  Also the two tests that need no kernel at all: the union of the table's claims and the policy's documented
decisions."""
import pytest
import torch

import gemm_forms_checks as GF

CPU = torch.device('cpu')


@pytest.mark.parametrize('c', [pytest.param(c, marks=pytest.mark.slow) if c['slow'] else c for c in GF.CASES], ids=lambda c: c['name'])
def test_emu_gemm_form_against_fp64(emu_lib, c):
    """One entry of the table: the claimed forms confirmed by ha_debug_gemm_plan, then finite / deterministic / NaN tails / fp64 bars / the
    bitwise relations (gemm_forms_checks.check_case)."""
    GF.check_case(emu_lib, CPU, c)


@pytest.mark.slow
@pytest.mark.parametrize('B,S', [(5, 3), (70, 3)])
def test_emu_gemm_rm2_prior_shaped_store(emu_lib, B, S):
    """The mean | exp(log-variance) store over S > 1 steps behind RM 2: a roll-out on the launch chain (the cheapest path here; the prior's
    batched launches are the same on every path) under gemm_rm 2 against gemm_rm 1 and gemm_fold 0, bit for bit.  70 x 3: three row tiles
    per step, a row group of two tiles straddles a step boundary.  Four roll-outs each, 2-4 and 10-15 minutes on the emulator: slow here,
    unmarked in the GPU tier (tests/test_gemm_forms_gpu.py::test_gemm_rm2_prior_shaped_store)."""
    emu_lib.call('ha_tune_set', b'rollout_persist', 0)
    try:
        GF.check_rollout_case(emu_lib, CPU, B, S, seed=B + S)
    finally:
        emu_lib.call('ha_tune_set', b'rollout_persist', 1)


def test_gemm_forms_table_covers_every_form_and_epilogue():
    """The union of what the table's entries claim (each claim is asserted against the hook when its entry runs) is exactly the set of
    (form, epilogue) cells the kernel is instantiated for: a cell that drops out of the table fails here."""
    got = GF.claimed()
    assert got == GF.REQUIRED, f'missing {sorted(GF.REQUIRED - got)}, unexpected {sorted(got - GF.REQUIRED)}'
    # and the not-slow part of the CPU tier alone covers every cell too
    quick = {cl for c in GF.CASES if not c['slow'] for cl in c['claims']}
    assert quick == GF.REQUIRED, f'only slow entries cover {sorted(GF.REQUIRED - quick)}'


def test_gemm_policy_documented_decisions(emu_lib):
    """plan_prior_gemm under the default knobs: the form column of DESIGN.md section 7's table of the sixteen launches of one evaluation,
    RM 2 at C5 size and RM 1 just below each threshold.  A change that moves the policy has to edit gemm_forms_checks.SIXTEEN on purpose."""
    GF.check_policy(emu_lib)


def test_gemm_launch_unsplit_agrees_with_the_plan(emu_lib):
    GF.check_launch_unsplit_agrees(emu_lib)
