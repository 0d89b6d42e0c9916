"""The committed float64 records under tests/golden/oracle/ are what the reference code computes.  No GPU.

(a) Every record of the step kinds (step, tab, coef, inv, bal, causal, gradnorm, sys and their training replays) is
accepted by conftest.cached_oracle on the inputs the job lists build today: the key exists and the inputs' digest
matches.  Only inputs are built, so no oracle runs; a GPU run that fell back to recomputing would otherwise only show
as a slow suite.

(b) A fixed list of small records goes through its real ``compute()`` and is compared array by array with the stored
one: max |new - stored| <= 1e-12 max(1, max |stored|).  The bound: the parent of the commit that introduced this test
reproduced every record of the list bit for bit on the CPU, except the three gradient-norm step records at 7e-17 to
1.7e-16 of that scale (threaded reductions in torch); a reassociated float64 sum over a few thousand terms stays below
1e-12, and the GPU tolerances that consume the records are 1e-4 and 2e-4.  A larger gap means a formula changed.  Each
record of the list takes 0.02 to 1.2 s (12 s together); the one ``causal`` record (n = 9, 48 s) is left to (a)."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, cached_oracle

_spec = importlib.util.spec_from_file_location("make_oracle_cache", os.path.join(GOLDEN, "make_oracle_cache.py"))
driver = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(driver)

KINDS = ("step", "tab", "tabtrain", "coef", "coeftrain", "inv", "invtrain", "bal", "baltrain", "causal", "causaltrain",
         "gradnorm", "gradnormtrain", "sys", "systrain")
N_RECORDS = 180
TOL = 1e-12

RECOMPUTED = (
    "step_cross_mesh_n1_L1_s1_angle_r12_i6_b7",
    "step_cascade_n2_L1_s1_angle_r64_i30_b33",
    "step_cascade_n2_L1_s1_angle_r64_i30_b33_drop_res",
    "step_cascade_n2_L1_s1_angle_r64_i30_b33_drop_unit",
    "step_cascade_n4_L1_s1_angle_r70_i30_b20_swap_haar",
    "tab_cascade_n2_L1_angle_r65_i1_b64",
    "tab_cascade_n4_L1_angle_r70_i30_b20",
    "tab_cascade_n3_L2_angle_r0_i70_b75",
    "tab_cascade_n4_L1_amplitude_r40_i10_b10",
    "tab_cascade_n4_L1_angle_r70_i30_b20_roll_val",
    "tabtrain_cascade4",
    "coef_cascade_n2_L1_angle_r65_i1_b64",
    "coef_cascade_n4_L1_angle_r70_i30_b20_roll",
    "coeftrain_cascade4",
    "inv_cascade_n2_L1_angle_r65_i1_b64",
    "inv_cascade_n4_L1_angle_r70_i30_b20_sign_dxx",
    "inv_uniform_c3_reg_cascade4",
    "invtrain_cascade4",
    "invtrain_cascade4_hold",
    "bal_cascade_n2_L1_angle_r65_i1_b64",
    "baltrain_cascade4",
    "baltrain_cascade4_hold",
    "causaltrain_cascade2_b128m2",
    "causaltrain_cascade2_b128m2_unit",
    "gradnorm_reg_cascade2",
    "gradnorm_reg_cascade4",
    "gradnorm_analytic",
    "gradnorm_coef",
    "gradnormtrain_cascade4_h16",
    "gradnormtrain_cascade4_h16_unit",
    "sys_cascade_n4_L1_angle_r20_i0_b0_K3",
    "sys_cascade_n4_L1_angle_r70_i30_b20_K3_drop_px",
    "systrain_cascade4_K3",
)


@pytest.fixture(scope="module")
def records():
    """key -> Record of every job of the step kinds (the adaptive-sampling records are another kind)."""
    return {r.key: r for r in driver.record_jobs() if r.key.split("_")[0] in KINDS}


def _refuse():
    raise AssertionError("the committed record was not accepted")


def test_every_record_of_the_step_kinds_is_accepted(records, monkeypatch):
    monkeypatch.delenv("QC_WRITE_ORACLE_CACHE", raising=False)
    assert len(records) == N_RECORDS
    assert {k.split("_")[0] for k in records} == set(KINDS)
    on_disk = {f[:-4] for f in os.listdir(os.path.join(GOLDEN, "oracle")) if f.split("_")[0] in KINDS}
    assert on_disk == set(records)
    for r in records.values():
        out = cached_oracle(r.key, r.inputs, _refuse)
        assert out and all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in out.values()), r.key


@pytest.mark.parametrize("key", RECOMPUTED)
def test_small_records_are_what_the_code_computes(key, records, monkeypatch):
    monkeypatch.delenv("QC_WRITE_ORACLE_CACHE", raising=False)
    r = records[key]
    stored = cached_oracle(r.key, r.inputs, _refuse)
    new = r.compute()
    assert set(new) == set(stored)
    for name, want in stored.items():
        got, want = np.asarray(new[name], dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, name
        if want.size:
            ratio = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            print(f"{key} {name}: {ratio:.2e}")
            assert ratio <= TOL, (name, ratio)
