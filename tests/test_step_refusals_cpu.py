"""Every refusal of the ten qc_fused_pinn_*_step entry points keeps its code and its precedence: the table of
tests/step_refusal_cases.py against tests/golden/step_refusals.json, recorded before the entry points were routed through one
step plan (tests/golden/make_step_refusals.py).

The baseline row of each entry passes validation, and with a GPU it would go on into a step on made-up addresses: the table is
evaluated only where no GPU is visible, and the test skips itself where one is."""
import json
import os

import pytest
import torch

import step_refusal_cases as S
from conftest import GOLDEN, pkg


def test_every_refusal_keeps_its_code():
    if torch.cuda.is_available():
        pytest.skip("the rows pass made-up device addresses: evaluated only where no GPU is visible")
    with open(os.path.join(GOLDEN, "step_refusals.json")) as f:
        want = json.load(f)
    got = S.evaluate(pkg("hip.lib").load())
    rows = lambda table: [(r["entry"], r["faults"], r["phases"]) for r in table]
    assert rows(got) == rows(want)
    # the fixture is a refusal table: QC_OK for the baseline of each of the ten entries, a refusal in every other row
    assert sorted(r["entry"] for r in want if not r["faults"]) == sorted(S.ENTRIES) and len(S.ENTRIES) == 10
    assert all(r["code"] in ((S.ERR_ARG, S.ERR_UNSUPPORTED) if r["faults"] else (S.OK,)) for r in want)
    assert any(r["code"] == S.ERR_UNSUPPORTED and len(r["faults"]) == 2 for r in want)
    differ = [(g, w["code"]) for g, w in zip(got, want) if g["code"] != w["code"]]
    assert not differ, differ
