"""The fused step's post stage around its tile geometry, against the float64 step reference (tests/step_reference.py).

In the fused post stage a residual tile is one block of four waves, and a value tile (BC / IC points, value channel only)
is one block of four waves as well, each on a quarter of the hidden units (csrc/qc_mlp.hip, k_post_fused_value_body; the
value blocks follow the residual blocks in the merged launch).  The cases put the value-point count on both sides of the
tile edges: 0, 1, 63, 64, 65, 127, 128, 129, 191 and 257, with the IC / BC split inside a tile.  The residual count is
0, 1, 65 or the benchmark's 65 536; H and n cover the widths and qubit counts whose post stage the fused kernel serves
(H <= 128; n = 2 through the interpreter's two-stream form, n = 4 and 5 through the merged launches).  Tolerances are those of test_gpu_fused_families.py.

The same cases run again in child processes under QC_POST_SPLIT=1 (point kernel + weight-gradient kernel, the pair
the fused kernel replaced) and QC_NO_MERGE=1 (the standalone value launch), and one case compares the fused
kernel's gradient with the split pair's directly."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import pkg
from step_reference import step_inputs, step_record
from test_gpu_fullsize import Log, base_args, grads_for

pytestmark = pytest.mark.gpu

TOL_G, TOL_L = 2e-4, 1e-4

# id -> (ansatz, n, H, B_res, n_ic, n_bc); every (ansatz, n, counts) is distinct, so each case has its own oracle record
CASES = {
    "v0": ("cascade", 4, 50, 65, 0, 0),
    "v1": ("cascade", 4, 50, 1, 1, 0),
    "v63": ("cascade", 4, 50, 0, 30, 33),
    "v64": ("cascade", 4, 50, 65, 32, 32),
    "v65": ("cascade", 4, 50, 1, 40, 25),
    "v127": ("cascade", 4, 50, 65, 64, 63),
    "v128": ("cascade", 4, 50, 0, 0, 128),
    "v129": ("cascade", 4, 50, 65, 129, 0),
    "v191": ("cascade", 4, 50, 1, 100, 91),
    "v257": ("cascade", 4, 50, 65, 128, 129),
    "r65536_v257": ("cascade", 4, 50, 65536, 129, 128),
    "h1_v129": ("cascade", 4, 1, 65, 60, 69),
    "h65_v191": ("cascade", 4, 65, 65, 91, 100),
    "h128_v257": ("cascade", 4, 128, 1, 130, 127),
    "n2_v129": ("cascade", 2, 50, 65, 70, 59),
    "n2_h128_v65": ("cascade", 2, 128, 0, 33, 32),
    "n5_v191": ("alternate", 5, 50, 65, 95, 96),
    "n5_h65_v63": ("cascade", 5, 65, 1, 63, 0),
}
SUBSET = ("v1", "v65", "v129", "v257", "h65_v191", "n2_v129", "n5_v191")   # rerun under the library's switches


def case_inputs(case):
    ans, n, H, B_res, n_ic, n_bc = CASES[case]
    n_theta = pkg("circuits").params_per_layer(ans, n)
    return step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=4)


def case_job(case):
    ans, n, H, *_ = CASES[case]
    return step_record(ans, n, 1, 1, "angle", *case_inputs(case), H=H)


def case_reference(case):
    return case_job(case).get()


def oracle_jobs():
    return [case_job(c) for c in CASES]


def case_grads(case, gpu_device):
    ans, n, H, *_ = CASES[case]
    flat, X_ic, X_bc, X_res = case_inputs(case)
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, q_ansatz=ans, classic_network=[3, H, 1], encoding="angle"), Log(),
                   device=gpu_device)
    eng = model._engine_for(gpu_device)
    with torch.no_grad():
        eng.flat.copy_(torch.from_numpy(np.asarray(flat, dtype=np.float32)))
    got = grads_for(model, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)
    return got, eng.n_theta


@pytest.mark.parametrize("case", list(CASES))
def test_post_value_geometry_matches_fp64(case, gpu_device):
    ans, n, H, *_ = CASES[case]
    ref = case_reference(case)
    got, n_theta = case_grads(case, gpu_device)
    assert np.isfinite(got).all()
    lay = pkg("hip.engine").param_layout(H, n, n_theta)
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    assert got.size == NP + 3
    for name, s in {"pre": slice(0, o_post), "post": slice(o_post, o_th), "theta": slice(o_th, NP)}.items():
        if s.stop > s.start:
            want = ref["grad"][s]
            err = np.abs(got[s] - want).max() / (TOL_G * max(1.0, np.abs(want).max()))
            assert err < 1.0, (name, err)
    parts = ref["parts"]
    assert np.abs(got[NP:] - parts).max() < TOL_L * max(1.0, np.abs(parts).max()), (got[NP:], parts)


def _child(env, code_or_args):
    return subprocess.run([sys.executable] + code_or_args, env=dict(os.environ, **env), capture_output=True, text=True,
                          timeout=900)


@pytest.mark.parametrize("env", [{"QC_POST_SPLIT": "1"}, {"QC_NO_MERGE": "1"}], ids=["post_split", "no_merge"])
def test_switch_variants_pass_the_same_checks(env):
    here = os.path.dirname(os.path.abspath(__file__))
    sel = "matches_fp64 and (" + " or ".join(f"[{c}]" for c in SUBSET) + ")"
    r = _child(env, ["-m", "pytest", os.path.join(here, "test_gpu_post_value_geometry.py"), "-m", "gpu", "-q", "-x",
                     "-k", sel])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(SUBSET)} passed" in r.stdout, r.stdout[-2000:]


def test_fused_post_matches_split_pair(gpu_device, tmp_path):
    """The fused kernel and the split pair (QC_POST_SPLIT=1, read once at load: a child process) on one batch with
    ragged residual and value tiles: same losses, gradients at rounding level."""
    case = "v257"
    got, _ = case_grads(case, gpu_device)
    here = os.path.dirname(os.path.abspath(__file__))
    out = tmp_path / "split.npy"
    code = (f"import sys; sys.path.insert(0, {here!r}); import numpy as np, torch; "
            f"import test_gpu_post_value_geometry as t; "
            f"np.save({str(out)!r}, t.case_grads({case!r}, torch.device('cuda', 0))[0])")
    r = _child({"QC_POST_SPLIT": "1"}, ["-c", code])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    split = np.load(out)
    scale = max(1.0, np.abs(split).max())
    assert np.abs(got - split).max() < 1e-5 * scale, np.abs(got - split).max() / scale
