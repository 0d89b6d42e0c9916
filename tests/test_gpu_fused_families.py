"""The fused step (qc_fused_pinn_residual_step, QC_PHASE_GRADS) against the float64 reference in every circuit family:
the [grad | L_r, L_bc, L_ic] vector of the register family (2 <= n <= 5), the lanes-as-amplitudes family (n = 1 and
6..8) and the HBM family (n >= 9), through the compile-time programs and the run-time interpreters, in both encodings,
on batches with empty, ragged and shared tiles.

The reference is tests/step_reference.py (pinned to the reference's own nn/pde.py by tests/test_step_reference.py);
its outputs for the seeded inputs below are committed under tests/golden/oracle/ (tests/golden/make_oracle_cache.py).
Two HBM cases compare with the reference's own train() (train_*.npz) and config 5 (cross_mesh n = 16) with the
reference's own nn/pde.py (operator_cross_mesh_n16.npz).

The gradient is checked block by block (pre network, theta, post network), each at 2e-4 x max(1, max |ref block|), so an
error in the small theta block cannot hide under the scale of the MLP weights; the loss parts at 1e-4.  Negative
controls (the reference without the last residual point, without the last value point, with the two fixed unitaries
swapped) must fail the same tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg
from step_reference import layout_from_fixture, step_inputs, step_record
from test_gpu_fullsize import Log, base_args, grads_for

pytestmark = pytest.mark.gpu

H = 50
TOL_G, TOL_L = 2e-4, 1e-4
THETA_MIN = 20 * TOL_G          # max |ref theta| must clear this, so the theta check is not vacuous

# id -> (ansatz, n, L, encoding, B_res, n_ic, n_bc); the comment names the path the case reaches
CASES = {
    # register family: compile-time programs (cascade 4, farhi 4, alternate 5) in merged launches, and the interpreter
    "reg_cascade4": ("cascade", 4, 1, "angle", 70, 30, 20),          # static, merged; one value tile holds IC and BC
    "reg_farhi4": ("farhi", 4, 1, "angle", 33, 0, 17),               # static, merged; n_ic = 0
    "reg_alternate5": ("alternate", 5, 1, "angle", 40, 25, 0),       # static, merged; n_bc = 0
    "reg_sim_circ_15_5": ("sim_circ_15", 5, 1, "angle", 20, 0, 0),   # interpreter; B_val = 0 (two-stream form)
    "reg_cascade3_L2": ("cascade", 3, 2, "angle", 0, 70, 75),        # interpreter; B_res = 0, three value tiles
    # n = 1 (the lanes-as-amplitudes family's run-time interpreter)
    "n1_farhi": ("farhi", 1, 1, "angle", 10, 5, 6),                  # no trainable angle at all (n_theta = 0)
    "n1_cross_mesh": ("cross_mesh", 1, 1, "angle", 12, 6, 7),
    # lanes-as-amplitudes family, n = 6..8
    "wave_cascade6": ("cascade", 6, 1, "angle", 200, 60, 70),        # static, kept store; 4 residual tiles (ragged), 3 value
    "wave_layered7": ("layered", 7, 1, "angle", 65, 1, 40),          # static; 2 residual tiles, IC/BC in one tile
    "wave_cross_mesh8": ("cross_mesh", 8, 1, "angle", 20, 10, 10),   # static (phase-table run)
    "wave_alternate7": ("alternate", 7, 1, "angle", 30, 0, 30),      # interpreter; n_ic = 0
    "wave_farhi6": ("farhi", 6, 1, "angle", 0, 40, 40),              # interpreter; B_res = 0, 2 value tiles
    # HBM family, n >= 9
    "hbm_cascade9": ("cascade", 9, 1, "angle", 65, 3, 2),            # plan interpreter; 2 resident residual tiles, ragged
    "hbm_layered12_L2": ("layered", 12, 2, "angle", 2, 5, 0),        # plan interpreter; n_bc = 0
    "hbm_sim_circ_15_11": ("sim_circ_15", 11, 1, "angle", 3, 0, 4),  # plan interpreter; n_ic = 0
    "hbm_farhi10": ("farhi", 10, 1, "angle", 0, 70, 60),             # plan interpreter; value rows only, 3 value tiles
    "hbm_cross_mesh12": ("cross_mesh", 12, 1, "angle", 2, 3, 3),     # stage program (one stage), fused RZ runs
    "hbm_cross_mesh13": ("cross_mesh", 13, 1, "angle", 1, 2, 2),     # stage program (two stages)
    # amplitude encoding: the u / ub carve of the step workspace in every family
    "amp_cascade4": ("cascade", 4, 1, "amplitude", 40, 10, 10),
    "amp_layered6": ("layered", 6, 1, "amplitude", 20, 5, 5),
    "amp_cascade9": ("cascade", 9, 1, "amplitude", 2, 4, 3),
}
# negative controls: each reference must FAIL the tolerance ("swap_haar" on the theta block)
CONTROLS = {"reg_cascade4": ("drop_res", "drop_val", "swap_haar"), "wave_layered7": ("drop_val", "swap_haar"),
            "hbm_cross_mesh12": ("drop_res", "drop_val", "swap_haar")}
MERGED = ("reg_cascade4", "reg_farhi4", "reg_alternate5")     # register family, angle encoding, both pipelines
STATIC = ("reg_cascade4", "reg_farhi4", "reg_alternate5", "wave_cascade6", "wave_layered7", "wave_cross_mesh8",
          "hbm_cross_mesh12", "hbm_cross_mesh13")                # programs of gen_static.py's whitelist


def oracle_jobs():
    """Every committed record (tests/golden/make_oracle_cache.py)."""
    return [case_job(c) for c in CASES] + [case_job(c, v) for c, vs in CONTROLS.items() for v in vs] + [n16_value_job()]


def case_inputs(case):
    ans, n, L, enc, B_res, n_ic, n_bc = CASES[case]
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    return step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=1)


def case_job(case, variant=""):
    ans, n, L, enc, *_ = CASES[case]
    return step_record(ans, n, L, 1, enc, *case_inputs(case), H=H, variant=variant)._replace(case=case)


def case_reference(case, variant=""):
    return case_job(case, variant).get()


def _model(gpu_device, ans, n, L, enc, flat=None):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, encoding=enc), Log(), device=gpu_device)
    eng = model._engine_for(gpu_device)
    if flat is not None:
        with torch.no_grad():
            eng.flat.copy_(torch.from_numpy(np.asarray(flat, dtype=np.float32)))
    return model, eng


def _blocks(n, n_theta):
    lay = pkg("hip.engine").param_layout(H, n, n_theta)
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    return {"pre": slice(0, o_post), "theta": slice(o_th, NP), "post": slice(o_post, o_th)}


def _errors(got, want_g, n, n_theta):
    """block -> error / tolerance (< 1 passes)."""
    out = {}
    for name, s in _blocks(n, n_theta).items():
        if s.stop > s.start:
            out[name] = np.abs(got[s] - want_g[s]).max() / (TOL_G * max(1.0, np.abs(want_g[s]).max()))
    return out


def _check(got, ref, n, n_theta):
    NP = got.size - 3
    err = _errors(got[:NP], ref["grad"], n, n_theta)
    assert max(err.values()) < 1.0, err
    parts = ref["parts"]
    assert np.abs(got[NP:] - parts).max() < TOL_L * max(1.0, np.abs(parts).max()), (got[NP:], parts)
    if n_theta:
        th = np.abs(ref["grad"][_blocks(n, n_theta)["theta"]]).max()
        assert th > THETA_MIN, th


def _merged_probe(model, eng, Xs):
    """0 when the step takes the merged form (qc_fused_step_stage runs only there; the pre stage writes nothing the
    step reads before writing it)."""
    engine, L = pkg("hip.engine"), pkg("hip.lib")
    fs = engine.FusedStep(eng, Xs[2].shape[0], Xs[0].shape[0], Xs[1].shape[0], engine.OptimState(eng.NP, 0.005, eng.device))
    rc = eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_PRE_FWD, torch.cuda.current_stream(eng.device).cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", list(CASES))
def test_fused_step_matches_fp64(case, gpu_device):
    ans, n, L, enc, B_res, n_ic, n_bc = CASES[case]
    flat, X_ic, X_bc, X_res = case_inputs(case)
    ref = case_reference(case)
    model, eng = _model(gpu_device, ans, n, L, enc, flat)
    n_theta, lib, c = eng.n_theta, eng.lib, eng.circuit
    got = grads_for(model, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    _check(got, ref, n, n_theta)
    # the path
    hbm = int(lib.qc_circuit_workspace_bytes(c.handle, 6, 1)) > 0
    assert hbm == (n >= 9)
    # the kept store: the register family always, the wave family for its compile-time programs; the HBM tiles
    kept = int(lib.qc_step_workspace_bytes(c.handle, B_res, n_ic + n_bc)) > 0
    if B_res and (hbm or 2 <= n <= 5):
        assert kept
    elif B_res and 6 <= n <= 8 and enc == "angle":
        assert kept == (case in STATIC and os.environ.get("QC_NO_STATIC") != "1")
    if 2 <= n <= 5:
        merged = case in MERGED and os.environ.get("QC_NO_MERGE") != "1"
        assert (_merged_probe(model, eng, (X_ic, X_bc, X_res)) == 0) == merged
    # negative controls
    for v in CONTROLS.get(case, ()):
        bad = case_reference(case, v)
        err = _errors(got[:-3], bad["grad"], n, n_theta)
        if v == "swap_haar":
            assert err["theta"] > 1.0, (v, err)
        else:
            assert max(err.values()) > 1.0, (v, err)


def test_fused_step_without_kept_store_matches_fp64(gpu_device):
    """Register family with the store withheld (circ_ws_dev = None): the two-stream form, value pipeline on the side
    stream, forward recomputed in the adjoint pass."""
    L = pkg("hip.lib")
    engine = pkg("hip.engine")
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = CASES[case]
    flat, X_ic, X_bc, X_res = case_inputs(case)
    ref = case_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    eng.refresh_gates()
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, gpu_device))
    assert fs.desc.circ_ws_bytes > 0
    fs.desc.circ_ws_dev, fs.desc.circ_ws_bytes = None, 0
    assert eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_PRE_FWD, torch.cuda.current_stream(gpu_device).cuda_stream) != 0
    fs.X_res[:B_res] = X_res.to(gpu_device)
    fs.X_val[:n_ic] = X_ic.to(gpu_device)
    fs.X_val[n_ic:n_ic + n_bc] = X_bc.to(gpu_device)
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    _check(fs.flat_grad.cpu().numpy().astype(np.float64), ref, n, eng.n_theta)


TRAIN_FIXTURES = [("cross_mesh_n10_b72", "cross_mesh", 10, 1), ("layered_n8_b136", "layered", 8, 2)]


@pytest.mark.parametrize("tag,ans,n,L", TRAIN_FIXTURES, ids=[t[0] for t in TRAIN_FIXTURES])
def test_first_step_matches_reference_train(tag, ans, n, L, gpu_device):
    """First batch of the reference's own train(): the raw gradient and loss parts of its first step.  n = 10: the plan
    interpreter on two ragged residual tiles; layered 8: the wave family on three residual tiles."""
    z = np.load(os.path.join(GOLDEN, f"train_{tag}.npz"))
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    model, eng = _model(gpu_device, ans, n, L, "angle", layout_from_fixture(z, "w0__", H, n, n_theta))
    Xs = [torch.from_numpy(z[k][0]) for k in ("X_ic", "X_bc", "X_res")]
    got = grads_for(model, *Xs).cpu().numpy().astype(np.float64)
    _check(got, {"grad": z["grad_raw0"].astype(np.float64), "parts": z["parts"][0][1:]}, n, n_theta)


# ---- config 5: cross_mesh n = 16 against the reference's own nn/pde.py
N16 = "cross_mesh_n16_value"


def _n16_points():
    from oracle import solver as osol
    g = torch.Generator().manual_seed(16)
    return [(torch.tensor(b[0]) + (torch.tensor(b[1]) - torch.tensor(b[0])) * torch.rand(5, 3, generator=g)).to(torch.float32)
            for b in (osol.BOX_IC, osol.BOX_BC1)]


def n16_value_job():
    z = np.load(os.path.join(GOLDEN, "operator_cross_mesh_n16.npz"))
    n_theta = pkg("circuits").params_per_layer("cross_mesh", 16)
    X_ic, X_bc = _n16_points()
    return step_record("cross_mesh", 16, 1, 1, "angle", layout_from_fixture(z, "w__", H, 16, n_theta), X_ic, X_bc, X_ic[:0], H=H)


def n16_value_reference():
    """fp64 reference of the value points alone on the fixture's weights (cheap at n = 16: no derivative channels)."""
    return n16_value_job().get()


def test_config5_step_matches_reference_pde(gpu_device):
    z = np.load(os.path.join(GOLDEN, "operator_cross_mesh_n16.npz"))
    n_theta = pkg("circuits").params_per_layer("cross_mesh", 16)
    model, eng = _model(gpu_device, "cross_mesh", 16, 1, "angle", layout_from_fixture(z, "w__", H, 16, n_theta))
    X = torch.from_numpy(z["X"])
    none = X[:0]
    grad = z["grad"].astype(np.float64)
    got = grads_for(model, none, none, X).cpu().numpy().astype(np.float64)
    _check(got, {"grad": grad, "parts": np.array([0.5 * float(z["loss"]), 0.0, 0.0])}, 16, n_theta)
    # the same residual points plus IC and BC points: the value part from the fp64 reference
    X_ic, X_bc = _n16_points()
    val = n16_value_reference()
    got = grads_for(model, X_ic, X_bc, X).cpu().numpy().astype(np.float64)
    want = {"grad": grad + val["grad"], "parts": val["parts"] + np.array([0.5 * float(z["loss"]), 0.0, 0.0])}
    _check(got, want, 16, n_theta)


# ---- the step after an in-library update: gate tables, diagonal tables and HBM phase records refreshed by the
# optimiser kernel must equal those of a fresh model built on the updated weights
UPDATE_CASES = [("cascade", 4, 1, 70, 30, 20), ("layered", 8, 2, 40, 10, 10), ("cross_mesh", 12, 1, 2, 3, 3),
                ("cross_mesh", 16, 1, 2, 3, 2)]


@pytest.mark.parametrize("ans,n,L,B_res,n_ic,n_bc", UPDATE_CASES, ids=[f"{c[0]}{c[1]}" for c in UPDATE_CASES])
def test_step_after_update_matches_fresh_model(ans, n, L, B_res, n_ic, n_bc, gpu_device):
    Lb = pkg("hip.lib")
    engine = pkg("hip.engine")
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=2)
    model, eng = _model(gpu_device, ans, n, L, "angle", flat)
    eng.refresh_gates()
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.05, gpu_device))
    fs.X_res[:B_res] = X_res.to(gpu_device)
    fs.X_val[:n_ic] = X_ic.to(gpu_device)
    fs.X_val[n_ic:n_ic + n_bc] = X_bc.to(gpu_device)
    fs.run(Lb.QC_PHASE_GRADS | Lb.QC_PHASE_UPDATE)
    fs.run(Lb.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    g1 = fs.flat_grad.cpu().numpy().astype(np.float64)
    new = eng.flat.detach().cpu().numpy()
    th = slice(eng.theta_off, eng.theta_off + n_theta)
    assert np.abs(new[th] - flat[th]).max() > 1e-2            # the update moved theta (lr 0.05)
    model2, _ = _model(gpu_device, ans, n, L, "angle", new)
    g2 = grads_for(model2, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)
    scale = max(1.0, np.abs(g2).max())
    assert np.abs(g1 - g2).max() < 1e-6 * scale, np.abs(g1 - g2).max() / scale


# ---- the same checks with the library's switches (read once at load, hence a child process)
def _sel(cases):
    return "matches_fp64 and (" + " or ".join(cases) + ")"


@pytest.mark.parametrize("env,sel,count", [
    ({"QC_NO_STATIC": "1"}, _sel(STATIC), len(STATIC)),
    ({"QC_NO_MERGE": "1"}, "without_kept_store or " + _sel(MERGED + ("reg_sim_circ_15_5", "reg_cascade3_L2")), 6),
    ({"QC_H2S_RB": "3"}, _sel(("hbm_cross_mesh12",)) + " or after_update and cross_mesh12", 2),
    ({"QC_NO_ABSORB": "1"}, _sel(("hbm_cascade9", "hbm_cross_mesh12")), 2)],
    ids=["no_static", "no_merge", "h2s_rb3", "no_absorb"])
def test_switch_variants_pass_the_same_checks(env, sel, count):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_fused_families.py"), "-m", "gpu", "-q",
                        "-x", "-k", f"({sel}) and not switch_variants"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{count} passed" in r.stdout, r.stdout[-2000:]
