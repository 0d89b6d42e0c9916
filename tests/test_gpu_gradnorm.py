"""The gradient-norm step on the GPU against the float64 class gradients of tests/gradnorm_reference.py: one GRADS call per
case at 128 + 64 + 70 points (two residual tiles, one IC tile, a full and a partial BC tile) in the register family
(merged and two-stream), the lanes family and the HBM family, with an empty IC and an empty BC class, on the tabulated,
the analytic and the coefficient-table problem, with QC_PHASE_SAMPLE, and the refusal of a value batch whose tiles would
mix the classes.

Tolerances are those of tests/test_gpu_causal.py: the gradient block by block at 2e-4 x max(1, max |ref block|), the loss
parts at 1e-4 (``_errors``), the record at 1e-4 relative.  The control with both weights held at 1 must miss."""
import ctypes as C

import numpy as np
import pytest
import torch

import gradnorm_reference as GR
import tabulated_reference as T
import tabulated_training as TT
from conftest import pkg
from test_gpu_tabulated import _errors, _load, _model

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _step(eng, kind, B_res, n_ic, n_bc, cfg=GR.STEP_CFG, capacity=2, hist_cap=0):
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    if kind == "analytic":
        eng.problem, eng.coeffs, eng.c_u, eng.coef_mode = L.QC_PROBLEM_CONVECTION_DIFFUSION, None, 0.0, False
    elif kind == "coef":
        eng.problem, eng.coeffs, eng.c_u, eng.coef_mode = L.QC_PROBLEM_TABULATED, (NAN,) * 5, NAN, True
    else:
        eng.problem, eng.coeffs, eng.c_u, eng.coef_mode = L.QC_PROBLEM_TABULATED, T.COEFFS, T.C_U, False
    eng.refresh_gates()
    opt = engine.OptimState(eng.NP, 0.005, eng.device, hist_cap=hist_cap)
    try:
        return engine.GradNormStep(eng, B_res, n_ic, n_bc, opt, cfg["alpha"], cfg["every"], cfg["lam_max"], cfg["init"],
                                   capacity=capacity, counts=(B_res, max(n_ic, 1), max(n_bc, 1)))
    finally:
        eng.coef_mode = False


def _fill(fs, kind, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef):
    dev = fs.eng.device
    to = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(dev)
    if kind == "analytic":
        n_ic, n_bc = len(X_ic), len(X_bc)
        fs.X_res[:len(X_res)] = to(X_res)
        if n_ic:
            fs.X_val[:n_ic] = to(X_ic)
        if n_bc:
            fs.X_val[n_ic:n_ic + n_bc] = to(X_bc)
        return
    _load(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res)
    if kind == "coef":
        fs.coef_res[:, :len(X_res)] = to(coef).t()


def _check(case, fs, eng, n, n_ic, n_bc, rec):
    got = fs.flat_grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    want, st_want, h_want = GR.expected_step(rec, n_ic, n_bc)
    unit, _, _ = GR.expected_step(rec, n_ic, n_bc, unit=True)
    NP = got.size - 3
    err = _errors(got, want[:NP], want[NP:], n, eng.n_theta)
    berr = _errors(got, unit[:NP], unit[NP:], n, eng.n_theta)
    st = fs.read_state()
    keys = [k for k in ("lam_bc", "lam_ic", "m_r", "a_bc", "a_ic", "hat_bc", "hat_ic") if st_want[k] != 0.0]
    rec_err = max(abs(st[k] - st_want[k]) / (1e-4 * abs(st_want[k])) for k in keys)
    factor = max(berr.values())
    print(case, "error / tolerance", {k: round(float(v), 4) for k, v in err.items()}, "record", round(rec_err, 4),
          "| unit weights miss by", round(float(factor), 1), "tolerances | m_r / a_ic", st["m_r"] / max(st["a_ic"], 1e-30),
          "lam", st["lam_bc"], st["lam_ic"])
    assert max(err.values()) < 1.0, err
    assert rec_err < 1.0, (st, st_want)
    assert all(st[k] == 0.0 for k in st_want if k not in keys and k.startswith(("a_", "hat_")))
    assert factor > 1.0
    assert (st["n_steps"], st["n_updates"], st["hist_base"]) == (1, 1, 0)
    h = fs.history()
    assert h.shape == (1, 7) and h[0, 6] == 1.0 and np.array_equal(h[0, :2], np.float32([st["lam_bc"], st["lam_ic"]]))
    assert h[0, 5] == pytest.approx(h_want[0, 5], rel=1e-4)
    return factor


CASES = [c for c in GR.STEP_CASES if c != "sampled"]


@pytest.mark.parametrize("case", CASES)
def test_one_grads_call_matches_the_fp64_class_gradients(case, gpu_device, monkeypatch):
    L = pkg("hip.lib")
    kind, ans, n, Lq, B_res, n_ic, n_bc = GR.STEP_CASES[case]
    if case == "reg_cascade2":
        monkeypatch.setenv("QC_NO_MERGE", "1")          # the two-stream form of the register family
    flat, *batch = GR.step_case_inputs(case)
    rec = GR.step_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, "None", flat)
    fs = _step(eng, kind, B_res, n_ic, n_bc)
    _fill(fs, kind, *batch)
    params = eng.flat.detach().clone()
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize(gpu_device)
    factor = _check(case, fs, eng, n, n_ic, n_bc, rec)
    if n_ic and n_bc:
        assert factor > 50.0                          # the held control misses with room to spare
    assert torch.equal(eng.flat.detach(), params)     # GRADS alone moves no parameter


def test_update_phase_alone_is_the_plain_optimiser_call_on_the_combined_gradient(gpu_device):
    """GRADS then UPDATE in two calls equals GRADS | UPDATE in one, bit for bit, and the optimiser record sees the
    unweighted w_res L_r + w_bc L_bc + w_ic L_ic."""
    L = pkg("hip.lib")
    case = "reg_cascade4"
    kind, ans, n, Lq, B_res, n_ic, n_bc = GR.STEP_CASES[case]
    flat, *batch = GR.step_case_inputs(case)
    out = []
    for split in (False, True):
        model, eng = _model(gpu_device, ans, n, Lq, "None", flat)
        fs = _step(eng, kind, B_res, n_ic, n_bc, hist_cap=2)
        _fill(fs, kind, *batch)
        for _ in range(2):
            if split:
                fs.run(L.QC_PHASE_GRADS)
                fs.run(L.QC_PHASE_UPDATE)
            else:
                fs.run(L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE)
        torch.cuda.synchronize(gpu_device)
        out.append((eng.flat.detach().cpu().numpy().copy(), fs.flat_grad.cpu().numpy().copy(), fs.state.cpu().numpy().copy(),
                    np.array(fs.opt.loss_history(2), np.float32), fs.opt.read()))
    (p0, g0, s0, h0, r0), (p1, g1, s1, h1, _) = out
    for a, b in ((p0, p1), (g0, g1), (s0, s1), (h0, h1)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.abs(p0 - np.asarray(flat, np.float32)).max() > 0
    assert r0["loss"] == pytest.approx(2.0 * r0["loss_res"] + 4.0 * r0["loss_bc"] + 2.0 * r0["loss_ic"], rel=1e-6)
    assert r0["grad_norm"] > 1.0 and np.linalg.norm(g0[:-3]) == pytest.approx(1.0, rel=1e-4)      # the clip acts on the combination


def test_sample_phase_draws_the_data_steps_batches_and_matches_fp64(gpu_device):
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    case = "sampled"
    kind, ans, n, Lq, B_res, n_ic, n_bc = GR.STEP_CASES[case]
    flat, *want_batch = GR.step_case_inputs(case)
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a).to(gpu_device) for a in TT.dataset_arrays())
    got = []
    for gradnorm in (True, False):
        model, eng = _model(gpu_device, ans, n, Lq, "None", flat)
        if gradnorm:
            fs = _step(eng, "tab", B_res, n_ic, n_bc)
        else:
            eng.problem, eng.coeffs, eng.c_u, eng.coef_mode = L.QC_PROBLEM_TABULATED, T.COEFFS, T.C_U, False
            fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, eng.device), (B_res, n_ic, n_bc))
        fs.set_dataset(((Xr, rr), (Xi, ui), (Xb, ub)))
        fs.set_sampler(GR.SAMPLE_SEED)
        fs.run(L.QC_PHASE_SAMPLE | L.QC_PHASE_GRADS)
        torch.cuda.synchronize(gpu_device)
        Xv, tv = fs.X_val.cpu().numpy(), fs.target_val.cpu().numpy()
        got.append((Xv[:n_ic], Xv[n_ic:n_ic + n_bc], fs.X_res.cpu().numpy()[:B_res], tv[:n_ic], tv[n_ic:n_ic + n_bc],
                    fs.target_res.cpu().numpy()[:B_res]))
        if gradnorm:
            keep = fs, eng
    for a, b, w in zip(got[0], got[1], want_batch):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))                      # the data step's batches, bit for bit
        assert np.array_equal(a, np.asarray(w, np.float32))                              # and the restated gather's
    fs, eng = keep
    _check(case, fs, eng, n, n_ic, n_bc, GR.step_reference(case, (flat, *got[0], None)))


def test_mixed_value_tiles_are_refused_and_nothing_is_touched(gpu_device):
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res, _ = GR.step_case_inputs("reg_cascade4")
    model, eng = _model(gpu_device, "cascade", 4, 1, "None", flat)
    with pytest.raises(L.QcError, match="multiple of 64"):
        _step(eng, "tab", 128, 21, 21)
    eng.problem, eng.coeffs, eng.c_u, eng.coef_mode = L.QC_PROBLEM_TABULATED, T.COEFFS, T.C_U, False
    fs = engine.FusedStep(eng, 128, 21, 21, engine.OptimState(eng.NP, 0.005, eng.device), (128, 21, 21))
    _load(fs, X_ic[:21], X_bc[:21], X_res, u_ic[:21], u_bc[:21], r_res)
    state = torch.full((L.QC_GRADNORM_STATE_WORDS,), 7.0, dtype=torch.float32, device=gpu_device)
    gn = L.QcStepGradnorm(0.5, 1e4, 1, 1.0, 1.0, state.data_ptr(), None, 0)
    fs.part.fill_(3.0)
    fs.flat_grad.fill_(5.0)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    for phases in (L.QC_PHASE_GRADS, L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE, L.QC_PHASE_UPDATE, L.QC_PHASE_SAMPLE):
        assert eng.lib.qc_fused_pinn_gradnorm_step(C.byref(fs.desc), C.byref(fs.data), None, C.byref(gn), phases, st) == -1
    torch.cuda.synchronize(gpu_device)
    assert (fs.part == 3.0).all() and (fs.flat_grad == 5.0).all() and (state == 7.0).all()
