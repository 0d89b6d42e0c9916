"""The inverse step on the GPU, through the C ABI: qc_post_learn alone, qc_fused_pinn_inverse_step (QC_PHASE_GRADS) against
the float64 reference with a trainable global operator (tests/inverse_reference.py) in every circuit family and form, its
agreement with the data and the coefficient step, determinism, one optimiser step with a frozen entry and the coefficient
history, the refusals, and InverseTrainer against float64 replays: six steps entry by entry, a continued run, and the
identification of a transport coefficient.

The cases are those of tests/test_gpu_tabulated.py (same weights, points, targets) under inverse_reference.BASE / SCALE /
P0.  Tolerances are the project's: the gradient block by block at 2e-4 x max(1, max |ref block|), the operator block under
the same rule, the loss parts at 1e-4, POINT_TOL / ROW_TOL of the post-stage tests, 1e-4 on a loss or coefficient history.
Negative controls (+d_xx u_xx, scale ignored, base ignored) must fail the same tolerance; tests/test_inverse_cpu.py shows
that each differs from the truth by far more."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inverse_reference as IR
import inverse_training as IT
import mlp_reference as R
import tabulated_reference as T
import tabulated_training as TT
from conftest import pkg
from test_gpu_fullsize import Log
from test_gpu_tabulated import (MERGED, POINT_TOL, ROW_TOL, THETA_MIN, TOL_G, TOL_L, _blocks, _errors as _tab_errors,
                                _merged_probe, _model)

pytestmark = pytest.mark.gpu

NAN = float("nan")
N_OP = IR.N_OP


def _inverse_step(eng, B_res, n_ic, n_bc, p=IR.P0, base=IR.BASE, scale=IR.SCALE, hist_cap=0, lr=0.005):
    """An InverseStep over [the engine's weights | p] behind poisoned buffers.  The scalar operator of the descriptor and
    data->c_u are NaN (InverseStep sets them so): the inverse step must not read them."""
    engine = pkg("hip.engine")
    flat = torch.cat([eng.flat.detach(), torch.tensor(p, dtype=torch.float32, device=eng.device)])
    opt = engine.OptimState(flat.numel(), lr, eng.device, hist_cap=hist_cap)
    fs = engine.InverseStep(eng.circuit, eng.H, flat, base, scale, B_res, n_ic, n_bc, opt)
    fs.refresh_gates()
    assert np.isnan(fs.desc.pde.c_t) and np.isnan(fs.desc.pde.d_yy) and np.isnan(fs.data.c_u)
    if fs.step_ws.numel() >= 4:
        nfl = fs.step_ws.numel() // 4
        fs.step_ws[: 4 * nfl].view(torch.float32).fill_(NAN)
    for buf in (fs.target_res, fs.target_val, fs.ws_res, fs.ws_val, fs.part, fs.flat_grad):
        buf.fill_(NAN)
    return fs


def _load(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res):
    dev = fs.device
    n_ic, n_bc, B_res = len(X_ic), len(X_bc), len(X_res)
    to = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(dev)
    if B_res:
        fs.X_res[:B_res], fs.target_res[:B_res] = to(X_res), to(r_res)
    if n_ic:
        fs.X_val[:n_ic], fs.target_val[:n_ic] = to(X_ic), to(u_ic)
    if n_bc:
        fs.X_val[n_ic:n_ic + n_bc], fs.target_val[n_ic:n_ic + n_bc] = to(X_bc), to(u_bc)


def inverse_grads(eng, X_ic, X_bc, X_res, u_ic, u_bc, r_res, **kw):
    """flat [grad (NP + 7) | L_r, L_bc, L_ic] of qc_fused_pinn_inverse_step's gradient phase on the given batches."""
    L = pkg("hip.lib")
    fs = _inverse_step(eng, len(X_res), len(X_ic), len(X_bc), **kw)
    _load(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res)
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    return fs.flat_grad.cpu().numpy().astype(np.float64)


def _errors(got, want_g, want_p, n, n_theta):
    """test_gpu_tabulated._errors on the network blocks and the parts, plus the operator block under the same rule."""
    NP = got.size - 3 - N_OP
    out = _tab_errors(np.concatenate([got[:NP], got[NP + N_OP:]]), want_g[:NP], want_p, n, n_theta)
    op, want = got[NP:NP + N_OP], want_g[NP:NP + N_OP]
    out["operator"] = np.abs(op - want).max() / (TOL_G * max(1.0, np.abs(want).max()))
    return out


# ---- 1. qc_post_learn alone
ROW0, STRIDE_PAD, N_THETA = 2, 7, 3


@pytest.mark.parametrize("Hn", [(50, 4), (129, 3)], ids=["H50_n4_fused", "H129_n3_split"])
def test_post_learn_alone(Hn, gpu_device):
    """B = 65 (two tiles, the second with one point) behind NaN-filled outputs; H = 129 takes the point kernel + weight-gradient
    kernel pair.  pde.c_t .. d_yy are NaN: not read.  A history buffer is handed over and must stay untouched."""
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    (Hh, n), B = Hn, 65
    g = np.random.default_rng(Hh + 7)
    lay, NP = R.layout(Hh, n, N_THETA)
    NP_L = NP + N_OP
    flat = np.full(NP_L, np.nan, np.float32)
    for k in ("W3", "b3", "W4", "b4"):
        o, s = lay[k]
        flat[o:o + int(np.prod(s))] = g.uniform(-1, 1, int(np.prod(s))) / np.sqrt({"W3": n, "b3": n}.get(k, Hh))
    flat[NP:] = IR.P0
    q = np.concatenate([g.uniform(-1, 1, (1, n, B)), g.standard_normal((5, n, B))]).astype(np.float32)
    target = g.standard_normal(B).astype(np.float32)
    pde = dict(D=0.01, vx=1.0, vy=1.0, c_t=NAN, c_x=NAN, c_y=NAN, d_xx=NAN, d_yy=NAN, w_res=4.0 / B, inv_n_res=1.0 / B,
               w_val_a=0.3, w_val_b=0.7, inv_n_a=0.11, inv_n_b=0.13, problem=L.QC_PROBLEM_TABULATED, n_seg_a=B // 3)
    nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device=dev)
    cot, qbar, part, hist = nan(6 * B + 64), nan(6 * n * B + 64), nan(ROW0 + 2 + 2, NP_L + 3 + STRIDE_PAD), nan(4, N_OP)
    prm, qd, tg = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (flat, q, target))
    lr = L.QcStepLearn()
    for k in range(N_OP):
        lr.base[k], lr.scale[k] = IR.BASE[k], IR.SCALE[k]
    lr.coef_hist_dev, lr.coef_hist_cap = hist.data_ptr(), 4
    qpde = L.QcPde(**pde)
    L.check(lib.qc_post_learn(prm.data_ptr(), Hh, n, N_THETA, C.byref(qpde), C.byref(lr), qd.data_ptr(), tg.data_ptr(),
                              cot.data_ptr(), qbar.data_ptr(), part.data_ptr(), part.shape[1], ROW0, B,
                              torch.cuda.current_stream(dev).cuda_stream), "qc_post_learn")
    torch.cuda.synchronize(dev)
    assert torch.isnan(hist).all()
    for buf, m in ((cot, 6 * B), (qbar, 6 * n * B)):
        a = buf.cpu().numpy()
        assert np.isnan(a[m:]).all() and np.isfinite(a[:m]).all()
    cot, qbar = cot.cpu().numpy()[:6 * B].reshape(6, B), qbar.cpu().numpy()[:6 * n * B].reshape(6, n, B)
    p = part.cpu().numpy()
    names = ("W3", "b3", "W4", "b4")
    wcols = np.concatenate([np.arange(lay[k][0], lay[k][0] + int(np.prod(lay[k][1]))) for k in names])
    ocols, lcols = np.arange(NP, NP_L), np.arange(NP_L, NP_L + 3)
    mask = np.zeros(p.shape, bool)
    mask[ROW0:ROW0 + 2, np.concatenate([wcols, ocols, lcols])] = True
    assert np.isnan(p[~mask]).all() and np.isfinite(p[mask]).all()
    assert (p[ROW0:ROW0 + 2, NP + 3] == 0.0).all()          # the frozen entry: exactly 0

    def errors(variant=""):
        flat64 = np.nan_to_num(flat[:NP].astype(np.float64))
        P = R.unpack(flat64, Hh, n, N_THETA)
        qt = torch.from_numpy(q).double().requires_grad_(True)
        pt = torch.tensor(np.asarray(IR.P0, np.float32).astype(np.float64), requires_grad=True)
        u = R.post_jets(P, qt)
        e = IR.residual_op(u, IR.operator(pt, variant=variant), variant) - torch.from_numpy(target).double()
        obj = 0.5 * pde["w_res"] * e * e
        qb = torch.autograd.grad(obj.sum(), qt, retain_graph=True)[0].numpy()
        ub = torch.autograd.grad(obj.sum(), u, retain_graph=True)[0].numpy()          # (6, B): d obj / d u channels
        rows = np.stack([R.flatten(dict(zip(names, gr)), Hh, n, N_THETA) for gr in R.tile_grads(obj, [P[k] for k in names], B)])
        orow = np.stack([torch.autograd.grad(obj[k:k + 64].sum(), pt, retain_graph=True)[0].numpy() for k in range(0, B, 64)])
        losses = np.stack([R.loss_parts(e[k:k + 64], pde, 6).detach().numpy() for k in range(0, B, 64)])
        rel = lambda got, want, tol: np.abs(got - want).max() / (tol * max(1.0, np.abs(want).max()))
        per_entry = np.abs(p[ROW0:ROW0 + 2][:, ocols] - orow).max(0)
        return {"cot": rel(cot, ub, POINT_TOL), "qbar": rel(qbar, qb, POINT_TOL),
                "rows": rel(p[ROW0:ROW0 + 2][:, wcols], rows[:, wcols], ROW_TOL),
                "operator": rel(p[ROW0:ROW0 + 2][:, ocols], orow, ROW_TOL),
                "loss": rel(p[ROW0:ROW0 + 2][:, lcols], losses, ROW_TOL)}, per_entry
    err, per_entry = errors()
    print({k: float(v) for k, v in err.items()}, "operator columns, |error| per entry:", per_entry)
    assert max(err.values()) < 1.0, err
    for v in ("sign_dxx", "noscale", "nobase"):
        bad, _ = errors(v)
        print(v, {k: round(float(x), 1) for k, x in bad.items()})
        assert bad["operator"] > 1.0, (v, bad)


# ---- 2. the step against float64 in every family and form
@pytest.mark.parametrize("case", list(IR.CASES))
def test_inverse_step_matches_fp64(case, gpu_device):
    ans, n, Lq, enc, B_res, n_ic, n_bc = IR.CASES[case]
    flat, *batch = IR.case_inputs(case)
    ref = IR.case_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat, IR.case_H(case))
    n_theta = eng.n_theta
    got = inverse_grads(eng, *batch)
    NP = eng.NP
    assert got.size == NP + N_OP + 3 and np.isfinite(got).all() and eng.H == IR.case_H(case)
    err = _errors(got, ref["grad"], ref["parts"], n, n_theta)
    print(case, {k: round(float(v), 4) for k, v in err.items()})
    print(case, "operator block, |error| per entry:", np.abs(got[NP:NP + N_OP] - ref["grad"][NP:]), "reference:", ref["grad"][NP:])
    assert max(err.values()) < 1.0, err
    assert got[NP + 3] == 0.0                                   # scale_k = 0: exactly 0
    if B_res == 0:
        assert (got[NP:NP + N_OP] == 0.0).all()                 # value tiles only: zeros, not what the scratch held
    else:
        assert np.abs(np.delete(ref["grad"][NP:], 3)).min() > 1e-3
    assert np.abs(ref["grad"][_blocks(n, n_theta, eng.H)["theta"]]).max() > THETA_MIN
    if 2 <= n <= 5:
        merged = case in MERGED and os.environ.get("QC_NO_MERGE") != "1"
        assert (_merged_probe(eng, B_res, n_ic, n_bc) == 0) == merged
    for v in IR.CONTROLS.get(case, ()):
        bad = IR.case_reference(case, v)
        berr = _errors(got, bad["grad"], bad["parts"], n, n_theta)
        print(case, v, {k: round(float(x), 2) for k, x in berr.items()})
        assert berr["operator"] > 1.0 and max(berr.values()) > 1.0, (v, berr)


# ---- 3. switch variants
@pytest.mark.parametrize("env", [{"QC_NO_STATIC": "1"}, {"QC_NO_MERGE": "1"}], ids=["no_static", "no_merge"])
def test_switch_variants_pass_the_same_check(env):
    """The two cascade n = 4 cases (H = 50 and H = 129) through the circuit interpreter, and through the two-stream form
    (the switches are read once at load: a child process)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_inverse.py"), "-m", "gpu", "-q", "-x",
                        "-k", "inverse_step_matches_fp64 and reg_cascade4"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-2000:]


# ---- 4. agreement with the existing steps
def test_frozen_operator_passes_the_records_of_the_data_and_the_coefficient_step(gpu_device):
    """scale = 0 and base = the data step's operator: the first NP entries and the parts pass the data step's own committed
    record, the operator block is exactly 0.  With c_3 = 0.4 as well they pass the coefficient step's float64 reference
    on the uniform table."""
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = IR.CASES[case]
    flat, *batch = IR.case_inputs(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    NP = eng.NP
    for c3, ref in ((0.0, T.case_reference(case)), (IR.UNIFORM_C3, IR.uniform_c3_reference(case))):
        got = inverse_grads(eng, *batch, base=(T.C_U,) + T.COEFFS + (c3,), scale=(0.0,) * N_OP)
        assert (got[NP:NP + N_OP] == 0.0).all()
        err = _tab_errors(np.concatenate([got[:NP], got[NP + N_OP:]]), ref["grad"], ref["parts"], n, eng.n_theta)
        print("c_3 =", c3, {k: round(float(v), 4) for k, v in err.items()})
        assert max(err.values()) < 1.0, err


# ---- 5. determinism
@pytest.mark.parametrize("case", ["reg_cascade4", "reg_cascade4_H129", "wave_layered7"])
def test_two_runs_give_the_same_bits(case, gpu_device):
    ans, n, Lq, enc, *_ = IR.CASES[case]
    flat, *batch = IR.case_inputs(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat, IR.case_H(case))
    a, b = inverse_grads(eng, *batch), inverse_grads(eng, *batch)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 6. one optimiser step
def test_one_update_moves_the_live_entries_and_writes_the_history(gpu_device):
    L = pkg("hip.lib")
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = IR.CASES[case]
    flat, *batch = IR.case_inputs(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    fs = _inverse_step(eng, B_res, n_ic, n_bc, hist_cap=3)
    _load(fs, *batch)
    fs.coef_hist.fill_(NAN)
    NP = eng.NP
    before = [t[NP:].clone() for t in (fs.flat, fs.opt.m, fs.opt.v)]
    w_before = fs.flat[:NP].clone()
    fs.run(L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE)
    torch.cuda.synchronize()
    after = [t[NP:] for t in (fs.flat, fs.opt.m, fs.opt.v)]
    for b, a in zip(before, after):
        assert b[3].cpu().numpy().view(np.uint32) == a[3].cpu().numpy().view(np.uint32)        # frozen: bit-unchanged
    live = [k for k in range(N_OP) if k != 3]
    assert (before[0][live] != after[0][live]).all() and (after[1][live] != 0).all() and (after[2][live] > 0).all()
    assert float((after[0][live] - before[0][live]).abs().max()) <= 0.005 * 1.001          # Adam's first step: lr at most
    assert not torch.equal(w_before, fs.flat[:NP]) and fs.opt.read()["step"] == 1
    hist = fs.coef_hist.cpu().numpy()
    want = IR.coefficients_f32()
    assert np.array_equal(hist[0].view(np.uint32), want.view(np.uint32)), (hist[0], want)
    assert np.isnan(hist[1:]).all()
    assert fs.opt.loss_history(1)[0] == pytest.approx(float(np.dot((2, 4, 2), IR.case_reference(case)["parts"])), rel=1e-4)


# ---- 7. refusals
def test_refusals_name_one_fault_each(gpu_device):
    """A descriptor that runs (rc 0), then the same descriptor with ONE fault: -1, and nothing written."""
    L = pkg("hip.lib")
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = IR.CASES[case]
    flat, *batch = IR.case_inputs(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    fs = _inverse_step(eng, B_res, n_ic, n_bc, hist_cap=2)
    _load(fs, *batch)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    ref = lambda s: None if s is None else C.byref(s)
    call = lambda desc, data, lr, phases=L.QC_PHASE_GRADS: eng.lib.qc_fused_pinn_inverse_step(ref(desc), ref(data), ref(lr), phases, st)
    assert call(fs.desc, fs.data, fs.learn) == 0
    torch.cuda.synchronize()
    fs.flat_grad.fill_(NAN)
    fs.part.fill_(NAN)
    fs.coef_hist.fill_(NAN)

    def broken(src, **kw):
        t = type(src).from_buffer_copy(src)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(t, k)[v[0]] = v[1]
            else:
                setattr(t, k, v)
        return t
    assert call(fs.desc, fs.data, None) == -1 and call(fs.desc, None, fs.learn) == -1
    for kw in (dict(base=(0, NAN)), dict(base=(6, float("inf"))), dict(scale=(3, NAN)), dict(scale=(1, -float("inf"))),
               dict(coef_hist_cap=-1), dict(coef_hist_dev=None)):
        assert call(fs.desc, fs.data, broken(fs.learn, **kw)) == -1, kw
    assert call(broken(fs.desc, part_stride=fs.stride - 1), fs.data, fs.learn) == -1          # NP_L + 2
    assert call(broken(fs.desc, part_stride=eng.NP + 3), fs.data, fs.learn) == -1             # the data step's stride
    # whatever the data step refuses
    assert call(fs.desc, broken(fs.data, target_res_dev=None), fs.learn) == -1
    assert call(fs.desc, broken(fs.data, target_val_dev=None), fs.learn) == -1
    assert call(fs.desc, fs.data, fs.learn, L.QC_PHASE_GRADS | L.QC_PHASE_SAMPLE) == -1       # no dataset
    for pb in (0, 1, 2, 4):
        fs.desc.pde.problem = pb
        assert call(fs.desc, fs.data, fs.learn) == -1
    fs.desc.pde.problem = L.QC_PROBLEM_TABULATED
    torch.cuda.synchronize()
    assert torch.isnan(fs.flat_grad).all() and torch.isnan(fs.part).all() and torch.isnan(fs.coef_hist).all()
    assert call(fs.desc, fs.data, fs.learn) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(fs.flat_grad).all()


# ---- 8. training replay
def _operator():
    LO = pkg("data.tabulated").LearnedOperator
    live = {k: b for k, b, s in zip(IR.COLS, IR.BASE, IR.SCALE) if s != 0}
    op = LO(fixed={k: b for k, b, s in zip(IR.COLS, IR.BASE, IR.SCALE) if s == 0}, learn=live,
            scale={k: s for k, s in zip(IR.COLS, IR.SCALE) if s != 0})
    with torch.no_grad():
        op.p.copy_(torch.tensor(IR.P0))
    return op


def _trainer(gpu_device, tmp_path, ans, n, capacity=IT.STEPS):
    TP = pkg("data.tabulated").TabulatedProblem
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    InverseTrainer = pkg("trainer.inverse_train").InverseTrainer

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(TT.base_args(ans, n), TmpLog(), device=gpu_device)
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in IT.dataset_arrays())
    op = _operator()
    torch.manual_seed(TT.TRAINER_SEED_AT)
    tr = InverseTrainer(model, IT.BATCH, TP(Xr, rr, Xi, ui, Xb, ub), op, capacity=capacity)
    assert tr.fs.desc.sample_seed == TT.trainer_seed()
    return model, op, tr


@pytest.mark.parametrize("case", list(IT.TRAIN_CASES))
def test_training_matches_the_fp64_replay_loss_and_coefficients(case, gpu_device, tmp_path):
    """Six steps of InverseTrainer on tabulated_training's dataset, seed and sizes: the batches bit for bit, the loss
    history and the coefficient history against the float64 replay.  The replay moves c by (-0.008, 0.012, 0.005, 0, 0.0006,
    0.089, -0.028) over the six steps; the control (the operator held at its start) must fail the coefficient check."""
    ans, n = IT.TRAIN_CASES[case]
    model, op, tr = _trainer(gpu_device, tmp_path, ans, n)
    batches = []
    for _ in range(IT.STEPS):
        tr.sample()
        tr.step()
        fs = tr.fs
        Xv, tv = fs.X_val.cpu().numpy(), fs.target_val.cpu().numpy()
        batches.append((Xv[:IT.N_IC], Xv[IT.N_IC:IT.N_IC + IT.N_BC], fs.X_res.cpu().numpy()[:IT.BATCH], tv[:IT.N_IC],
                        tv[IT.N_IC:IT.N_IC + IT.N_BC], fs.target_res.cpu().numpy()[:IT.BATCH]))
    for got, want in zip(batches, IT.expected_batches()):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    ref, held = IT.training_reference(case, batches), IT.training_reference(case, batches, hold=True)
    got_l, got_c = np.array(tr.loss_history()), tr.coefficient_history().numpy().astype(np.float64)
    assert got_l.shape == (IT.STEPS,) and got_c.shape == (IT.STEPS, N_OP)
    err_l = np.abs(got_l - ref["loss"]).max() / (1e-4 * max(1.0, np.abs(ref["loss"]).max()))
    rel_c = lambda want: (np.abs(got_c - want) / (1e-4 * np.maximum(1.0, np.abs(want)))).max()
    print(case, "loss", got_l, ref["loss"], "error / tolerance", err_l)
    print(case, "coefficients moved by", got_c[-1] - got_c[0], "reference", ref["coef"][-1] - ref["coef"][0])
    print(case, "largest coefficient error / tolerance", rel_c(ref["coef"]), "against the held operator", rel_c(held["coef"]))
    assert err_l < 1.0 and rel_c(ref["coef"]) < 1.0
    assert rel_c(held["coef"]) > 1.0
    assert np.array_equal(got_c[0].astype(np.float32), IR.coefficients_f32())
    # the trained values are where the objects look for them
    now = np.array([tr.coefficients()[k] for k in IR.COLS])
    assert np.abs(now - ref["coef"][-1]).max() < 0.02 and now[3] == np.float32(IR.BASE[3])
    assert op.p.data_ptr() == tr.flat.data_ptr() + 4 * tr.NP and model._packed_ok()


# ---- 9. continuation
def test_a_saved_and_reloaded_run_continues_bit_for_bit(gpu_device, tmp_path):
    ans, n = IT.TRAIN_CASES["cascade4"]
    InverseTrainer = pkg("trainer.inverse_train").InverseTrainer
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    _, _, straight = _trainer(gpu_device, tmp_path, ans, n)
    for _ in range(IT.STEPS):
        straight.sample()
        straight.step()
    want_l, want_c = straight.loss_history(), straight.coefficient_history()

    model, op, first = _trainer(gpu_device, tmp_path, ans, n)
    for _ in range(3):
        first.sample()
        first.step()
    path = os.path.join(str(tmp_path), "half.pth")
    model.save_state(path)
    op_state = {k: v.cpu().clone() for k, v in op.state_dict().items()}
    seed, sample_step = first.fs.desc.sample_seed, first.fs.desc.sample_step
    got_l, got_c = first.loss_history(), first.coefficient_history()

    state = Solver.load_state(path)
    model2, op2, _ = None, None, None
    torch.manual_seed(5)
    model2 = Solver(TT.base_args(ans, n), Log(), device=gpu_device)
    op2 = _operator()
    op2.load_state_dict(op_state)
    for name in ("preprocessor", "quantum_layer", "postprocessor"):
        getattr(model2, name).load_state_dict(state[name])
    InverseTrainer.attach(model2, op2)
    model2.optimizer.load_state_dict(state["optimizer"])
    model2.scheduler.load_state_dict(state["scheduler"])
    TP = pkg("data.tabulated").TabulatedProblem
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in IT.dataset_arrays())
    second = InverseTrainer(model2, IT.BATCH, TP(Xr, rr, Xi, ui, Xb, ub), op2, capacity=3)
    second.fs.set_sampler(seed)
    second.fs.desc.sample_step = sample_step
    for _ in range(3):
        second.sample()
        second.step()
    assert second.opt.read()["step"] == IT.STEPS
    got_l, got_c = got_l + second.loss_history(), torch.cat([got_c, second.coefficient_history()])
    assert np.array_equal(np.array(got_l, np.float32).view(np.uint32), np.array(want_l, np.float32).view(np.uint32))
    assert torch.equal(got_c, want_c)


# ---- 10. recovery of a transport coefficient
def test_a_transport_coefficient_is_identified(gpu_device, tmp_path):
    """u* = sin 2 pi x cos pi y exp(-t / 2) + 0.3 observed at interior points, r = u*_t + 0.8 u*_x - 0.05 (u*_xx + u*_yy); c_t,
    d_xx, d_yy fixed, c_x learnt from 0.2.  4 000 steps on the device sampler (the length at which the float64 replay on
    these batches has settled, tests/inverse_training.py): the mean of the last 500 coefficients is within 0.05 of 0.8
    (three times the band of the float64 replay, tests/test_inverse_cpu.py, for fp32 and a chaotic trajectory), and row 0
    is the start."""
    tab = pkg("data.tabulated")
    InverseTrainer = pkg("trainer.inverse_train").InverseTrainer
    Solver = pkg("nn.DVPDESolver").DVPDESolver

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(dict(IT.REC_ARGS), TmpLog(), device=gpu_device)
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in IT.recovery_dataset())
    op = tab.LearnedOperator(fixed=IT.REC_FIXED, learn={"c_x": IT.REC_START})
    tr = InverseTrainer(model, IT.REC_BATCH, tab.TabulatedProblem(Xr, rr, Xi, ui, Xb, ub), op, n_ic=IT.REC_N_IC,
                        n_bc=IT.REC_N_BC, capacity=IT.REC_STEPS)
    tr.fs.set_sampler(IT.REC_SEED)
    for _ in range(IT.REC_STEPS):
        tr.sample()
        tr.step()
    torch.cuda.synchronize()
    c = tr.coefficient_history().numpy()
    k = IR.COLS.index("c_x")
    ref = IT.recovery_reference()["c_x"]
    print("c_x every", IT.REC_EVERY, "steps:", c[::IT.REC_EVERY, k], "float64 replay:", ref)
    assert c.shape == (IT.REC_STEPS, N_OP) and c[0, k] == np.float32(IT.REC_START)
    others = [j for j in range(N_OP) if j != k]
    assert (c[:, others] == np.array([IT.REC_FIXED.get(n_, 0.0) for n_ in IR.COLS], np.float32)[others]).all()
    mean = float(c[-500:, k].astype(np.float64).mean())
    print("mean of the last 500:", mean, "now:", tr.coefficients()["c_x"])
    assert abs(mean - IT.REC_TRUE) < 0.05, mean
