"""The balanced step on the GPU, through the C ABI: qc_post_balance alone, qc_fused_pinn_balanced_step (QC_PHASE_GRADS)
against the float64 reference (tests/balanced_reference.py: the per-class gradients of the tabulated cases combined under
SCALE and P0) in every circuit family and form, its agreement with the data step at scale 0, qc_balance_adam_step alone
on synthetic vectors (both kernels, the frozen term, the fixed point of s_k), one update through the step (the folding
kernel), determinism and the refusals.  The trainer is tested in tests/test_gpu_balanced_train.py.

Tolerances are the project's: the network gradient block by block at 2e-4 x max(1, max |ref block|), the loss parts at
1e-4, POINT_TOL / ROW_TOL of the post-stage tests.  The balancer's gradient entry scale_k (1 - w_k e_k L_k) inherits the
parts' tolerance through its factor scale_k w_k e_k.  Negative controls (exp(+s), scale ignored, BC and IC factors swapped)
must fail the same tolerance; tests/test_balanced_cpu.py shows that each differs from the truth by more."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import balanced_reference as BR
import mlp_reference as R
import tabulated_reference as T
from conftest import pkg
from test_gpu_tabulated import (MERGED, POINT_TOL, ROW_TOL, THETA_MIN, TOL_G, TOL_L, _blocks, _errors as _tab_errors,
                                _merged_probe, _model)

pytestmark = pytest.mark.gpu

NAN = float("nan")
N_BAL = BR.N_BAL


def device_weights(dev, p=BR.P0, scale=BR.SCALE, w=BR.W):
    """w_k * expf(-(scale_k * p_k)) in float32 with the DEVICE's expf (torch.exp on the device), every step rounded to
    float32 as the kernels round it: the bits the weight history must hold."""
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)
    return (f(w) * torch.exp(-(f(scale) * f(p)))).cpu().numpy()


def _balanced_step(eng, B_res, n_ic, n_bc, p=BR.P0, scale=BR.SCALE, hist_cap=0, lr=0.005):
    """A BalancedStep over [the engine's weights | p] behind poisoned buffers, with the tabulated cases' operator."""
    engine = pkg("hip.engine")
    flat = torch.cat([eng.flat.detach(), torch.tensor(p, dtype=torch.float32, device=eng.device)])
    opt = engine.OptimState(flat.numel(), lr, eng.device, hist_cap=hist_cap)
    fs = engine.BalancedStep(eng.circuit, eng.H, flat, scale, B_res, n_ic, n_bc, opt, T.COEFFS, T.C_U)
    fs.refresh_gates()
    if fs.step_ws.numel() >= 4:
        nfl = fs.step_ws.numel() // 4
        fs.step_ws[: 4 * nfl].view(torch.float32).fill_(NAN)
    for buf in (fs.target_res, fs.target_val, fs.ws_res, fs.ws_val, fs.part, fs.flat_grad, fs.weight_hist):
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


def balanced_grads(eng, X_ic, X_bc, X_res, u_ic, u_bc, r_res, **kw):
    """flat [grad (NP + 3) | L_r, L_bc, L_ic] of qc_fused_pinn_balanced_step's gradient phase on the given batches."""
    L = pkg("hip.lib")
    fs = _balanced_step(eng, len(X_res), len(X_ic), len(X_bc), **kw)
    _load(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res)
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    assert torch.isnan(fs.weight_hist).all()           # the history is the optimiser launch's
    return fs.flat_grad.cpu().numpy().astype(np.float64)


def _errors(got, want_g, want_p, n, n_theta):
    """test_gpu_tabulated._errors on the network blocks and the parts (the balancer's three entries taken out)."""
    NP = got.size - 3 - N_BAL
    return _tab_errors(np.concatenate([got[:NP], got[NP + N_BAL:]]), want_g[:NP], want_p, n, n_theta)


# ---- 1. qc_post_balance alone
ROW0, STRIDE_PAD, N_THETA = 2, 7, 3


@pytest.mark.parametrize("Hn", [(50, 4), (129, 3)], ids=["H50_n4_fused", "H129_n3_split"])
@pytest.mark.parametrize("nchB", [(6, 65), (1, 70)], ids=["res_B65", "val_B70"])
def test_post_balance_alone(Hn, nchB, gpu_device):
    """Two tiles behind NaN-filled outputs; the value batch has n_seg_a = 30, so its first tile holds IC and BC points; H = 129
    takes the point kernel + weight-gradient kernel pair.  A history buffer is handed over and must stay untouched."""
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    (Hh, n), (nch, B) = Hn, nchB
    g = np.random.default_rng(Hh + nch)
    lay, NP = R.layout(Hh, n, N_THETA)
    NP_B = NP + N_BAL
    flat = np.full(NP_B, np.nan, np.float32)
    for k in ("W3", "b3", "W4", "b4"):
        o, s = lay[k]
        flat[o:o + int(np.prod(s))] = g.uniform(-1, 1, int(np.prod(s))) / np.sqrt({"W3": n, "b3": n}.get(k, Hh))
    flat[NP:] = BR.P0
    q = np.concatenate([g.uniform(-1, 1, (1, n, B)), g.standard_normal((5, n, B))]).astype(np.float32)[:nch]
    target = g.standard_normal(B).astype(np.float32)
    c_u = 0.7
    pde = dict(D=0.01, vx=1.0, vy=1.0, c_t=1.3, c_x=0.7, c_y=-0.4, d_xx=0.02, d_yy=0.05, w_res=4.0 / B, inv_n_res=1.0 / B,
               w_val_a=0.3, w_val_b=0.7, inv_n_a=0.11, inv_n_b=0.13, problem=L.QC_PROBLEM_TABULATED, n_seg_a=30)
    qpde = L.QcPde(**pde)
    nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device=dev)
    out_u, out_res, qbar, hist = nan(B + 64), nan(B + 64), nan(nch * n * B + 64), nan(4, N_BAL)
    part = nan(ROW0 + 2 + 2, NP_B + 3 + STRIDE_PAD)
    prm, qd, tg = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (flat, q, target))
    bl = L.QcStepBalance()
    for k in range(N_BAL):
        bl.scale[k] = BR.SCALE[k]
    bl.weight_hist_dev, bl.weight_hist_cap = hist.data_ptr(), 4
    L.check(lib.qc_post_balance(prm.data_ptr(), Hh, n, N_THETA, C.byref(qpde), C.byref(bl), qd.data_ptr(), tg.data_ptr(), c_u,
                                out_u.data_ptr(), out_res.data_ptr() if nch == 6 else None, qbar.data_ptr(), part.data_ptr(),
                                part.shape[1], ROW0, B, nch, torch.cuda.current_stream(dev).cuda_stream), "qc_post_balance")
    torch.cuda.synchronize(dev)
    assert torch.isnan(hist).all()
    names = ("W3", "b3", "W4", "b4")
    wcols = np.concatenate([np.arange(lay[k][0], lay[k][0] + int(np.prod(lay[k][1]))) for k in names])
    ocols, lcols = np.arange(NP, NP_B), np.arange(NP_B, NP_B + 3)
    p = part.cpu().numpy()
    mask = np.zeros(p.shape, bool)
    mask[ROW0:ROW0 + 2, np.concatenate([wcols, ocols, lcols])] = True
    assert np.isnan(p[~mask]).all() and np.isfinite(p[mask]).all()
    assert (p[ROW0:ROW0 + 2][:, ocols] == 0.0).all()          # columns NP .. NP + 2: exactly 0 in rows pre-filled with NaN
    for buf, m in ((out_u, B), (out_res, B if nch == 6 else 0), (qbar, nch * n * B)):
        a = buf.cpu().numpy()
        assert np.isnan(a[m:]).all() and np.isfinite(a[:m]).all()

    def errors(variant=""):
        e_res, e_bc, e_ic = BR.factors(variant=variant)
        flat64 = np.nan_to_num(flat[:NP].astype(np.float64))
        P = R.unpack(flat64, Hh, n, N_THETA)
        qt = torch.from_numpy(q).double().requires_grad_(True)
        u = R.post_jets(P, qt)
        tt = torch.from_numpy(target).double()
        if nch == 6:
            e = c_u * u[0] + R.residual(u, (pde["c_t"], pde["c_x"], pde["c_y"], pde["d_xx"], pde["d_yy"])) - tt
        else:
            e = u[0] - tt
        scaled = dict(pde, w_res=pde["w_res"] * e_res, w_val_a=pde["w_val_a"] * e_ic, w_val_b=pde["w_val_b"] * e_bc)
        w = R.point_weights(B, scaled, nch)
        obj = 0.5 * w * e * e
        cot = (w * e).detach().numpy()
        qb = torch.autograd.grad(obj.sum(), qt, retain_graph=True)[0].numpy()
        rows = np.stack([R.flatten(dict(zip(names, gr)), Hh, n, N_THETA) for gr in R.tile_grads(obj, [P[k] for k in names], B)])
        losses = np.stack([R.loss_parts(e[k:k + 64], dict(pde, n_seg_a=pde["n_seg_a"] - k), nch).detach().numpy()
                           for k in range(0, B, 64)])
        rel = lambda got, want, tol: np.abs(got - want).max() / (tol * max(1.0, np.abs(want).max()))
        out = {"qbar": rel(qbar.cpu().numpy()[:nch * n * B].reshape(nch, n, B), qb, POINT_TOL),
               "rows": rel(p[ROW0:ROW0 + 2][:, wcols], rows[:, wcols], ROW_TOL),
               "loss": rel(p[ROW0:ROW0 + 2][:, lcols], losses, ROW_TOL)}
        if nch == 6:
            out["rbar"] = rel(out_res.cpu().numpy()[:B], cot, POINT_TOL)
            out["ubar"] = rel(out_u.cpu().numpy()[:B], c_u * cot, POINT_TOL)
        else:
            out["ubar"] = rel(out_u.cpu().numpy()[:B], cot, POINT_TOL)
        return out
    err = errors()
    print({k: float(v) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    for v in BR.VARIANTS if nch == 1 else ("exp_plus",):      # (residual points: the swap and the scale of 1 change nothing)
        bad = errors(v)
        print(v, {k: round(float(x), 1) for k, x in bad.items()})
        assert bad["ubar"] > 1.0 and bad["qbar"] > 1.0 and bad["loss"] < 1.0, (v, bad)      # the loss columns stay raw


# ---- 2. the step against float64 in every family and form
@pytest.mark.parametrize("case", list(BR.CASES))
def test_balanced_step_matches_fp64(case, gpu_device):
    ans, n, Lq, enc, B_res, n_ic, n_bc = BR.CASES[case]
    flat, *batch = BR.case_inputs(case)
    rec = BR.class_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat, BR.case_H(case))
    n_theta = eng.n_theta
    got = balanced_grads(eng, *batch)
    NP = eng.NP
    assert got.size == NP + N_BAL + 3 and np.isfinite(got).all() and eng.H == BR.case_H(case)
    ref = BR.combine(rec)
    err = _errors(got, ref, rec["parts"], n, n_theta)
    print(case, {k: round(float(v), 4) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    assert (got[NP:NP + N_BAL] == 0.0).all()                    # GRADS only: exactly 0, written by every tile row
    assert np.abs(ref[_blocks(n, n_theta, eng.H)["theta"]]).max() > THETA_MIN
    if 2 <= n <= 5:
        merged = case in MERGED and os.environ.get("QC_NO_MERGE") != "1"
        assert (_merged_probe(eng, B_res, n_ic, n_bc) == 0) == merged
    for v in BR.CONTROLS.get(case, ()):
        berr = _errors(got, BR.combine(rec, variant=v), rec["parts"], n, n_theta)
        print(case, v, {k: round(float(x), 2) for k, x in berr.items()})
        assert max(berr.values()) > 1.0 and berr["parts"] < 1.0, (v, berr)


# ---- 3. switch variants
@pytest.mark.parametrize("env", [{"QC_NO_STATIC": "1"}, {"QC_NO_MERGE": "1"}], ids=["no_static", "no_merge"])
def test_switch_variants_pass_the_same_check(env):
    """The two cascade n = 4 cases (H = 50 and H = 129) through the circuit interpreter, and through the two-stream form
    (the switches are read once at load: a child process)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_balanced.py"), "-m", "gpu", "-q", "-x",
                        "-k", "balanced_step_matches_fp64 and reg_cascade4"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-2000:]


# ---- 4. agreement with the data step
def test_scale_zero_passes_the_record_of_the_data_step(gpu_device):
    """scale = 0 (every e_k = 1 whatever p holds): the first NP entries and the parts pass the data step's own committed
    record, the three entries are 0."""
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = BR.CASES[case]
    flat, *batch = BR.case_inputs(case)
    ref = T.case_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    got = balanced_grads(eng, *batch, scale=(0.0, 0.0, 0.0))
    NP = eng.NP
    assert (got[NP:NP + N_BAL] == 0.0).all()
    err = _tab_errors(np.concatenate([got[:NP], got[NP + N_BAL:]]), ref["grad"], ref["parts"], n, eng.n_theta)
    print({k: round(float(v), 4) for k, v in err.items()})
    assert max(err.values()) < 1.0, err


# ---- 5. determinism
@pytest.mark.parametrize("case", ["reg_cascade4", "reg_cascade4_H129", "wave_layered7"])
def test_two_runs_give_the_same_bits(case, gpu_device):
    ans, n, Lq, enc, *_ = BR.CASES[case]
    flat, *batch = BR.case_inputs(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat, BR.case_H(case))
    a, b = balanced_grads(eng, *batch), balanced_grads(eng, *batch)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 6. the optimiser alone
LR = 0.005


def _adam_setup(dev, NP_B, scale, seed=0, hist_cap=3, p_tail=BR.P0, parts=(0.31, 0.052, 0.47), grad_scale=1.0):
    """Synthetic [grad[NP_B] | parts] with 1e6 in the balancer's slots, parameters with p in the tail, zero moments."""
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    g = np.random.default_rng(seed + NP_B)
    NP = NP_B - N_BAL
    flat = np.concatenate([grad_scale * g.standard_normal(NP), [1e6, -1e6, 1e6], parts]).astype(np.float32)
    prm = np.concatenate([g.standard_normal(NP), p_tail]).astype(np.float32)
    opt = engine.OptimState(NP_B, LR, dev, hist_cap=hist_cap)
    opt.hist.fill_(NAN)
    whist = torch.full((max(hist_cap, 1), N_BAL), NAN, dtype=torch.float32, device=dev)
    bl = L.QcStepBalance()
    for k in range(N_BAL):
        bl.scale[k] = scale[k]
    bl.weight_hist_dev, bl.weight_hist_cap = (whist.data_ptr(), hist_cap) if hist_cap else (None, 0)
    return flat, prm, opt, whist, bl


def _adam_call(lib, dev, flat_d, NP_B, prm_d, opt, bl, prog=None, theta_off=0, trig=None):
    return lib.qc_balance_adam_step(flat_d.data_ptr(), NP_B, prm_d.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(),
                                    opt.state.data_ptr(), C.byref(opt.hyper), C.byref(bl),
                                    opt.hist.data_ptr() if opt.hist_cap else None, opt.hist_cap, prog, theta_off, trig,
                                    torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize("NP_B", [4, 3069, 3070], ids=["NP_B4", "last_fast_3069", "first_general_3070"])
def test_balance_adam_step_alone(NP_B, gpu_device):
    """One call against a float64 Adam: the three gradient entries formed from the loss columns (whatever flat held in their
    slots: 1e6), the clip over the first NP entries only, F, the weight row to the bit, the record, the moved parameters."""
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    NP = NP_B - N_BAL
    flat, prm, opt, whist, bl = _adam_setup(dev, NP_B, BR.SCALE, grad_scale=3.0)      # |grad| > 1: the clip is active
    flat_d, prm_d = torch.from_numpy(flat).to(dev), torch.from_numpy(prm).to(dev)
    L.check(_adam_call(lib, dev, flat_d, NP_B, prm_d, opt, bl), "qc_balance_adam_step")
    torch.cuda.synchronize(dev)
    ref = BR.adam_reference(flat, prm, np.zeros(NP_B), np.zeros(NP_B), NP, lr=LR)
    got = flat_d.cpu().numpy().astype(np.float64)
    parts = flat[NP_B:].astype(np.float64)
    assert ref["norm"] > 1.0
    # the clipped network gradient: one float32 product per entry
    assert np.abs(got[:NP] - ref["grad"][:NP]).max() < 4e-7 * max(1.0, np.abs(ref["grad"][:NP]).max())
    # the three entries: scale_k (1 - w_k e_k L_k), the parts' tolerance through the factor scale_k w_k e_k
    bound = np.abs(np.asarray(BR.SCALE)) * ref["weights"] * TOL_L * max(1.0, np.abs(parts).max())
    print(NP_B, "own gradient", got[NP:NP_B], "reference", ref["grad"][NP:], "bound", bound)
    assert (np.abs(got[NP:NP_B] - ref["grad"][NP:]) <= bound).all()
    assert np.array_equal(got[NP_B:], parts)
    rec = opt.read()
    assert rec["step"] == 1 and rec["grad_norm"] == pytest.approx(ref["norm"], rel=1e-6)
    assert (np.float32(rec["loss_res"]), np.float32(rec["loss_bc"]), np.float32(rec["loss_ic"])) == tuple(flat[NP_B:])
    hist = opt.hist.cpu().numpy()
    # F: three fused multiply-adds and two sums in float32
    assert abs(hist[0] - ref["F"]) < 1e-6 * max(1.0, np.abs(ref["weights"] * parts).sum() + np.abs(BR.log_vars()).sum())
    assert rec["loss"] == hist[0] and np.isnan(hist[1:]).all()
    wh = whist.cpu().numpy()
    want_w = device_weights(dev)
    assert np.array_equal(wh[0].view(np.uint32), want_w.view(np.uint32)), (wh[0], want_w)
    assert np.abs(wh[0] - ref["weights"]).max() < 1e-6 * ref["weights"].max() and np.isnan(wh[1:]).all()
    # Adam's first step moves every entry by lr against the sign of its gradient
    p_new = prm_d.cpu().numpy().astype(np.float64)
    assert np.abs(p_new - ref["p"]).max() < 1e-6
    for a, b, tol in ((opt.m, ref["m"], 1e-6), (opt.v, ref["v"], 1e-6)):
        a = a.cpu().numpy().astype(np.float64)
        assert np.abs(a - b).max() < tol * max(1.0, np.abs(b).max())


def test_a_frozen_term_stays_bit_unchanged(gpu_device):
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    NP_B = 40
    NP = NP_B - N_BAL
    flat, prm, opt, whist, bl = _adam_setup(dev, NP_B, (1.0, 0.0, 0.5))
    flat_d, prm_d = torch.from_numpy(flat).to(dev), torch.from_numpy(prm).to(dev)
    for _ in range(2):
        L.check(_adam_call(lib, dev, flat_d, NP_B, prm_d, opt, bl), "qc_balance_adam_step")
        flat_d.copy_(torch.from_numpy(flat))
    torch.cuda.synchronize(dev)
    k = NP + 1
    assert prm_d[k].cpu().numpy().view(np.uint32) == prm[k:k + 1].view(np.uint32)[0]
    assert opt.m[k].cpu().numpy().view(np.uint32) == 0 and opt.v[k].cpu().numpy().view(np.uint32) == 0
    live = [NP, NP + 2]
    assert (prm_d[live].cpu().numpy() != prm[live]).all() and (opt.v[live] > 0).all()
    # the frozen term's weight is its base weight, whatever p holds
    assert whist[0, 1].item() == BR.W[1] and whist[1, 1].item() == BR.W[1]


def test_repeated_calls_drive_s_to_its_fixed_point(gpu_device):
    """Fixed L_k and a zero network gradient: s_k = scale_k p_k runs towards log(w_k L_k), where w_k e_k L_k = 1.  The number
    of calls and the distance reached come from the float64 Adam on the CPU; the device is held against that replay."""
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    NP_B, calls = 8, 300
    NP = NP_B - N_BAL
    scale = BR.SCALE
    parts = (0.55, 0.20, 0.62)                                   # log(w L) = (0.095, -0.223, 0.215)
    flat, prm, opt, whist, bl = _adam_setup(dev, NP_B, scale, hist_cap=0, p_tail=(0.0, 0.0, 0.0), parts=parts, grad_scale=0.0)
    s_fix = np.log(np.asarray(BR.W) * np.asarray(parts, dtype=np.float32).astype(np.float64))
    # float64 replay
    p, m, v = prm.astype(np.float64), np.zeros(NP_B), np.zeros(NP_B)
    for step in range(1, calls + 1):
        r = BR.adam_reference(flat, p, m, v, NP, scale=scale, lr=LR, step=step)
        p, m, v = r["p"], r["m"], r["v"]
    s_ref = np.asarray(scale) * p[NP:]
    d_ref = np.abs(s_ref - s_fix)
    print("float64 replay after", calls, "calls: s", s_ref, "fixed point", s_fix, "distance", d_ref)
    # the replay passes (0.098, -0.236, 0.113) at call 50 and (0.0953, -0.2231, 0.2139) at call 200, and is within 2.4e-6
    # of the fixed point at call 300 (IC, the slowest: scale 0.5); a float32 emulation of the same Adam differs from it by 5e-8
    assert d_ref.max() < 1e-5
    flat_d, prm_d = torch.from_numpy(flat).to(dev), torch.from_numpy(prm).to(dev)
    keep = torch.from_numpy(flat).to(dev)
    for _ in range(calls):
        L.check(_adam_call(lib, dev, flat_d, NP_B, prm_d, opt, bl), "qc_balance_adam_step")
        flat_d.copy_(keep)
    torch.cuda.synchronize(dev)
    s_dev = np.asarray(scale) * prm_d.cpu().numpy().astype(np.float64)[NP:]
    print("device: s", s_dev, "difference to the replay", np.abs(s_dev - s_ref))
    # 300 float32 Adam steps of a contracting iteration against float64 (5e-8 in the emulation): the replay's own distance
    # to the fixed point bounds it
    assert np.abs(s_dev - s_ref).max() < 1e-5 and np.abs(s_dev - s_fix).max() < 2e-5
    assert opt.read()["step"] == calls and np.array_equal(prm_d.cpu().numpy()[:NP], prm[:NP])      # zero gradient: unmoved


# ---- 7. one update through the step: the folding kernel
def test_one_update_through_the_step(gpu_device):
    L = pkg("hip.lib")
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = BR.CASES[case]
    flat, *batch = BR.case_inputs(case)
    rec = BR.class_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    fs = _balanced_step(eng, B_res, n_ic, n_bc, hist_cap=3)
    _load(fs, *batch)
    NP = eng.NP
    p_before = fs.flat.clone()
    fs.run(L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE)
    torch.cuda.synchronize()
    got = fs.flat_grad.cpu().numpy().astype(np.float64)
    own = BR.own_gradient(rec["parts"])
    we = np.asarray(BR.W) * BR.factors()
    bound = np.abs(np.asarray(BR.SCALE)) * we * TOL_L * max(1.0, np.abs(rec["parts"]).max())
    print("own gradient", got[NP:NP + N_BAL], "reference", own, "bound", bound)
    assert (np.abs(got[NP:NP + N_BAL] - own) <= bound).all()
    # the clipped network gradient next to them: the reference scaled by the clip of ITS first NP entries
    ref = BR.combine(rec)[:NP]
    norm = np.sqrt((ref ** 2).sum())
    err = _tab_errors(np.concatenate([got[:NP], got[NP + N_BAL:]]), ref * min(1.0, 1.0 / (norm + 1e-6)), rec["parts"], n, eng.n_theta)
    assert max(err.values()) < 1.0, err
    r = fs.opt.read()
    assert r["step"] == 1 and r["grad_norm"] == pytest.approx(norm, rel=TOL_G)
    assert (r["loss_res"], r["loss_bc"], r["loss_ic"]) == pytest.approx(tuple(rec["parts"]), abs=TOL_L * max(1.0, rec["parts"].max()))
    F = BR.objective(rec["parts"])
    assert fs.opt.loss_history(1)[0] == pytest.approx(F, abs=1e-4 * max(1.0, abs(F))) and r["loss"] == fs.opt.loss_history(1)[0]
    wh = fs.weight_hist.cpu().numpy()
    want_w = device_weights(gpu_device)
    assert np.array_equal(wh[0].view(np.uint32), want_w.view(np.uint32)) and np.isnan(wh[1:]).all()
    moved = (fs.flat - p_before).cpu().numpy()
    assert (np.abs(moved[NP:]) > 0.9 * 0.005).all() and (np.abs(moved[NP:]) < 1.001 * 0.005).all()      # Adam's first step
    assert (np.sign(moved[NP:]) == -np.sign(own)).all()


# ---- 8. refusals
def test_refusals_name_one_fault_each(gpu_device):
    """A descriptor that runs (rc 0), then the same descriptor with ONE fault: -1, and nothing written."""
    L = pkg("hip.lib")
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = BR.CASES[case]
    flat, *batch = BR.case_inputs(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    fs = _balanced_step(eng, B_res, n_ic, n_bc, hist_cap=2)
    _load(fs, *batch)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    ref = lambda s: None if s is None else C.byref(s)
    call = lambda desc, data, bl, phases=L.QC_PHASE_GRADS: eng.lib.qc_fused_pinn_balanced_step(ref(desc), ref(data), ref(bl), phases, st)
    assert call(fs.desc, fs.data, fs.bal) == 0
    torch.cuda.synchronize()
    fs.flat_grad.fill_(NAN)
    fs.part.fill_(NAN)
    fs.weight_hist.fill_(NAN)

    def broken(src, **kw):
        t = type(src).from_buffer_copy(src)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(t, k)[v[0]] = v[1]
            else:
                setattr(t, k, v)
        return t
    assert call(fs.desc, fs.data, None) == -1 and call(fs.desc, None, fs.bal) == -1
    for kw in (dict(scale=(0, NAN)), dict(scale=(2, float("inf"))), dict(scale=(1, -float("inf"))), dict(weight_hist_cap=-1),
               dict(weight_hist_dev=None)):
        assert call(fs.desc, fs.data, broken(fs.bal, **kw)) == -1, kw
        assert call(fs.desc, fs.data, broken(fs.bal, **kw), L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE) == -1, kw
    assert call(broken(fs.desc, part_stride=fs.stride - 1), fs.data, fs.bal) == -1          # NP_B + 2
    assert call(broken(fs.desc, part_stride=eng.NP + 3), fs.data, fs.bal) == -1             # the data step's stride
    # whatever the data step refuses
    assert call(fs.desc, broken(fs.data, target_res_dev=None), fs.bal) == -1
    assert call(fs.desc, broken(fs.data, target_val_dev=None), fs.bal) == -1
    assert call(fs.desc, fs.data, fs.bal, L.QC_PHASE_GRADS | L.QC_PHASE_SAMPLE) == -1       # no dataset
    for pb in (0, 1, 2, 4):
        fs.desc.pde.problem = pb
        assert call(fs.desc, fs.data, fs.bal) == -1
    fs.desc.pde.problem = L.QC_PROBLEM_TABULATED
    # the optimiser call: theta must lie in front of the balancer's entries
    opt = fs.opt
    adam = lambda NP_B, theta_off: _adam_call(eng.lib, gpu_device, fs.flat_grad, NP_B, fs.flat, opt, fs.bal, eng.circuit.handle,
                                              theta_off, eng.circuit.trig.data_ptr())
    assert adam(fs.NP_B, fs.theta_off + 1) == -1 and adam(fs.NP_B - 1, fs.theta_off) == -1 and adam(fs.NP_B, -1) == -1
    torch.cuda.synchronize()
    assert torch.isnan(fs.flat_grad).all() and torch.isnan(fs.part).all() and torch.isnan(fs.weight_hist).all()
    assert opt.read()["step"] == 0
    assert call(fs.desc, fs.data, fs.bal) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(fs.flat_grad).all()
