"""The tabulated step on the GPU, through the C ABI: qc_fused_pinn_data_step (QC_PHASE_GRADS) against the float64
reference with targets as arrays (tests/tabulated_reference.py) in every circuit family and form, its agreement with the
analytic step, qc_post_data alone, the bits of the dataset gather, and training on a device-resident dataset against a
float64 replay.

Targets are float32 roundings of u* = sin(2 pi x) cos(pi y) exp(-t / 2) + 0.3 and r* = 1.5 cos(3 t + x - 2 y), the operator
has c_u = 0.7 and no coefficient at its default.  Tolerances are those of tests/test_gpu_fused_families.py: the gradient
block by block (pre network, theta, post network) at 2e-4 x max(1, max |ref block|), the loss parts at 1e-4.  Negative
controls (residual targets rolled by one point, value targets rolled by one, c_u = 0) must fail the same tolerance;
tests/test_tabulated_cpu.py shows that each differs from the true reference by more than ten times it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlp_reference as R
import tabulated_reference as T
import tabulated_training as TT
from conftest import GOLDEN, pkg
from test_gpu_fullsize import Log, base_args

pytestmark = pytest.mark.gpu

H = T.H
TOL_G, TOL_L = 2e-4, 1e-4
THETA_MIN = 20 * TOL_G
MERGED = ("reg_cascade4", "reg_cascade4_H129", "reg_cascade2", "reg_cascade5")


def _model(gpu_device, ans, n, L, enc, flat=None, hidden=H):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, encoding=enc,
                             classic_network=[3, hidden, 1]), Log(), device=gpu_device)
    eng = model._engine_for(gpu_device)
    if flat is not None:
        with torch.no_grad():
            eng.flat.copy_(torch.from_numpy(np.asarray(flat, dtype=np.float32)))
    return model, eng


def _tabulated_step(eng, B_res, n_ic, n_bc, coeffs=T.COEFFS, c_u=T.C_U):
    """A FusedStep of the tabulated problem with poisoned workspace and targets."""
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    eng.problem, eng.coeffs, eng.c_u = L.QC_PROBLEM_TABULATED, coeffs, c_u
    eng.refresh_gates()
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, eng.device),
                          (max(B_res, 1), max(n_ic, 1), max(n_bc, 1)))
    assert fs.tabulated
    if fs.step_ws.numel() >= 4:
        nfl = fs.step_ws.numel() // 4
        fs.step_ws[: 4 * nfl].view(torch.float32).fill_(float("nan"))
    fs.target_res.fill_(float("nan"))
    fs.target_val.fill_(float("nan"))
    return fs


def _load(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res):
    dev = fs.eng.device
    n_ic, n_bc, B_res = len(X_ic), len(X_bc), len(X_res)
    to = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(dev)
    if B_res:
        fs.X_res[:B_res], fs.target_res[:B_res] = to(X_res), to(r_res)
    if n_ic:
        fs.X_val[:n_ic], fs.target_val[:n_ic] = to(X_ic), to(u_ic)
    if n_bc:
        fs.X_val[n_ic:n_ic + n_bc], fs.target_val[n_ic:n_ic + n_bc] = to(X_bc), to(u_bc)


def data_grads(eng, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coeffs=T.COEFFS, c_u=T.C_U):
    """flat [grad | L_r, L_bc, L_ic] of qc_fused_pinn_data_step's gradient phase on the given batches and targets."""
    L = pkg("hip.lib")
    fs = _tabulated_step(eng, len(X_res), len(X_ic), len(X_bc), coeffs, c_u)
    _load(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res)
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    return fs.flat_grad.cpu().numpy().astype(np.float64)


def _blocks(n, n_theta, hidden=H):
    lay = pkg("hip.engine").param_layout(hidden, n, n_theta)
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    return {"pre": slice(0, o_post), "theta": slice(o_th, NP), "post": slice(o_post, o_th)}


def _errors(got, want_g, want_p, n, n_theta):
    """name -> error / tolerance (< 1 passes) of the three gradient blocks and the loss parts."""
    NP = got.size - 3
    hidden = (NP - n_theta - 1 - n) // (6 + 2 * n)          # NP = H (3 + 1 + n + n + 1 + 1) + n + 1 + n_theta
    out = {"parts": np.abs(got[NP:] - want_p).max() / (TOL_L * max(1.0, np.abs(want_p).max()))}
    for name, s in _blocks(n, n_theta, hidden).items():
        if s.stop > s.start:
            out[name] = np.abs(got[:NP][s] - want_g[s]).max() / (TOL_G * max(1.0, np.abs(want_g[s]).max()))
    return out


def _merged_probe(eng, B_res, n_ic, n_bc):
    """0 when a step of these sizes takes the merged form (qc_fused_step_stage is analytic-only: probed on problem 0)."""
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    keep = eng.problem, eng.coeffs, eng.c_u
    eng.problem, eng.coeffs, eng.c_u = L.QC_PROBLEM_CONVECTION_DIFFUSION, None, 0.0
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, eng.device))
    rc = eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_PRE_FWD, torch.cuda.current_stream(eng.device).cuda_stream)
    torch.cuda.synchronize()
    eng.problem, eng.coeffs, eng.c_u = keep
    return rc


# ---- 6. the data step against the float64 reference in every family and form
@pytest.mark.parametrize("case", list(T.CASES))
def test_data_step_matches_fp64(case, gpu_device):
    ans, n, Lq, enc, B_res, n_ic, n_bc = T.CASES[case]
    flat, *batch = T.case_inputs(case)
    ref = T.case_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat, T.case_H(case))
    n_theta = eng.n_theta
    got = data_grads(eng, *batch)
    assert np.isfinite(got).all() and eng.H == T.case_H(case)
    err = _errors(got, ref["grad"], ref["parts"], n, n_theta)
    print(case, {k: round(float(v), 4) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    assert np.abs(ref["grad"][_blocks(n, n_theta, eng.H)["theta"]]).max() > THETA_MIN
    if 2 <= n <= 5:
        merged = case in MERGED and os.environ.get("QC_NO_MERGE") != "1"
        assert (_merged_probe(eng, B_res, n_ic, n_bc) == 0) == merged
    for v in T.CONTROLS.get(case, ()):
        bad = T.case_reference(case, v)
        berr = _errors(got, bad["grad"], bad["parts"], n, n_theta)
        print(case, v, {k: round(float(x), 2) for k, x in berr.items()})
        assert max(berr.values()) > 1.0, (v, berr)


@pytest.mark.parametrize("env", [{"QC_NO_STATIC": "1"}, {"QC_NO_MERGE": "1"}], ids=["no_static", "no_merge"])
def test_switch_variants_pass_the_same_check(env):
    """The two cascade n = 4 cases (H = 50 and H = 129) through the circuit interpreter, and through the two-stream form
    (the switches are read once at load: a child process)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_tabulated.py"), "-m", "gpu", "-q", "-x",
                        "-k", "data_step_matches_fp64 and reg_cascade4"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-2000:]


# ---- 7. agreement with the analytic step
def test_data_step_with_analytic_targets_agrees_with_the_analytic_step(gpu_device):
    from oracle import solver as osol
    from test_gpu_fullsize import grads_for
    ans, n, Lq, enc, B_res, n_ic, n_bc = T.CASES["reg_cascade4"]
    flat, X_ic, X_bc, X_res, *_ = T.case_inputs("reg_cascade4")
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    want = grads_for(model, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)      # problem 0, in-kernel fp32 targets
    tg = [osol.analytic_u(X_ic.double())[:, 0].float().numpy(), osol.analytic_u(X_bc.double())[:, 0].float().numpy(),
          osol.analytic_r(X_res.double())[:, 0].float().numpy()]
    got = data_grads(eng, X_ic, X_bc, X_res, *tg, coeffs=None, c_u=0.0)
    err = _errors(got, want[:-3], want[-3:], n, eng.n_theta)
    print({k: float(v) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    assert np.abs(want[:-3]).max() > 0.1          # a gradient is there to agree on


# ---- 8. qc_post_data alone
POINT_TOL, ROW_TOL = 5e-5, 2e-4          # tests/test_gpu_mlp_shapes.py
ROW0, STRIDE_PAD, N_THETA = 2, 7, 3


@pytest.mark.parametrize("Hn", [(50, 4), (129, 3)], ids=["H50_n4_fused", "H129_n3_split"])
@pytest.mark.parametrize("nch", [6, 1])
def test_post_data_alone(Hn, nch, gpu_device):
    """B = 65 (two tiles, the second with one point) behind NaN-filled buffers, as test_post_network_every_mode does for
    qc_post mode 2; H = 129 takes the point kernel + weight-gradient kernel pair."""
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    (Hh, n), B, dev = Hn, 65, gpu_device
    g = np.random.default_rng(Hh + nch)
    lay, NP = R.layout(Hh, n, N_THETA)
    flat = np.full(NP, np.nan, np.float32)
    for k in ("W3", "b3", "W4", "b4"):
        o, s = lay[k]
        flat[o:o + int(np.prod(s))] = g.uniform(-1, 1, int(np.prod(s))) / np.sqrt({"W3": n, "b3": n}.get(k, Hh))
    q = np.concatenate([g.uniform(-1, 1, (1, n, B)), g.standard_normal((5, n, B))]).astype(np.float32)[:nch]
    target = g.standard_normal(B).astype(np.float32)
    c_u = 0.7
    pde = dict(D=0.01, vx=1.0, vy=1.0, c_t=1.3, c_x=0.7, c_y=-0.4, d_xx=0.02, d_yy=0.05, w_res=4.0 / B, inv_n_res=1.0 / B,
               w_val_a=0.3, w_val_b=0.7, inv_n_a=0.11, inv_n_b=0.13, problem=L.QC_PROBLEM_TABULATED, n_seg_a=B // 3)
    qpde = L.QcPde(**pde)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out_u, out_res, qbar = nan(B + 64), nan(B + 64), nan(nch * n * B + 64)
    part = nan(ROW0 + 2 + 2, NP + 3 + STRIDE_PAD)
    prm, qd, tg = (torch.from_numpy(a).to(dev) for a in (flat, q, target))
    L.check(lib.qc_post_data(prm.data_ptr(), Hh, n, N_THETA, C.byref(qpde), qd.data_ptr(), tg.data_ptr(), c_u,
                             out_u.data_ptr(), out_res.data_ptr() if nch == 6 else None, qbar.data_ptr(), part.data_ptr(),
                             part.shape[1], ROW0, B, nch, st), "qc_post_data")
    torch.cuda.synchronize(dev)
    names = ("W3", "b3", "W4", "b4")
    cols = np.concatenate([np.arange(lay[k][0], lay[k][0] + int(np.prod(lay[k][1]))) for k in names] + [[NP, NP + 1, NP + 2]])
    p = part.cpu().numpy()
    mask = np.zeros(p.shape, bool)
    mask[ROW0:ROW0 + 2, cols] = True
    assert np.isnan(p[~mask]).all() and np.isfinite(p[mask]).all()
    for buf, m in ((out_u, B), (out_res, B if nch == 6 else 0), (qbar, nch * n * B)):
        a = buf.cpu().numpy()
        assert np.isnan(a[m:]).all() and np.isfinite(a[:m]).all()

    def errors(c_u_ref, tgt):
        flat64 = np.nan_to_num(flat.astype(np.float64))
        P = R.unpack(flat64, Hh, n, N_THETA)
        qt = torch.from_numpy(q).double().requires_grad_(True)
        u = R.post_jets(P, qt)
        tt = torch.from_numpy(tgt).double()
        if nch == 6:
            e = c_u_ref * u[0] + R.residual(u, (pde["c_t"], pde["c_x"], pde["c_y"], pde["d_xx"], pde["d_yy"])) - tt
        else:
            e = u[0] - tt
        w = R.point_weights(B, pde, nch)
        obj = 0.5 * w * e * e
        cot = (w * e).detach().numpy()
        qb = torch.autograd.grad(obj.sum(), qt, retain_graph=True)[0].numpy()
        rows = np.stack([R.flatten(dict(zip(names, gr)), Hh, n, N_THETA) for gr in R.tile_grads(obj, [P[k] for k in names], B)])
        losses = np.stack([R.loss_parts(e[k:k + 64], dict(pde, n_seg_a=pde["n_seg_a"] - k), nch).detach().numpy()
                           for k in range(0, B, 64)])
        rel = lambda got, want, tol: np.abs(got - want).max() / (tol * max(1.0, np.abs(want).max()))
        out = {"qbar": rel(qbar.cpu().numpy()[:nch * n * B].reshape(nch, n, B), qb, POINT_TOL),
               "rows": rel(p[ROW0:ROW0 + 2][:, cols[:-3]], rows[:, cols[:-3]], ROW_TOL),
               "loss": rel(p[ROW0:ROW0 + 2][:, cols[-3:]], losses, ROW_TOL)}
        if nch == 6:
            out["rbar"] = rel(out_res.cpu().numpy()[:B], cot, POINT_TOL)
            out["ubar"] = rel(out_u.cpu().numpy()[:B], c_u_ref * cot, POINT_TOL)
        else:
            out["ubar"] = rel(out_u.cpu().numpy()[:B], cot, POINT_TOL)
        return out
    err = errors(c_u, target)
    print({k: float(v) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    assert max(errors(c_u, np.roll(target, 1)).values()) > 1.0          # the target of ANOTHER point is told apart
    if nch == 6:
        assert max(errors(0.0, target).values()) > 1.0                  # and so is a dropped c_u


# ---- 9. the gather's bits
DS_N = (1000, 7, 1)
BATCH = (130, 33, 31)


def _dataset(dev, sizes=DS_N, seed=5):
    g = np.random.default_rng(seed)
    arr = [(g.random((m, 3)).astype(np.float32), g.standard_normal(m).astype(np.float32)) for m in sizes]
    ten = [(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)) for X, y in arr]
    return arr, ten


def _step_data(L, ten, tr=None, tv=None):
    (Xr, rr), (Xi, ui), (Xb, ub) = ten
    return L.QcStepData(tr, tv, 0.0, Xr.data_ptr(), rr.data_ptr(), Xr.shape[0], Xi.data_ptr(), ui.data_ptr(), Xi.shape[0],
                        Xb.data_ptr(), ub.data_ptr(), Xb.shape[0])


def _expected(arr, offs, counts, seed, step):
    out = []
    for seg, ((X, y), off, cnt) in enumerate(zip(arr, offs, counts)):
        k = T.dataset_indices(seg, off, cnt, X.shape[0], seed, step)
        out.append((X[k], y[k]))
    (Xr, rr), (Xi, ui), (Xb, ub) = out
    return Xr, rr, np.concatenate([Xi, Xb]), np.concatenate([ui, ub])


def _gather(lib, L, dev, data, counts, offs, seed, step):
    n_res, n_ic, n_bc = counts
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    Xr, tr, Xv, tv = nan(n_res + 3, 3), nan(n_res + 3), nan(n_ic + n_bc + 3, 3), nan(n_ic + n_bc + 3)
    L.check(lib.qc_sample_dataset(Xr.data_ptr(), tr.data_ptr(), n_res, offs[0], Xv.data_ptr(), tv.data_ptr(), n_ic, offs[1],
                                  n_bc, offs[2], C.byref(data), seed, step, torch.cuda.current_stream(dev).cuda_stream),
            "qc_sample_dataset")
    torch.cuda.synchronize(dev)
    out = [t.cpu().numpy() for t in (Xr, tr, Xv, tv)]
    for a, m in zip(out, (n_res, n_res, n_ic + n_bc, n_ic + n_bc)):
        assert np.isnan(a[m:]).all(), "the gather wrote past its batch"
    return [a[:m] for a, m in zip(out, (n_res, n_res, n_ic + n_bc, n_ic + n_bc))]


def test_gather_bits_and_shards(gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    arr, ten = _dataset(gpu_device)
    data = _step_data(L, ten)
    seed, step = 0xC0FFEE1234567, (1 << 33) + 5
    got = _gather(lib, L, gpu_device, data, BATCH, (0, 0, 0), seed, step)
    want = _expected(arr, (0, 0, 0), BATCH, seed, step)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert len(np.unique(got[1])) > 100 and np.unique(got[3][:33]).size > 3          # rows of the whole dataset
    # two shards with offsets concatenate to the single call
    cut = (70, 20, 9)
    a = _gather(lib, L, gpu_device, data, cut, (0, 0, 0), seed, step)
    rest = tuple(b - c for b, c in zip(BATCH, cut))
    b = _gather(lib, L, gpu_device, data, rest, cut, seed, step)
    assert np.array_equal(np.concatenate([a[0], b[0]]), got[0]) and np.array_equal(np.concatenate([a[1], b[1]]), got[1])
    n_ic = BATCH[1]
    assert np.array_equal(np.concatenate([a[2][:cut[1]], b[2][:rest[1]]]), got[2][:n_ic])
    assert np.array_equal(np.concatenate([a[2][cut[1]:], b[2][rest[1]:]]), got[2][n_ic:])
    assert np.array_equal(np.concatenate([a[3][:cut[1]], b[3][:rest[1]], a[3][cut[1]:], b[3][rest[1]:]]), got[3])
    # a global index past 2^32 reaches the high counter word
    far = _gather(lib, L, gpu_device, data, (5, 0, 0), ((1 << 32) + 3, 0, 0), seed, step)
    assert np.array_equal(far[1], _expected(arr, ((1 << 32) + 3, 0, 0), (5, 0, 0), seed, step)[1])


def test_sample_phase_of_the_merged_step_leaves_the_gathered_batch(gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    ans, n, Lq, enc, B_res, n_ic, n_bc = T.CASES["reg_cascade4"]
    flat, *_ = T.case_inputs("reg_cascade4")
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    assert (_merged_probe(eng, B_res, n_ic, n_bc) == 0) == (os.environ.get("QC_NO_MERGE") != "1")
    arr, ten = _dataset(gpu_device, (300, 40, 50), seed=8)
    tg = lambda X: T.u_star(X)
    arr = [(X, tg(X)) for X, _ in arr]
    ten = [(torch.from_numpy(X).to(gpu_device), torch.from_numpy(y).to(gpu_device)) for X, y in arr]
    fs = _tabulated_step(eng, B_res, n_ic, n_bc)
    fs.set_dataset(ten)
    fs.set_sampler(0xABCDEF, 11, 5, 7)
    fs.run(L.QC_PHASE_SAMPLE | L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    step = fs.desc.sample_step
    assert step == 1
    alone = _gather(lib, L, gpu_device, _step_data(L, ten), (B_res, n_ic, n_bc), (11, 5, 7), 0xABCDEF, step)
    for got, want in zip((fs.X_res[:B_res], fs.target_res[:B_res], fs.X_val[:n_ic + n_bc], fs.target_val[:n_ic + n_bc]), alone):
        assert np.array_equal(got.cpu().numpy(), want)
    want = _expected(arr, (11, 5, 7), (B_res, n_ic, n_bc), 0xABCDEF, step)
    assert np.array_equal(alone[0], want[0]) and np.array_equal(alone[3], want[3])
    # and the gradient of that call is the gradient on the gathered batch
    got = fs.flat_grad.cpu().numpy().astype(np.float64)
    again = data_grads(eng, want[2][:n_ic], want[2][n_ic:], want[0], want[3][:n_ic], want[3][n_ic:], want[1])
    assert np.array_equal(got, again)


def test_refusals_name_one_fault_each(gpu_device):
    """A descriptor that runs (rc 0), then the same descriptor with ONE fault: -1, and nothing written."""
    L = pkg("hip.lib")
    ans, n, Lq, enc, B_res, n_ic, n_bc = T.CASES["reg_cascade4"]
    flat, *batch = T.case_inputs("reg_cascade4")
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    _, ten = _dataset(gpu_device, (300, 40, 50), seed=8)
    fs = _tabulated_step(eng, B_res, n_ic, n_bc)
    _load(fs, *batch)
    fs.set_dataset(ten)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    both = L.QC_PHASE_GRADS | L.QC_PHASE_SAMPLE
    call = lambda data, phases, desc=fs.desc: eng.lib.qc_fused_pinn_data_step(C.byref(desc), C.byref(data), phases, st)
    assert call(fs.data, L.QC_PHASE_GRADS) == 0 and call(fs.data, both) == 0
    torch.cuda.synchronize()
    fs.flat_grad.fill_(float("nan"))
    fs.X_res.fill_(float("nan"))

    def broken(**kw):
        t = L.QcStepData.from_buffer_copy(fs.data)
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    assert call(broken(target_res_dev=None), L.QC_PHASE_GRADS) == -1
    assert call(broken(target_val_dev=None), L.QC_PHASE_GRADS) == -1
    for kw in (dict(ds_n_res=0), dict(ds_X_ic=None), dict(ds_u_bc=None), dict(ds_n_bc=2 ** 31), dict(ds_n_ic=-1)):
        assert call(broken(**kw), both) == -1, kw
    for pb in (0, 1, 2, 4):
        fs.desc.pde.problem = pb
        assert call(fs.data, L.QC_PHASE_GRADS) == -1
    fs.desc.pde.problem = L.QC_PROBLEM_TABULATED
    assert eng.lib.qc_fused_pinn_residual_step(C.byref(fs.desc), L.QC_PHASE_GRADS, st) == -1
    assert eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_POST, st) == -1
    torch.cuda.synchronize()
    assert torch.isnan(fs.flat_grad).all() and torch.isnan(fs.X_res).all()


# ---- 10. training on a device-resident dataset
@pytest.mark.parametrize("case", list(TT.TRAIN_CASES))
def test_training_on_a_dataset_matches_the_fp64_replay(case, gpu_device, tmp_path):
    trainer = pkg("trainer.diffusion_train")
    TP = pkg("data.tabulated").TabulatedProblem
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    ans, n = TT.TRAIN_CASES[case]

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(TT.base_args(ans, n), TmpLog(), device=gpu_device)
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in TT.dataset_arrays())
    co = dict(zip(("c_t", "c_x", "c_y", "d_xx", "d_yy"), T.COEFFS), c_u=T.C_U)
    ds = TP(Xr, rr, Xi, ui, Xb, ub, **co)
    torch.manual_seed(TT.TRAINER_SEED_AT)
    tr = trainer.FusedTrainer(model, TT.BATCH, capacity=TT.STEPS, dataset=ds)
    assert tr.fs.desc.sample_seed == TT.trainer_seed() and tr.fs.tabulated
    batches = []
    for _ in range(TT.STEPS):
        tr.sample()
        tr.step()
        fs = tr.fs
        Xv, tv = fs.X_val.cpu().numpy(), fs.target_val.cpu().numpy()
        batches.append((Xv[:TT.N_IC], Xv[TT.N_IC:TT.N_IC + TT.N_BC], fs.X_res.cpu().numpy()[:TT.BATCH], tv[:TT.N_IC],
                        tv[TT.N_IC:TT.N_IC + TT.N_BC], fs.target_res.cpu().numpy()[:TT.BATCH]))
    for got, want in zip(batches, TT.expected_batches()):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    got = np.array(tr.opt.loss_history(TT.STEPS))
    want = TT.training_reference(case, batches)["loss"]
    print(case, got, want)
    assert got.shape == want.shape == (TT.STEPS,)
    assert np.abs(got - want).max() < 1e-4 * max(1.0, np.abs(want).max()), (got, want)
    assert len(set(np.round(want, 6))) == TT.STEPS          # six different batches, six different losses
    model.save_state()
    state = Solver.load_state(os.path.join(model.log_path, "model.pth"))
    assert isinstance(state, dict) and state


# ---- 11. targets need a tabulated step; the analytic training of the same model is untouched
def test_targets_need_a_dataset_and_the_analytic_train_still_trains_problem_0(gpu_device):
    trainer = pkg("trainer.diffusion_train")
    TP = pkg("data.tabulated").TabulatedProblem
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    z = np.load(os.path.join(GOLDEN, "train_cascade_n4_b64.npz"))
    torch.manual_seed(1)
    model = Solver(base_args(), Log(), device=gpu_device)
    B = int(z["batch_size"])
    Xs = [torch.from_numpy(z[k][0]) for k in ("X_ic", "X_bc", "X_res")]
    tg = (T.u_star(Xs[0]), T.u_star(Xs[1]), T.r_star(Xs[2]))
    with pytest.raises(ValueError, match="tabulated"):
        trainer.FusedTrainer(model, B, capacity=1).load_batches(*Xs, targets=tg)
    # a tabulated trainer on the same model: targets required, then one step on them
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in TT.dataset_arrays())
    tr = trainer.FusedTrainer(model, B, capacity=1, dataset=TP(Xr, rr, Xi, ui, Xb, ub, c_u=T.C_U))
    with pytest.raises(ValueError, match="targets"):
        tr.load_batches(*Xs)
    w0 = model._engine_for(gpu_device).flat.clone()
    tr.load_batches(*Xs, targets=tg)
    tr.step()
    first_tab = tr.losses()[0][0]
    # the old train() on the same model and weights: problem 0 again, the first loss of the reference's own run
    with torch.no_grad():
        model._engine_for(gpu_device).flat.copy_(w0)
    model.loss_history.clear()
    trainer.train(model, batch_size=B, batches=[tuple(Xs)])
    ref0 = float(z["loss_history"][0])
    assert abs(model.loss_history[0] - ref0) < 1e-4 * max(1.0, ref0), (model.loss_history, ref0)
    assert abs(first_tab - ref0) > 1e-2          # the tabulated step trained towards other targets
