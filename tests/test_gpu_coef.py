"""The coefficient step on the GPU, through the C ABI: qc_post_coef alone, qc_fused_pinn_coef_step (QC_PHASE_GRADS)
against the float64 reference with one operator row per residual point (tests/coef_reference.py) in every circuit family
and form, its agreement with the data step on a uniform table, the bits of the gather with coefficient rows, the
refusals, and training on a coefficient dataset against a float64 replay.

The cases are those of tests/test_gpu_tabulated.py (same weights, points, targets) with the table coef_reference.coef_star:
smooth fields, c_u and c_3 of both signs, every fifth row the flux row (0, 0, 1, 0, 0, 0, 0).  Tolerances are the
project's: the gradient block by block at 2e-4 x max(1, max |ref block|), the loss parts at 1e-4, POINT_TOL / ROW_TOL of
the post-stage tests, 1e-4 on a loss history.  Negative controls (table rolled by one point, c_3 zeroed, d_xx / d_yy
swapped) must fail the same tolerance; tests/test_coef_cpu.py shows that each differs from the truth by far more."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coef_reference as CR
import coef_training as CT
import mlp_reference as R
import tabulated_reference as T
import tabulated_training as TT
from conftest import GOLDEN, pkg
from test_gpu_fullsize import Log
from test_gpu_tabulated import (BATCH, DS_N, MERGED, POINT_TOL, ROW_TOL, THETA_MIN, TOL_G, TOL_L, _blocks, _dataset, _errors,
                                _load, _merged_probe, _model, _step_data, data_grads)

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _coef_step(eng, B_res, n_ic, n_bc):
    """A FusedStep in coefficient mode behind poisoned buffers.  The scalar operator of the descriptor is NaN: the
    coefficient step must not read pde.c_t .. d_yy or data->c_u."""
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    eng.problem, eng.coeffs, eng.c_u, eng.coef_mode = L.QC_PROBLEM_TABULATED, (NAN,) * 5, NAN, True
    eng.refresh_gates()
    try:
        fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, eng.device),
                              (max(B_res, 1), max(n_ic, 1), max(n_bc, 1)))
    finally:
        eng.coef_mode = False
    assert fs.tabulated and fs.coef_mode and fs.coef_res.shape == (7, max(B_res, 1))
    if fs.step_ws.numel() >= 4:
        nfl = fs.step_ws.numel() // 4
        fs.step_ws[: 4 * nfl].view(torch.float32).fill_(NAN)
    for buf in (fs.target_res, fs.target_val, fs.coef_res, fs.ws_res, fs.ws_val):
        buf.fill_(NAN)
    return fs


def _load_coef(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef):
    _load(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res)
    if len(X_res):
        fs.coef_res[:, :len(X_res)] = torch.as_tensor(np.asarray(coef), dtype=torch.float32).to(fs.eng.device).t()


def coef_grads(eng, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef):
    """flat [grad | L_r, L_bc, L_ic] of qc_fused_pinn_coef_step's gradient phase on the given batches, targets and rows."""
    L = pkg("hip.lib")
    fs = _coef_step(eng, len(X_res), len(X_ic), len(X_bc))
    _load_coef(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef)
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    return fs.flat_grad.cpu().numpy().astype(np.float64)


# ---- 1. qc_post_coef alone
ROW0, STRIDE_PAD, N_THETA = 2, 7, 3


def _post_coef(lib, L, dev, flat, Hh, n, n_theta, q, target, coef, pde, row0=ROW0, pad=STRIDE_PAD):
    """qc_post_coef behind NaN-filled outputs -> (cot, qbar, part) numpy, after checking nothing else was written."""
    B = q.shape[2]
    NP = R.layout(Hh, n, n_theta)[1]
    nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device=dev)
    tiles = (B + 63) // 64
    cot, qbar, part = nan(6 * B + 64), nan(6 * n * B + 64), nan(row0 + tiles + 2, NP + 3 + pad)
    prm, qd, tg, cf = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (flat, q, target, coef.T))
    qpde = L.QcPde(**pde)
    L.check(lib.qc_post_coef(prm.data_ptr(), Hh, n, n_theta, C.byref(qpde), qd.data_ptr(), tg.data_ptr(), cf.data_ptr(),
                             cot.data_ptr(), qbar.data_ptr(), part.data_ptr(), part.shape[1], row0, B,
                             torch.cuda.current_stream(dev).cuda_stream), "qc_post_coef")
    torch.cuda.synchronize(dev)
    for buf, m in ((cot, 6 * B), (qbar, 6 * n * B)):
        a = buf.cpu().numpy()
        assert np.isnan(a[m:]).all() and np.isfinite(a[:m]).all()
    return cot.cpu().numpy()[:6 * B].reshape(6, B), qbar.cpu().numpy()[:6 * n * B].reshape(6, n, B), part.cpu().numpy()


@pytest.mark.parametrize("Hn", [(50, 4), (129, 3)], ids=["H50_n4_fused", "H129_n3_split"])
def test_post_coef_alone(Hn, gpu_device):
    """B = 65 (two tiles, the second with one point); H = 129 takes the point kernel + weight-gradient kernel pair, whose
    second kernel reads the six cotangents in its gen mode.  pde.c_t .. d_yy are NaN: not read."""
    L = pkg("hip.lib")
    lib = L.load()
    (Hh, n), B = Hn, 65
    g = np.random.default_rng(Hh + 6)
    lay, NP = R.layout(Hh, n, N_THETA)
    flat = np.full(NP, np.nan, np.float32)
    for k in ("W3", "b3", "W4", "b4"):
        o, s = lay[k]
        flat[o:o + int(np.prod(s))] = g.uniform(-1, 1, int(np.prod(s))) / np.sqrt({"W3": n, "b3": n}.get(k, Hh))
    q = np.concatenate([g.uniform(-1, 1, (1, n, B)), g.standard_normal((5, n, B))]).astype(np.float32)
    target = g.standard_normal(B).astype(np.float32)
    coef = CR.coef_star(g.random((B, 3)))
    pde = dict(D=0.01, vx=1.0, vy=1.0, c_t=NAN, c_x=NAN, c_y=NAN, d_xx=NAN, d_yy=NAN, w_res=4.0 / B, inv_n_res=1.0 / B,
               w_val_a=0.3, w_val_b=0.7, inv_n_a=0.11, inv_n_b=0.13, problem=L.QC_PROBLEM_TABULATED, n_seg_a=B // 3)
    cot, qbar, p = _post_coef(lib, L, gpu_device, flat, Hh, n, N_THETA, q, target, coef, pde)
    names = ("W3", "b3", "W4", "b4")
    cols = np.concatenate([np.arange(lay[k][0], lay[k][0] + int(np.prod(lay[k][1]))) for k in names] + [[NP, NP + 1, NP + 2]])
    mask = np.zeros(p.shape, bool)
    mask[ROW0:ROW0 + 2, cols] = True
    assert np.isnan(p[~mask]).all() and np.isfinite(p[mask]).all()

    def errors(tab):
        flat64 = np.nan_to_num(flat.astype(np.float64))
        P = R.unpack(flat64, Hh, n, N_THETA)
        qt = torch.from_numpy(q).double().requires_grad_(True)
        u = R.post_jets(P, qt)
        u.retain_grad()
        e = CR.residual_coef(u, tab) - torch.from_numpy(target).double()
        obj = 0.5 * pde["w_res"] * e * e
        qb = torch.autograd.grad(obj.sum(), qt, retain_graph=True)[0].numpy()
        ub = torch.autograd.grad(obj.sum(), u, retain_graph=True)[0].numpy()          # (6, B): d obj / d u channels
        rows = np.stack([R.flatten(dict(zip(names, gr)), Hh, n, N_THETA) for gr in R.tile_grads(obj, [P[k] for k in names], B)])
        losses = np.stack([R.loss_parts(e[k:k + 64], pde, 6).detach().numpy() for k in range(0, B, 64)])
        rel = lambda got, want, tol: np.abs(got - want).max() / (tol * max(1.0, np.abs(want).max()))
        return {"cot": rel(cot, ub, POINT_TOL), "qbar": rel(qbar, qb, POINT_TOL),
                "rows": rel(p[ROW0:ROW0 + 2][:, cols[:-3]], rows[:, cols[:-3]], ROW_TOL),
                "loss": rel(p[ROW0:ROW0 + 2][:, cols[-3:]], losses, ROW_TOL)}
    err = errors(coef)
    print({k: float(v) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    # the b4 column is the sum of the first cotangent
    b4 = lay["b4"][0]
    want_b4 = np.array([cot[0, :64].astype(np.float64).sum(), cot[0, 64:].astype(np.float64).sum()])
    assert np.abs(p[ROW0:ROW0 + 2, b4] - want_b4).max() < ROW_TOL * max(1.0, np.abs(want_b4).max())
    for v in ("roll", "c3zero", "swap_d"):
        bad = errors(CR.variant_table(v, coef))
        print(v, {k: round(float(x), 1) for k, x in bad.items()})
        assert max(bad.values()) > 1.0, (v, bad)


def test_klein_gordon_fixture_through_the_kernels(gpu_device):
    """qc_pre_forward -> qc_forward_jets -> qc_post_coef with the Klein-Gordon rows and target 0 on the weights and points
    of tests/golden/other_operators.npz (a [3, 16, 1] model, zero first column, (t, x) on the x / y slots): the L_r column
    sums to mean(klein_gordon__out1^2), the reference's own operator on its own model."""
    from test_coef_cpu import kg_inputs
    L = pkg("hip.lib")
    z = np.load(os.path.join(GOLDEN, "other_operators.npz"))
    flat, X = kg_inputs(z)
    model, eng = _model(gpu_device, "cascade", 4, 1, "None", flat, hidden=16)
    B = len(X)
    _, _, _, qjets = eng.forward(X.to(gpu_device), 6)
    pde = dict(D=0.0, vx=0.0, vy=0.0, c_t=NAN, c_x=NAN, c_y=NAN, d_xx=NAN, d_yy=NAN, w_res=2.0 / B, inv_n_res=1.0 / B,
               w_val_a=0.0, w_val_b=0.0, inv_n_a=0.0, inv_n_b=0.0, problem=L.QC_PROBLEM_TABULATED, n_seg_a=0)
    cot, qbar, p = _post_coef(eng.lib, L, gpu_device, eng.flat.cpu().numpy(), 16, 4, eng.n_theta, qjets.cpu().numpy(),
                              np.zeros(B, np.float32), np.tile(CR.KLEIN_GORDON_ROW, (B, 1)), pde, row0=0, pad=0)
    want = float((z["klein_gordon__out1"].astype(np.float64) ** 2).mean())
    got = float(p[:1, eng.NP].astype(np.float64).sum())
    print(got, want)
    assert abs(got - want) < 1e-4 * max(1.0, want), (got, want)
    assert want > 1e-3


# ---- 2. the step against float64 in every family and form
@pytest.mark.parametrize("case", list(CR.CASES))
def test_coef_step_matches_fp64(case, gpu_device):
    ans, n, Lq, enc, B_res, n_ic, n_bc = CR.CASES[case]
    flat, *batch = CR.case_inputs(case)
    coef = CR.case_table(case)
    ref = CR.case_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat, CR.case_H(case))
    n_theta = eng.n_theta
    got = coef_grads(eng, *batch, coef)
    assert np.isfinite(got).all() and eng.H == CR.case_H(case)
    err = _errors(got, ref["grad"], ref["parts"], n, n_theta)
    print(case, {k: round(float(v), 4) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    assert np.abs(ref["grad"][_blocks(n, n_theta, eng.H)["theta"]]).max() > THETA_MIN
    if 2 <= n <= 5:
        merged = case in MERGED and os.environ.get("QC_NO_MERGE") != "1"
        assert (_merged_probe(eng, B_res, n_ic, n_bc) == 0) == merged
    for v in CR.CONTROLS.get(case, ()):
        bad = CR.case_reference(case, v)
        berr = _errors(got, bad["grad"], bad["parts"], n, n_theta)
        print(case, v, {k: round(float(x), 2) for k, x in berr.items()})
        assert max(berr.values()) > 1.0, (v, berr)


# ---- 3. switch variants
@pytest.mark.parametrize("env", [{"QC_NO_STATIC": "1"}, {"QC_NO_MERGE": "1"}], ids=["no_static", "no_merge"])
def test_switch_variants_pass_the_same_check(env):
    """The two cascade n = 4 cases (H = 50 and H = 129) through the circuit interpreter, and through the two-stream form
    (the switches are read once at load: a child process)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_coef.py"), "-m", "gpu", "-q", "-x",
                        "-k", "coef_step_matches_fp64 and reg_cascade4"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-2000:]


# ---- 4. a uniform table against the data step
def test_uniform_table_agrees_with_the_data_step(gpu_device):
    """The same batch through qc_fused_pinn_data_step (scalar operator) and through the coefficient step on the uniform
    table with c_3 = 0: both pass the float64 check of the data step's own record; their mutual difference is printed
    (bit equality is not required: the products of the residual associate differently)."""
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = CR.CASES[case]
    flat, *batch = CR.case_inputs(case)
    ref = CR.uniform_reference(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    a = data_grads(eng, *batch)
    b = coef_grads(eng, *batch, CR.uniform_table(B_res, T.COEFFS, T.C_U))
    for got in (a, b):
        err = _errors(got, ref["grad"], ref["parts"], n, eng.n_theta)
        assert max(err.values()) < 1.0, err
    diff = np.abs(a - b).max() / max(1.0, np.abs(a).max())
    print("largest mutual difference, relative to max(1, max |flat|):", diff)
    assert diff < TOL_G


# ---- 5. the gather
def _gather_coef(lib, L, dev, data, table, counts, offs, seed, step):
    n_res, n_ic, n_bc = counts
    nan = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=dev)
    Xr, tr, Xv, tv = nan(n_res + 3, 3), nan(n_res + 3), nan(n_ic + n_bc + 3, 3), nan(n_ic + n_bc + 3)
    cf = nan(7 * n_res + 5)
    coef = L.QcStepCoef(cf.data_ptr(), table.data_ptr())
    L.check(lib.qc_sample_dataset_coef(Xr.data_ptr(), tr.data_ptr(), n_res, offs[0], Xv.data_ptr(), tv.data_ptr(), n_ic,
                                       offs[1], n_bc, offs[2], cf.data_ptr(), C.byref(data), C.byref(coef), seed, step,
                                       torch.cuda.current_stream(dev).cuda_stream), "qc_sample_dataset_coef")
    torch.cuda.synchronize(dev)
    out = [t.cpu().numpy() for t in (Xr, tr, Xv, tv, cf)]
    sizes = (n_res, n_res, n_ic + n_bc, n_ic + n_bc, 7 * n_res)
    for a, m in zip(out, sizes):
        assert np.isnan(a[m:]).all(), "the gather wrote past its batch"
    out = [a[:m] for a, m in zip(out, sizes)]
    out[4] = out[4].reshape(7, n_res).T          # (n_res, 7) rows
    return out


def _expected_coef(arr, table, offs, counts, seed, step):
    from test_gpu_tabulated import _expected
    k = T.dataset_indices(0, offs[0], counts[0], arr[0][0].shape[0], seed, step)
    return list(_expected(arr, offs, counts, seed, step)) + [table[k]]


def test_gather_bits_and_shards(gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    arr, ten = _dataset(gpu_device)
    table = CR.coef_star(arr[0][0])
    tab_dev = torch.from_numpy(table).to(gpu_device)
    data = _step_data(L, ten)
    seed, step = 0xC0FFEE1234567, (1 << 33) + 5
    got = _gather_coef(lib, L, gpu_device, data, tab_dev, BATCH, (0, 0, 0), seed, step)
    want = _expected_coef(arr, table, (0, 0, 0), BATCH, seed, step)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert len(np.unique(got[4][:, 0])) > 50
    # the same batches as the plain gather on the same seed
    from test_gpu_tabulated import _gather
    plain = _gather(lib, L, gpu_device, data, BATCH, (0, 0, 0), seed, step)
    for g, w in zip(got[:4], plain):
        assert np.array_equal(g, w)
    # two shards with offsets concatenate to the single call
    cut = (70, 20, 9)
    a = _gather_coef(lib, L, gpu_device, data, tab_dev, cut, (0, 0, 0), seed, step)
    rest = tuple(b - c for b, c in zip(BATCH, cut))
    b = _gather_coef(lib, L, gpu_device, data, tab_dev, rest, cut, seed, step)
    for k in (0, 1, 4):
        assert np.array_equal(np.concatenate([a[k], b[k]]), got[k])
    n_ic = BATCH[1]
    assert np.array_equal(np.concatenate([a[3][:cut[1]], b[3][:rest[1]], a[3][cut[1]:], b[3][rest[1]:]]), got[3])
    assert np.array_equal(np.concatenate([a[2][:cut[1]], b[2][:rest[1]]]), got[2][:n_ic])
    # a global index past 2^32 reaches the high counter word
    offs = ((1 << 32) + 3, 0, 0)
    far = _gather_coef(lib, L, gpu_device, data, tab_dev, (5, 0, 0), offs, seed, step)
    want = _expected_coef(arr, table, offs, (5, 0, 0), seed, step)
    assert np.array_equal(far[1], want[1]) and np.array_equal(far[4], want[4])
    assert DS_N == (1000, 7, 1) and BATCH == (130, 33, 31)


def test_sample_phase_of_the_merged_step_leaves_the_gathered_batch(gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    ans, n, Lq, enc, B_res, n_ic, n_bc = CR.CASES["reg_cascade4"]
    flat, *_ = CR.case_inputs("reg_cascade4")
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    assert (_merged_probe(eng, B_res, n_ic, n_bc) == 0) == (os.environ.get("QC_NO_MERGE") != "1")
    arr, _ = _dataset(gpu_device, (300, 40, 50), seed=8)
    arr = [(X, T.u_star(X)) for X, _ in arr]
    ten = [(torch.from_numpy(X).to(gpu_device), torch.from_numpy(y).to(gpu_device)) for X, y in arr]
    table = CR.coef_star(arr[0][0])
    tab_dev = torch.from_numpy(table).to(gpu_device)
    fs = _coef_step(eng, B_res, n_ic, n_bc)
    fs.set_dataset(ten, tab_dev)
    fs.set_sampler(0xABCDEF, 11, 5, 7)
    fs.run(L.QC_PHASE_SAMPLE | L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    step = fs.desc.sample_step
    assert step == 1
    counts, offs = (B_res, n_ic, n_bc), (11, 5, 7)
    alone = _gather_coef(lib, L, gpu_device, _step_data(L, ten), tab_dev, counts, offs, 0xABCDEF, step)
    left = (fs.X_res[:B_res], fs.target_res[:B_res], fs.X_val[:n_ic + n_bc], fs.target_val[:n_ic + n_bc], fs.coef_res[:, :B_res].t())
    for got, want in zip(left, alone):
        assert np.array_equal(got.cpu().numpy(), want)
    want = _expected_coef(arr, table, offs, counts, 0xABCDEF, step)
    assert np.array_equal(alone[0], want[0]) and np.array_equal(alone[3], want[3]) and np.array_equal(alone[4], want[4])
    # and the gradient of that call is the gradient on the gathered batch, loaded explicitly
    got = fs.flat_grad.cpu().numpy().astype(np.float64)
    again = coef_grads(eng, want[2][:n_ic], want[2][n_ic:], want[0], want[3][:n_ic], want[3][n_ic:], want[1], want[4])
    assert np.array_equal(got, again)


# ---- 6. refusals
def test_refusals_name_one_fault_each(gpu_device):
    """A descriptor that runs (rc 0), then the same descriptor with ONE fault: -1, and nothing written."""
    L = pkg("hip.lib")
    ans, n, Lq, enc, B_res, n_ic, n_bc = CR.CASES["reg_cascade4"]
    flat, *batch = CR.case_inputs("reg_cascade4")
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat)
    arr, ten = _dataset(gpu_device, (300, 40, 50), seed=8)
    tab_dev = torch.from_numpy(CR.coef_star(arr[0][0])).to(gpu_device)
    fs = _coef_step(eng, B_res, n_ic, n_bc)
    _load_coef(fs, *batch, CR.case_table("reg_cascade4"))
    fs.set_dataset(ten, tab_dev)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    both = L.QC_PHASE_GRADS | L.QC_PHASE_SAMPLE
    ref = lambda s: None if s is None else C.byref(s)
    call = lambda data, coef, phases: eng.lib.qc_fused_pinn_coef_step(C.byref(fs.desc), ref(data), ref(coef), phases, st)
    assert call(fs.data, fs.coef, L.QC_PHASE_GRADS) == 0 and call(fs.data, fs.coef, both) == 0
    torch.cuda.synchronize()
    fs.flat_grad.fill_(NAN)
    fs.X_res.fill_(NAN)
    fs.coef_res.fill_(NAN)

    def broken(src, **kw):
        t = type(src).from_buffer_copy(src)
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    assert call(fs.data, None, L.QC_PHASE_GRADS) == -1 and call(None, fs.coef, L.QC_PHASE_GRADS) == -1
    assert call(fs.data, broken(fs.coef, coef_res_dev=None), L.QC_PHASE_GRADS) == -1
    assert call(fs.data, broken(fs.coef, ds_coef=None), both) == -1
    # whatever the data step refuses
    assert call(broken(fs.data, target_res_dev=None), fs.coef, L.QC_PHASE_GRADS) == -1
    assert call(broken(fs.data, target_val_dev=None), fs.coef, L.QC_PHASE_GRADS) == -1
    for kw in (dict(ds_n_res=0), dict(ds_X_ic=None), dict(ds_u_bc=None), dict(ds_n_bc=2 ** 31)):
        assert call(broken(fs.data, **kw), fs.coef, both) == -1, kw
    for pb in (0, 1, 2, 4):
        fs.desc.pde.problem = pb
        assert call(fs.data, fs.coef, L.QC_PHASE_GRADS) == -1
    fs.desc.pde.problem = L.QC_PROBLEM_TABULATED
    torch.cuda.synchronize()
    assert torch.isnan(fs.flat_grad).all() and torch.isnan(fs.X_res).all() and torch.isnan(fs.coef_res).all()
    # ds_coef may be absent without QC_PHASE_SAMPLE
    _load_coef(fs, *batch, CR.case_table("reg_cascade4"))
    assert call(fs.data, broken(fs.coef, ds_coef=None), L.QC_PHASE_GRADS) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(fs.flat_grad).all()


# ---- 7. training on a coefficient dataset
@pytest.mark.parametrize("case", list(CT.TRAIN_CASES))
def test_training_on_a_coefficient_dataset_matches_the_fp64_replay(case, gpu_device, tmp_path):
    trainer = pkg("trainer.diffusion_train")
    TP = pkg("data.tabulated").TabulatedProblem
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    ans, n = CT.TRAIN_CASES[case]

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(TT.base_args(ans, n), TmpLog(), device=gpu_device)
    Xr, rr, Xi, ui, Xb, ub, coef = (torch.from_numpy(a) for a in CT.dataset_arrays())
    ds = TP(Xr, rr, Xi, ui, Xb, ub, coef_res=coef)
    torch.manual_seed(TT.TRAINER_SEED_AT)
    tr = trainer.FusedTrainer(model, CT.BATCH, capacity=CT.STEPS, dataset=ds)
    assert tr.fs.desc.sample_seed == TT.trainer_seed() and tr.fs.tabulated and tr.fs.coef_mode
    assert not model._engine_for(gpu_device).coef_mode          # the engine is left as it was found
    batches = []
    for _ in range(CT.STEPS):
        tr.sample()
        tr.step()
        fs = tr.fs
        Xv, tv = fs.X_val.cpu().numpy(), fs.target_val.cpu().numpy()
        batches.append((Xv[:CT.N_IC], Xv[CT.N_IC:CT.N_IC + CT.N_BC], fs.X_res.cpu().numpy()[:CT.BATCH], tv[:CT.N_IC],
                        tv[CT.N_IC:CT.N_IC + CT.N_BC], fs.target_res.cpu().numpy()[:CT.BATCH],
                        np.ascontiguousarray(fs.coef_res.cpu().numpy()[:, :CT.BATCH].T)))
    for got, want in zip(batches, CT.expected_batches()):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    got = np.array(tr.opt.loss_history(CT.STEPS))
    want = CT.training_reference(case, batches)["loss"]
    print(case, got, want)
    assert got.shape == want.shape == (CT.STEPS,)
    assert np.abs(got - want).max() < 1e-4 * max(1.0, np.abs(want).max()), (got, want)
    assert len(set(np.round(want, 6))) == CT.STEPS          # six different batches, six different losses
