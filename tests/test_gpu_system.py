"""The system step on the GPU, through the C ABI and the trainer: qc_post_system alone behind poisoned buffers,
qc_fused_pinn_system_step (QC_PHASE_GRADS) against the float64 reference (tests/system_reference.py) in every circuit
family and encoding, the reference's own Navier-Stokes operator (tests/golden/other_operators.npz), the K = 1 system against
the committed record of the tabulated step, the bits of the gather, and SystemTrainer against a float64 replay.

Tolerances are those of tests/test_gpu_tabulated.py: the gradient block by block (pre network, post network, theta) at
2e-4 x max(1, max |ref block|), the loss parts at 1e-4, points at 5e-5 and tile rows at 2e-4.  The negative controls
(tests/test_system_cpu.py shows each differs from the true reference by more than ten times the tolerance) must fail."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mlp_reference as R
import system_reference as S
import system_training as ST
import tabulated_reference as T
from conftest import GOLDEN, pkg
from test_gpu_fullsize import Log, base_args

pytestmark = pytest.mark.gpu

TOL_G, TOL_L = 2e-4, 1e-4
POINT_TOL, ROW_TOL = 5e-5, 2e-4
THETA_MIN = 20 * TOL_G


def _circuit(dev, ans, n, Lq, enc, hidden, K):
    """A K-output DVPDESolver (for its gate program and fixed unitaries) and its device circuit."""
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=Lq, q_ansatz=ans, encoding=enc, classic_network=[3, hidden, K]),
                   Log(), device=dev)
    return model, model.quantum_layer._circuit_for(dev)


def _step(dev, circ, hidden, flat, K, terms, w_eq, w_out, B_res, n_ic, n_bc, loss_weights=S.LOSS_WEIGHTS, res_targets=True):
    """A SystemStep on a copy of ``flat`` with poisoned workspace and targets."""
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    fl = torch.from_numpy(np.asarray(flat, dtype=np.float32)).to(dev)
    opt = engine.OptimState(fl.numel(), 0.005, dev, loss_weights=loss_weights)
    fs = engine.SystemStep(circ, hidden, fl, L.system_record(K, len(w_eq), terms, w_eq, w_out), B_res, n_ic, n_bc, opt,
                           loss_weights=loss_weights, res_targets=res_targets)
    fs.refresh_gates()
    if fs.step_ws.numel() >= 4:
        fs.step_ws[: 4 * (fs.step_ws.numel() // 4)].view(torch.float32).fill_(float("nan"))
    for t in (fs.target_res, fs.target_val, fs.part, fs.flat_grad):
        if t is not None:
            t.fill_(float("nan"))
    return fs


def _load(fs, X_ic, X_bc, X_res, U_ic, U_bc, R_res):
    dev = fs.device
    n_ic, n_bc, B_res = len(X_ic), len(X_bc), len(X_res)
    to = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(dev)
    if B_res:
        fs.X_res[:B_res] = to(X_res)
        if R_res is not None:
            fs.target_res[:, :B_res] = to(R_res).t()
    if n_ic:
        fs.X_val[:n_ic], fs.target_val[:, :n_ic] = to(X_ic), to(U_ic).t()
    if n_bc:
        fs.X_val[n_ic:n_ic + n_bc], fs.target_val[:, n_ic:n_ic + n_bc] = to(X_bc), to(U_bc).t()


def _grads(fs):
    L = pkg("hip.lib")
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    return fs.flat_grad.cpu().numpy().astype(np.float64)


# ---- 1. qc_post_system alone
ROW0, STRIDE_PAD, N_THETA = 2, 7, 3


def _two_factor_terms():
    """K = 4 outputs, 4 equations: every output and every equation used, one term with two multipliers (u0 u1^2)."""
    return [(0, 0, 1, -1, -1, 1.0), (0, 0, 0, 1, 1, -0.8), (0, 0, 4, -1, -1, -0.05), (1, 1, 1, -1, -1, 1.0), (1, 1, 2, 0, -1, 0.6),
            (1, 1, 5, -1, -1, -0.03), (2, 2, 3, 3, -1, 0.9), (2, 2, 0, -1, -1, 0.4), (3, 3, 1, -1, -1, 0.7), (3, 3, 2, 2, 1, -0.5),
            (3, 0, 3, -1, -1, 0.3)]


def _linear_terms():
    return [(0, 0, 0, -1, -1, T.C_U), (0, 0, 1, -1, -1, T.COEFFS[0]), (0, 0, 2, -1, -1, T.COEFFS[1]), (0, 0, 3, -1, -1, T.COEFFS[2]),
            (0, 0, 4, -1, -1, -T.COEFFS[3]), (0, 0, 5, -1, -1, -T.COEFFS[4])]


POST_CASES = {   # id -> (H, n, K, terms, w_eq, w_out, B, nch)
    "res_H50_n4_K3": (50, 4, 3, None, S.W_EQ, S.W_OUT, 65, 6),
    "res_H5_n3_K4": (5, 3, 4, "two", (1.0, 0.5, 2.0, 0.7), (1.0, 0.5, 0.0, 0.3), 65, 6),      # the last wave owns no hidden unit
    "res_H129_n3_K1": (129, 3, 1, "lin", (1.0,), (1.0,), 1, 6),
    "val_H50_n4_K3": (50, 4, 3, None, S.W_EQ, S.W_OUT, 65, 1),                                  # IC and BC in the first tile
}


@pytest.mark.parametrize("case", list(POST_CASES))
def test_post_system_alone(case, gpu_device):
    """Behind NaN-filled outputs and padding: nothing but qbar, the tile rows' W3 / b3 / W4 / b4 columns and the three loss
    columns may be written."""
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    Hh, n, K, tsel, w_eq, w_out, B, nch = POST_CASES[case]
    terms = {None: S.ns_terms(), "two": _two_factor_terms(), "lin": _linear_terms()}[tsel]
    n_eq, dev = len(w_eq), gpu_device
    g = np.random.default_rng(Hh + nch + K)
    lay, NP = S.layout(Hh, n, N_THETA, K)
    flat = np.full(NP, np.nan, np.float32)
    for k in ("W3", "b3", "W4", "b4"):
        o, s = lay[k]
        flat[o:o + int(np.prod(s))] = g.uniform(-1, 1, int(np.prod(s))) / np.sqrt({"W3": n, "b3": n}.get(k, Hh))
    q = np.concatenate([g.uniform(-1, 1, (1, n, B)), g.standard_normal((5, n, B))]).astype(np.float32)[:nch]
    width = n_eq if nch == 6 else K
    target = g.standard_normal((width, B)).astype(np.float32)
    n_seg_a = 30 if nch == 1 else 0
    pde = dict(D=0.0, vx=0.0, vy=0.0, c_t=0.0, c_x=0.0, c_y=0.0, d_xx=0.0, d_yy=0.0, w_res=4.0 / B, inv_n_res=1.0 / B,
               w_val_a=0.3, w_val_b=0.7, inv_n_a=0.11, inv_n_b=0.13, problem=L.QC_PROBLEM_TABULATED, n_seg_a=n_seg_a)
    qpde = L.QcPde(**pde)
    sysrec = L.system_record(K, n_eq, terms, w_eq, w_out)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    tiles = (B + 63) // 64
    qbar = nan(nch * n * B + 64)
    part = nan(ROW0 + tiles + 2, NP + 3 + STRIDE_PAD)
    prm, qd, tg = (torch.from_numpy(a).to(dev) for a in (flat, q, target))
    L.check(lib.qc_post_system(prm.data_ptr(), Hh, n, N_THETA, C.byref(sysrec), C.byref(qpde), qd.data_ptr(), tg.data_ptr(),
                               qbar.data_ptr(), part.data_ptr(), part.shape[1], ROW0, B, nch, st), "qc_post_system")
    torch.cuda.synchronize(dev)
    names = ("W3", "b3", "W4", "b4")
    cols = np.concatenate([np.arange(lay[k][0], lay[k][0] + int(np.prod(lay[k][1]))) for k in names] + [[NP, NP + 1, NP + 2]])
    p = part.cpu().numpy()
    mask = np.zeros(p.shape, bool)
    mask[ROW0:ROW0 + tiles, cols] = True
    assert np.isnan(p[~mask]).all() and np.isfinite(p[mask]).all()
    a = qbar.cpu().numpy()
    assert np.isnan(a[nch * n * B:]).all() and np.isfinite(a[:nch * n * B]).all()

    def errors(terms_ref, tgt):
        P = S.unpack(np.nan_to_num(flat.astype(np.float64)), Hh, n, N_THETA, K)
        qt = torch.from_numpy(q).double().requires_grad_(True)
        u = R.post_jets(P, qt, w4=P["W4"], b4=P["b4"])                       # (K, nch, B)
        tt = torch.from_numpy(tgt).double()
        if nch == 6:
            e = S.eval_terms(u, terms_ref, n_eq) - tt                       # (n_eq, B)
            w = torch.tensor(w_eq, dtype=R.F64)[:, None] * pde["w_res"]
            e2 = (torch.tensor(w_eq, dtype=R.F64)[:, None] * e * e).sum(0)
            losses = np.stack([[pde["inv_n_res"] * e2[k:k + 64].sum().item(), 0.0, 0.0] for k in range(0, B, 64)])
        else:
            e = u[:, 0] - tt                                                # (K, B)
            seg_a = torch.arange(B) < n_seg_a
            wv = torch.where(seg_a, torch.tensor(pde["w_val_a"], dtype=R.F64), torch.tensor(pde["w_val_b"], dtype=R.F64))
            w = torch.tensor(w_out, dtype=R.F64)[:, None] * wv[None]
            e2 = (torch.tensor(w_out, dtype=R.F64)[:, None] * e * e).sum(0)
            losses = np.stack([[0.0, pde["inv_n_b"] * e2[k:k + 64][~seg_a[k:k + 64]].sum().item(),
                                pde["inv_n_a"] * e2[k:k + 64][seg_a[k:k + 64]].sum().item()] for k in range(0, B, 64)])
        obj = (0.5 * w * e * e).sum(0)
        qb = torch.autograd.grad(obj.sum(), qt, retain_graph=True)[0].numpy()
        rows = np.stack([S.flatten(dict(zip(names, gr)), Hh, n, N_THETA, K) for gr in R.tile_grads(obj, [P[k] for k in names], B)])
        rel = lambda got, want, tol: np.abs(got - want).max() / (tol * max(1.0, np.abs(want).max()))
        return {"qbar": rel(a[:nch * n * B].reshape(nch, n, B), qb, POINT_TOL),
                "rows": rel(p[ROW0:ROW0 + tiles][:, cols[:-3]], rows[:, cols[:-3]], ROW_TOL),
                "loss": rel(p[ROW0:ROW0 + tiles][:, cols[-3:]], losses, ROW_TOL)}
    err = errors(terms, target)
    print(case, {k: float(v) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    if B > 1:
        assert max(errors(terms, np.roll(target, 1, axis=1)).values()) > 1.0      # the target of ANOTHER point is told apart
    if nch == 6:                                                                # and so is a term without its multiplier
        t = next(i for i, tm in enumerate(terms) if tm[3] >= 0) if tsel != "lin" else 0
        bad = list(terms)
        bad[t] = bad[t][:3] + (-1, -1) + (bad[t][5] * (1.0 if tsel != "lin" else 0.0),)
        assert max(errors(bad, target).values()) > 1.0


# ---- 2. the step against the float64 reference in every family and encoding
@pytest.mark.parametrize("case", list(S.CASES))
def test_system_step_matches_fp64(case, gpu_device):
    ans, n, Lq, enc, B_res, n_ic, n_bc, K = S.CASES[case]
    flat, *batch = S.case_inputs(case)
    ref = S.case_reference(case)
    model, circ = _circuit(gpu_device, ans, n, Lq, enc, S.H, K)
    terms, w_eq, w_out = S.system_of(K)
    fs = _step(gpu_device, circ, S.H, flat, K, terms, w_eq, w_out, B_res, n_ic, n_bc)
    _load(fs, *batch)
    got = _grads(fs)
    n_theta = circ.n_params
    assert np.isfinite(got).all() and got.size == S.layout(S.H, n, n_theta, K)[1] + 3
    err = S.errors(got, ref["grad"], ref["parts"], S.H, n, n_theta, K, TOL_G, TOL_L)
    print(case, {k: round(float(v), 4) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    for name, s in S.blocks(S.H, n, n_theta, K).items():
        assert np.abs(ref["grad"][s]).max() >= THETA_MIN, name
    if K == 3:      # the pressure is not prescribed and enters through its derivatives only
        assert got[S.layout(S.H, n, n_theta, K)[0]["b4"][0] + 2] == 0.0
    if case in S.CONTROL_CASES:
        for v in S.CONTROLS:
            bad = S.case_reference(case, v)
            berr = S.errors(got, bad["grad"], bad["parts"], S.H, n, n_theta, K, TOL_G, TOL_L)
            print(case, v, {k: round(float(x), 1) for k, x in berr.items()})
            assert max(berr.values()) > 1.0, (v, berr)


# ---- 3. pinned by the reference's own operator
def test_navier_stokes_fixture_of_the_reference_operator(gpu_device, tmp_path):
    """tests/golden/other_operators.npz navier_stokes__*: outputs, loss = sum_i (i + 1) mean(res_i^2) and its gradient from
    the reference's navier_stokes_2D_operator on the CPU oracle (B = 24, [3, 16, 3], cascade n = 4).  The step with
    navier_stokes_2D_terms(), zero targets, no value points, loss weights (1, 0, 0) and w_eq = 512 (1, 2, 3): the power of
    two is exact in fp32 and lifts the gradient (max 3.1e-3 unscaled, where a check against max(1, .) is vacuous) to block
    maxima 0.89 / 1.59 / 0.50 and the loss to 0.227."""
    from test_gpu_operators_fused import _ref_grad, _solver_from_fixture
    z = np.load(os.path.join(GOLDEN, "other_operators.npz"))
    model, _ = _solver_from_fixture(z, "navier_stokes", gpu_device, tmp_path, network=(3, 16, 3))
    ref = _ref_grad(z, "navier_stokes", model, n_in=3, n_out=3)
    want = 512.0 * np.concatenate([ref[name].reshape(-1) for name, _ in model.named_parameters()]).astype(np.float64)
    flat = np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in model.parameters()])
    circ = model.quantum_layer._circuit_for(gpu_device)
    X = z["navier_stokes__X"]
    B, K, Hh, n = X.shape[0], 3, 16, 4
    fs = _step(gpu_device, circ, Hh, flat, K, pkg("nn.pde").navier_stokes_2D_terms(), (512.0, 1024.0, 1536.0), (1.0, 1.0, 1.0),
               B, 0, 0, loss_weights=(1.0, 0.0, 0.0), res_targets=False)
    assert fs.sys.target_res_dev is None
    _load(fs, X[:0], X[:0], X, None, None, None)
    got = _grads(fs)
    parts = np.array([512.0 * float(z["navier_stokes__loss"]), 0.0, 0.0])
    err = S.errors(got, want, parts, Hh, n, circ.n_params, K, TOL_G, TOL_L)
    print({k: round(float(v), 4) for k, v in err.items()}, parts[0])
    assert max(err.values()) < 1.0, err
    blocks = {k: np.abs(want[s]).max() for k, s in S.blocks(Hh, n, circ.n_params, K).items()}
    assert min(blocks.values()) > 0.4 and parts[0] > 0.2, blocks          # TOL_G and TOL_L bite


# ---- 4. K = 1: the system step with six linear terms is the tabulated step
def test_single_output_system_meets_the_tabulated_record(gpu_device):
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = T.CASES[case]
    flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res = T.case_inputs(case)
    ref = T.case_reference(case)
    model, circ = _circuit(gpu_device, ans, n, Lq, enc, T.H, 1)
    fs = _step(gpu_device, circ, T.H, flat, 1, _linear_terms(), (1.0,), (1.0,), B_res, n_ic, n_bc)
    _load(fs, X_ic, X_bc, X_res, u_ic[:, None], u_bc[:, None], r_res[:, None])
    got = _grads(fs)
    err = S.errors(got, ref["grad"], ref["parts"], T.H, n, circ.n_params, 1, TOL_G, TOL_L)
    print({k: round(float(v), 4) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    bad = T.case_reference(case, "cu0")
    assert max(S.errors(got, bad["grad"], bad["parts"], T.H, n, circ.n_params, 1, TOL_G, TOL_L).values()) > 1.0


# ---- 5. the gather's bits
DS_N, BATCH = (1000, 7, 1), (130, 33, 31)


def test_gather_bits(gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    dev, K, n_eq = gpu_device, 3, 2
    st = torch.cuda.current_stream(dev).cuda_stream
    g = np.random.default_rng(5)
    arr = [(g.random((m, 3)).astype(np.float32), g.standard_normal((m, w)).astype(np.float32)) for m, w in zip(DS_N, (n_eq, K, K))]
    ten = [(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)) for X, Y in arr]
    sysrec = L.system_record(K, n_eq, [(0, 0, 0, -1, -1, 1.0)], (1.0, 1.0), (1.0, 1.0, 1.0))
    for name, (X, Y) in zip(("res", "ic", "bc"), ten):
        setattr(sysrec, "ds_X_" + name, X.data_ptr())
        setattr(sysrec, {"res": "ds_r", "ic": "ds_u_ic", "bc": "ds_u_bc"}[name], Y.data_ptr())
        setattr(sysrec, "ds_n_" + name, X.shape[0])
    seed, step = 0xC0FFEE1234567, (1 << 33) + 5
    n_res, n_ic, n_bc = BATCH
    n_val = n_ic + n_bc
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)

    def gather(offs, with_r=True):
        Xr, tr, Xv, tv = nan(n_res + 3, 3), nan(n_eq * n_res + 3), nan(n_val + 3, 3), nan(K * n_val + 3)
        keep = sysrec.ds_r
        if not with_r:
            sysrec.ds_r = None
        L.check(lib.qc_sample_dataset_system(Xr.data_ptr(), tr.data_ptr(), n_res, offs[0], Xv.data_ptr(), tv.data_ptr(), n_ic,
                                             offs[1], n_bc, offs[2], C.byref(sysrec), seed, step, st), "qc_sample_dataset_system")
        torch.cuda.synchronize(dev)
        sysrec.ds_r = keep
        out = [t.cpu().numpy() for t in (Xr, tr, Xv, tv)]
        for a, m in zip(out, (n_res, n_eq * n_res, n_val, K * n_val)):
            assert np.isnan(a[m:]).all(), "the gather wrote past its batch"
        return out[0][:n_res], out[1][:n_eq * n_res].reshape(n_eq, n_res), out[2][:n_val], out[3][:K * n_val].reshape(K, n_val)

    for offs in ((0, 0, 0), ((1 << 32) + 3, 11, 5)):
        idx = [T.dataset_indices(seg, off, cnt, m, seed, step) for seg, (off, cnt, m) in enumerate(zip(offs, BATCH, DS_N))]
        Xr, tr, Xv, tv = gather(offs)
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
        assert np.array_equal(bits(Xr), bits(arr[0][0][idx[0]])) and np.array_equal(bits(tr), bits(arr[0][1][idx[0]].T))
        assert np.array_equal(bits(Xv), bits(np.concatenate([arr[1][0][idx[1]], arr[2][0][idx[2]]])))
        assert np.array_equal(bits(tv), bits(np.concatenate([arr[1][1][idx[1]], arr[2][1][idx[2]]]).T))
        # the points are those of qc_sample_dataset on the same seed, step and offsets
        one = [torch.from_numpy(np.ascontiguousarray(Y[:, 0])).to(dev) for _, Y in arr]
        data = L.QcStepData(None, None, 0.0, ten[0][0].data_ptr(), one[0].data_ptr(), DS_N[0], ten[1][0].data_ptr(),
                            one[1].data_ptr(), DS_N[1], ten[2][0].data_ptr(), one[2].data_ptr(), DS_N[2])
        Xr1, tr1, Xv1, tv1 = nan(n_res, 3), nan(n_res), nan(n_val, 3), nan(n_val)
        L.check(lib.qc_sample_dataset(Xr1.data_ptr(), tr1.data_ptr(), n_res, offs[0], Xv1.data_ptr(), tv1.data_ptr(), n_ic, offs[1],
                                      n_bc, offs[2], C.byref(data), seed, step, st), "qc_sample_dataset")
        torch.cuda.synchronize(dev)
        assert np.array_equal(bits(Xr1.cpu().numpy()), bits(Xr)) and np.array_equal(bits(Xv1.cpu().numpy()), bits(Xv))
        assert np.array_equal(bits(tr1.cpu().numpy()), bits(tr[0])) and np.array_equal(bits(tv1.cpu().numpy()), bits(tv[0]))
    assert len(np.unique(tr[0])) > 100
    # without a residual table the points are gathered and the residual targets are left alone
    Xr, tr, Xv, tv = gather((0, 0, 0), with_r=False)
    assert np.isnan(tr).all() and np.isfinite(Xr).all() and np.isfinite(tv).all()


# ---- 6. refusals on a descriptor that runs but for the one fault named
def test_refusals_name_one_fault_each(gpu_device):
    L = pkg("hip.lib")
    case = "no_val"
    ans, n, Lq, enc, B_res, n_ic, n_bc, K = S.CASES[case]
    flat, *batch = S.case_inputs(case)
    model, circ = _circuit(gpu_device, ans, n, Lq, enc, S.H, K)
    terms, w_eq, w_out = S.system_of(K)
    fs = _step(gpu_device, circ, S.H, flat, K, terms, w_eq, w_out, B_res, n_ic, n_bc)
    _load(fs, *batch)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    call = lambda phases=L.QC_PHASE_GRADS: fs.lib.qc_fused_pinn_system_step(C.byref(fs.desc), C.byref(fs.sys), phases, st)
    assert call() == 0

    def refused(obj, field, bad, phases=L.QC_PHASE_GRADS):
        keep = getattr(obj, field)
        setattr(obj, field, bad)
        rc = call(phases)
        setattr(obj, field, keep)
        return rc == -1
    assert refused(fs.sys, "K", 5) and refused(fs.sys, "n_eq", 0) and refused(fs.sys, "n_terms", 33)
    assert refused(fs.desc, "part_stride", fs.NP + 2)
    assert refused(fs.sys, "ds_n_res", 0, L.QC_PHASE_GRADS | L.QC_PHASE_SAMPLE)          # no dataset behind the residual batch
    keep = fs.sys.terms[3].mul0
    fs.sys.terms[3].mul0 = 3
    assert call() == -1
    fs.sys.terms[3].mul0 = keep
    fs.sys.w_eq[1] = float("nan")
    assert call() == -1
    fs.sys.w_eq[1] = w_eq[1]
    assert call() == 0
    torch.cuda.synchronize()


# ---- 7. training against a float64 replay
def test_system_trainer_matches_fp64_replay(gpu_device, tmp_path):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    TS = pkg("data.tabulated").TabulatedSystem
    Trainer = pkg("trainer.system_train").SystemTrainer
    terms, w_eq, w_out = S.system_of(ST.K)
    Xr, Rr, Xi, Ui, Xb, Ub = (torch.from_numpy(a) for a in ST.dataset_arrays())
    torch.manual_seed(1)
    model = Solver(ST.base_args(), Log(), device=gpu_device)
    ds = TS((Xr, Rr), (Xi, Ui), (Xb, Ub), terms, eq_weights=w_eq, out_weights=w_out)
    torch.manual_seed(ST.TT.TRAINER_SEED_AT)
    tr = Trainer(model, ST.BATCH, dataset=ds, capacity=ST.STEPS)
    assert (tr.B_res, tr.n_ic, tr.n_bc) == (ST.BATCH, ST.N_IC, ST.N_BC) and model._packed_ok()
    lay = pkg("hip.engine").param_layout(50, ST.N_QUBITS, tr.circuit.n_params, ST.K)
    assert tr.NP == lay["__total__"][0] and model.postprocessor[2].weight.data_ptr() == tr.flat.data_ptr() + 4 * lay["postprocessor.2.weight"][0]
    want = ST.expected_batches()
    for k in range(ST.STEPS):
        tr.sample()
        tr.step()
        if k in (0, ST.STEPS - 1):         # the device gathered the rows the record was computed for
            torch.cuda.synchronize()
            X_ic, X_bc, X_res, U_ic, U_bc, R_res = want[k]
            assert np.array_equal(tr.fs.X_res.cpu().numpy(), X_res) and np.array_equal(tr.fs.target_res.cpu().numpy(), R_res.T)
            assert np.array_equal(tr.fs.X_val.cpu().numpy(), np.concatenate([X_ic, X_bc]))
            assert np.array_equal(tr.fs.target_val.cpu().numpy(), np.concatenate([U_ic, U_bc]).T)
    got = np.array(tr.loss_history())
    ref = ST.training_reference()["loss"]
    print(got, ref)
    assert got.shape == ref.shape == (ST.STEPS,)
    assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
    assert ref[0] - ref[-1] > 10 * 1e-4          # the run moves: a trainer that did not update would not pass
    # the parameters the torch modules see are the trained ones, and jets_all keeps working on them
    J = model.jets_all(torch.from_numpy(want[0][2]).to(gpu_device))
    assert J.shape == (ST.BATCH, ST.K, 6) and torch.isfinite(J).all()
    # sync_to_torch, then save_state round-trips
    tr.sync_to_torch()
    path = os.path.join(str(tmp_path), "model.pth")
    model.save_state(path)
    state = Solver.load_state(path)
    assert torch.equal(state["postprocessor"]["2.weight"].cpu(), model.postprocessor[2].weight.detach().cpu())
    assert state["postprocessor"]["2.weight"].shape == (ST.K, 50)
    st0 = state["optimizer"]["state"]
    assert len(st0) == len(list(model.parameters())) and float(st0[0]["step"]) == ST.STEPS
    off = lay["postprocessor.2.weight"][0]
    assert torch.equal(st0[6]["exp_avg"].cpu().reshape(-1), tr.opt.m[off:off + ST.K * 50].cpu())
