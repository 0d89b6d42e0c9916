"""The optimiser launch's staged tail (csrc/qc_common.h: qc_gate_stage_*; k_adam_fast and k_lbfgs) and the branch-free
fold loads of k_adam_fast<FOLD>.

After an update the trig buffer - the per-gate entries and every phase table of the diagonal runs - must hold, bit for
bit, what ``refresh_gates()`` (k_prep_trig, which keeps the unstaged qc_fill_diag_tables) builds from the updated theta
on a fresh engine: the staged form reads the gate records, the run list and the run ranges from copies made at kernel
entry, so a stale or misplaced copy shows as a wrong table.  theta must have moved by more than 1e-2 (lr 0.05), so
that a table left from before the update cannot pass.

The programs are chosen for where the staging can go wrong: no fixed unitaries and one run of two gates (cascade n = 2),
the flagship program (cascade n = 4), several runs through the device list (layered n = 8, two layers), one run of 64
gates through the device list - more gates than one wave, more (run, amplitude) pairs than one pass of the block - (cross_mesh
n = 8), no run at all (farhi n = 4), tables skipped with more than 64 gates (cross_mesh n = 10), three entries behind theta
(the balanced step) and an update without a circuit.

Fold loads: cascade n = 2 at H = 13 / 100 / 200, i.e. one, two and three live 1024-column blocks of k_adam_fast, at 2, 31,
32 and 33 rows (both sides of RS = 32).  The hidden widths are the issue's; the number of parameter layers (2, 4 and 8: six
angles each) is what puts NP + 3 into the three ranges asserted below - with two, three or four layers H = 100 and H = 200
would stay one block short.  The five stages run one by one (qc_fused_step_stage) on a NaN-filled ``part``; the rows are
copied out and summed on the host in float32 in the kernels' order (k_fold_rows: per wave two chains over every second of
its rows, a0 + a1, the eight waves in order; then the surviving rows left to right), and the fold + update launch must
give exactly those sums: the loss columns always (the clip never scales them), the gradient columns as well while the
clip is inactive (the loss weights are scaled by 2^-10 so that the norm stays below max_norm = 1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import balanced_reference as BR
import lbfgs_driver as D
from conftest import pkg
from step_reference import step_inputs
from test_gpu_balanced import _balanced_step, _load
from test_gpu_fullsize import Log, base_args
from test_gpu_tabulated import _model as _tab_model

pytestmark = pytest.mark.gpu

LR = 0.05
B_RES, N_IC, N_BC = 70, 30, 20
# name -> (ansatz, n, layers, phase tables expected: a count, or "some" (at least one), or "several" (at least two))
PROGRAMS = {
    "cascade2": ("cascade", 2, 1, 1),
    "cascade4": ("cascade", 4, 1, 1),
    "layered8_L2": ("layered", 8, 2, "several"),
    "cross_mesh8": ("cross_mesh", 8, 1, "some"),
    "farhi4": ("farhi", 4, 1, 0),
    "cross_mesh10": ("cross_mesh", 10, 1, 0),
}


def _model(device, ans, n, L, H, flat):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, classic_network=[3, H, 1]), Log(), device=device)
    eng = model._engine_for(device)
    with torch.no_grad():
        eng.flat.copy_(torch.from_numpy(np.asarray(flat, dtype=np.float32)))
    return model, eng


def _table_rows(circ):
    """Phase tables behind the per-gate entries of a circuit's trig buffer (qc_trig_bytes)."""
    words = circ.trig.numel()
    assert words % 4 == 0 and (words // 4 - circ.program.n_gates) % (1 << circ.n) == 0
    return (words // 4 - circ.program.n_gates) >> circ.n


def _assert_trig_of_fresh_engine(circ, fresh_circ, theta):
    fresh_circ.trig.fill_(float("nan"))
    fresh_circ.prepare(theta.clone())
    torch.cuda.synchronize()
    got, want = circ.trig.view(torch.int32), fresh_circ.trig.view(torch.int32)
    assert got.shape == want.shape
    bad = torch.nonzero(got != want).flatten()
    assert bad.numel() == 0, (bad[:8].tolist(), circ.program.n_gates, circ.trig.numel())
    assert torch.isfinite(circ.trig).all()


@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_trig_after_an_update_is_that_of_a_fresh_engine(name, split, gpu_device):
    """GRADS | UPDATE in one call (k_adam_fast<true>), or GRADS, then UPDATE (k_adam_fast<false>)."""
    Lb, engine = pkg("hip.lib"), pkg("hip.engine")
    ans, n, L, runs = PROGRAMS[name]
    H = 50
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_RES, N_IC, N_BC, salt=6)
    model, eng = _model(gpu_device, ans, n, L, H, flat)
    assert eng.NP + 3 <= 3072                                      # the k_adam_fast sizes
    have = _table_rows(eng.circuit)
    assert have >= {"some": 1, "several": 2}[runs] if isinstance(runs, str) else have == runs, (name, have)
    if name in ("cross_mesh8", "cross_mesh10"):
        assert eng.circuit.program.n_gates > 64
    eng.refresh_gates()
    fs = engine.FusedStep(eng, B_RES, N_IC, N_BC, engine.OptimState(eng.NP, LR, gpu_device))
    fs.X_res[:B_RES] = X_res.to(gpu_device)
    fs.X_val[:N_IC] = X_ic.to(gpu_device)
    fs.X_val[N_IC:N_IC + N_BC] = X_bc.to(gpu_device)
    if split:
        fs.run(Lb.QC_PHASE_GRADS)
        fs.run(Lb.QC_PHASE_UPDATE)
    else:
        fs.run(Lb.QC_PHASE_GRADS | Lb.QC_PHASE_UPDATE)
    torch.cuda.synchronize()
    assert fs.opt.read()["step"] == 1
    new = eng.flat.detach().cpu().numpy()
    th = slice(eng.theta_off, eng.theta_off + n_theta)
    assert np.isfinite(new).all() and np.abs(new[th] - flat[th]).max() > 1e-2      # the update moved theta
    model2, eng2 = _model(gpu_device, ans, n, L, H, new)
    _assert_trig_of_fresh_engine(eng.circuit, eng2.circuit, eng2.flat[th])


def test_trig_after_a_balanced_update(gpu_device):
    """Three entries behind theta (slot < n_theta): k_adam_fast<true, QcBal>."""
    Lb = pkg("hip.lib")
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = BR.CASES[case]
    flat, *batch = BR.case_inputs(case)
    model, eng = _tab_model(gpu_device, ans, n, Lq, enc, flat)
    fs = _balanced_step(eng, B_res, n_ic, n_bc, lr=LR)
    _load(fs, *batch)
    before = fs.flat.clone()
    assert fs.flat.numel() == fs.theta_off + fs.n_theta + BR.N_BAL and _table_rows(fs.circuit) == 1
    fs.run(Lb.QC_PHASE_GRADS | Lb.QC_PHASE_UPDATE)
    torch.cuda.synchronize()
    assert fs.opt.read()["step"] == 1
    th = slice(fs.theta_off, fs.theta_off + fs.n_theta)
    assert (fs.flat[th] - before[th]).abs().max().item() > 1e-2
    assert (fs.flat[th.stop:] != before[th.stop:]).all()           # the balancer's entries moved as well
    model2, eng2 = _tab_model(gpu_device, ans, n, Lq, enc, flat)
    _assert_trig_of_fresh_engine(fs.circuit, eng2.circuit, fs.flat[th])


@pytest.mark.parametrize("NP", [40, 2500], ids=["NP40", "NP2500"])
def test_an_update_without_a_circuit_is_the_update_with_one(NP, gpu_device):
    """prog = None stages nothing and skips both table parts: parameters, moments, gradient, record and history have
    the bits of the same update called with a circuit (cascade n = 4, theta the last entries)."""
    L, engine, circuits = pkg("hip.lib"), pkg("hip.engine"), pkg("circuits")
    lib, dev = L.load(), gpu_device
    prog = circuits.build_program("cascade", 4, 1, True)
    haar = circuits.haar_unitaries(3, 4)
    circ, fresh = engine.Circuit(prog, haar, dev), engine.Circuit(prog, haar, dev)
    theta_off = NP - prog.n_params
    g = np.random.default_rng(NP)
    vec = np.concatenate([3.0 * g.standard_normal(NP), [0.31, 0.052, 0.47]]).astype(np.float32)     # the clip is active
    p0 = g.standard_normal(NP).astype(np.float32)
    out = []
    for with_circuit in (False, True):
        opt = engine.OptimState(NP, LR, dev, hist_cap=2)
        opt.hist.fill_(float("nan"))
        flat_d, prm_d = torch.from_numpy(vec).to(dev), torch.from_numpy(p0).to(dev)
        handle, trig = (circ.handle, circ.trig.data_ptr()) if with_circuit else (None, None)
        L.check(lib.qc_adam_step(flat_d.data_ptr(), NP, prm_d.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(),
                                 opt.state.data_ptr(), C.byref(opt.hyper), opt.hist.data_ptr(), opt.hist_cap,
                                 handle, theta_off if with_circuit else 0, trig,
                                 torch.cuda.current_stream(dev).cuda_stream), "qc_adam_step")
        torch.cuda.synchronize()
        out.append([t.clone().view(torch.int32) for t in (flat_d, prm_d, opt.m, opt.v, opt.state, opt.hist)])
        rec = opt.read()
        assert rec["step"] == 1 and rec["grad_norm"] > 1.0 and np.isfinite(prm_d.cpu().numpy()).all()
        assert (prm_d.cpu().numpy() != p0).all()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    _assert_trig_of_fresh_engine(circ, fresh, prm_d[theta_off:NP])


# ---- L-BFGS: the shared helper's second caller
@pytest.mark.parametrize("ans,n", [("cascade", 4), ("cross_mesh", 8)], ids=["cascade4", "cross_mesh8"])
def test_lbfgs_evaluation_leaves_the_tables_of_the_new_theta(ans, n, gpu_device):
    circuits, engine = pkg("circuits"), pkg("hip.engine")
    prog = circuits.build_program(ans, n, 1, True)
    haar = circuits.haar_unitaries(3, 4)
    circ, fresh = engine.Circuit(prog, haar, gpu_device), engine.Circuit(prog, haar, gpu_device)
    assert _table_rows(circ) >= 1
    NP = 300
    theta_off = NP - prog.n_params
    seq, _ = D.scripted(NP, 3, "FA", 9)
    x0 = np.random.default_rng(10).standard_normal(NP).astype(np.float32)
    dev = D.Device(NP, x0, gpu_device, 3, "armijo", circuit=circ, theta_off=theta_off)
    _, parts, g = seq[0]
    x = dev.call(parts, g)
    _assert_trig_of_fresh_engine(circ, fresh, dev.prm[theta_off:NP])
    assert float(np.abs(x - x0)[theta_off:].max()) > 1e-3          # the first evaluation moved theta
    dev.assert_guards()


# ---- fold loads
FOLD_WIDTHS = [(13, 2, 0, 1021), (100, 4, 1022, 2045), (200, 8, 2046, 3069)]      # (H, layers, NP above, NP at most)
FOLD_ROWS = [2, 31, 32, 33]
SCALE = 2.0 ** -10


def _host_fold(P):
    """k_fold_rows, then the left-to-right sum of the surviving rows, in float32: [ncols]."""
    rows = P.shape[0]
    RS, W = min(rows, 32), 8
    hop = RS * W
    zero = np.zeros(P.shape[1], np.float32)
    surv = []
    for rs in range(RS):
        s = []
        for w in range(W):
            r0 = rs + RS * w
            v = [P[r0 + k * hop] if r0 + k * hop < rows else zero for k in range(8)]
            a0, a1 = zero.copy(), zero.copy()
            for k in range(0, 8, 2):
                a0 = a0 + v[k]
                a1 = a1 + v[k + 1]
            r = r0 + 8 * hop
            while r < rows:
                a0 = a0 + P[r]
                if r + hop < rows:
                    a1 = a1 + P[r + hop]
                r += 2 * hop
            s.append(a0 + a1)
        t = s[0]
        for w in range(1, W):
            t = t + s[w]
        surv.append(t)
    t = zero.copy()
    for j in range(RS):
        t = t + surv[j]
    assert t.dtype == np.float32
    return t


@pytest.mark.parametrize("rows", FOLD_ROWS)
@pytest.mark.parametrize("H,layers,lo,hi", FOLD_WIDTHS, ids=[f"H{w[0]}" for w in FOLD_WIDTHS])
def test_fold_and_update_give_the_host_sums_of_the_rows(H, layers, lo, hi, rows, gpu_device):
    Lb, engine = pkg("hip.lib"), pkg("hip.engine")
    n, ans = 2, "cascade"
    rows_val, rows_res = 1, rows - 1
    B_res, B_val = 64 * rows_res - 5, 64 * rows_val - 3
    n_ic = B_val // 2 - 4
    n_bc = B_val - n_ic
    n_theta = layers * pkg("circuits").params_per_layer(ans, n)
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=7)
    model, eng = _model(gpu_device, ans, n, layers, H, flat)
    NP = eng.NP
    assert lo < NP <= hi, NP                                       # NP + 3 in (1024 (k - 1), 1024 k]: k live column blocks
    eng.loss_weights = tuple(SCALE * w for w in eng.loss_weights)
    eng.refresh_gates()
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(NP, 0.005, gpu_device))
    assert fs.part.shape == (rows, NP + 3)
    fs.X_res[:B_res] = X_res.to(gpu_device)
    fs.X_val[:n_ic] = X_ic.to(gpu_device)
    fs.X_val[n_ic:] = X_bc.to(gpu_device)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    fs.part.fill_(float("nan"))
    for stage in range(5):
        assert eng.lib.qc_fused_step_stage(C.byref(fs.desc), stage, st) == 0
    torch.cuda.synchronize()
    P = fs.part.cpu().numpy().copy()
    assert P.dtype == np.float32 and np.isfinite(P).all()
    want = _host_fold(P)
    assert (want[NP:] > 0).all() and np.abs(want[:NP]).max() > 0

    fs.part.fill_(float("nan"))
    fs.flat_grad.fill_(float("nan"))
    fs.run(Lb.QC_PHASE_GRADS | Lb.QC_PHASE_UPDATE)
    torch.cuda.synchronize()
    got = fs.flat_grad.cpu().numpy()
    rec = fs.opt.read()
    print(f"\nfold H={H} rows={rows}: NP={NP}, grad_norm={rec['grad_norm']:.4g}")
    assert rec["step"] == 1 and np.isfinite(eng.flat.cpu().numpy()).all()
    bad = np.flatnonzero(got[NP:] != want[NP:])
    assert bad.size == 0, (got[NP:], want[NP:])                    # the loss columns: never scaled by the clip
    assert (np.float32(rec["loss_res"]), np.float32(rec["loss_bc"]), np.float32(rec["loss_ic"])) == tuple(want[NP:])
    assert rec["grad_norm"] < 0.5                                  # the clip is inactive: its factor is exactly 1
    bad = np.flatnonzero(got[:NP] != want[:NP])
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
