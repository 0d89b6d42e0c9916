"""The seven-channel step on the GPU: qc_fused_pinn_coef_tt_step (QC_PHASE_GRADS) against the float64 reference of
tests/tt_reference.py, its agreement with the coefficient step on a zero d_tt column, the bits of its gather, three training
steps on the standing-wave problem against a float64 replay, the bits of three steps against a recording of the step as it
was before it shared the other entry points' host code, and the autograd path (DVPDESolver.jets_tt, wave_2d_operator).

Tolerances are the project's (tests/test_gpu_tabulated.py): the gradient block by block at TOL_G x max(1, max |ref block|),
the loss parts at TOL_L, 1e-4 on a loss history and 2e-3 on the weights behind it.  The negative controls (d_tt zeroed, d_tt
and d_xx swapped, the table rolled by one row) must fail the same tolerance; tests/test_tt_cpu.py shows that each moves the
reference by far more."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tt_reference as TR
from conftest import GOLDEN, pkg
from step_reference import haar_for
from test_gpu_coef import _coef_step, _load_coef
from test_gpu_fullsize import Log, base_args
from test_gpu_tabulated import POINT_TOL, TOL_G, TOL_L, _blocks, _errors, _load, _model

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = {"cascade4": ("cascade", 4, 1, 50, 130, 64, 37), "layered5": ("layered", 5, 2, 20, 65, 0, 3), "cascade2": ("cascade", 2, 1, 3, 1, 1, 0)}


def _tt_step(eng, B_res, n_ic, n_bc):
    """A FusedStepTT behind poisoned buffers; the scalar operator of the descriptor is NaN: the step must not read it."""
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    eng.problem, eng.coeffs, eng.c_u = L.QC_PROBLEM_TABULATED, (NAN,) * 5, NAN
    eng.refresh_gates()
    fs = engine.FusedStepTT(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, eng.device),
                            (max(B_res, 1), max(n_ic, 1), max(n_bc, 1)))
    assert fs.coef_res.shape == (8, max(B_res, 1)) and fs.ws_res.shape[1] == 7
    fs.desc.circ_ws_dev, fs.desc.circ_ws_bytes = None, 0        # the step needs no circuit workspace
    for buf in (fs.target_res, fs.target_val, fs.coef_res, fs.ws_res, fs.ws_val):
        buf.fill_(NAN)
    return fs


def _load_tt(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef):
    _load(fs, X_ic, X_bc, X_res, u_ic, u_bc, r_res)
    if len(X_res):
        fs.coef_res[:, :len(X_res)] = torch.as_tensor(np.asarray(coef), dtype=torch.float32).to(fs.eng.device).t()


def _grads(fs):
    fs.run(pkg("hip.lib").QC_PHASE_GRADS)
    torch.cuda.synchronize()
    return fs.flat_grad.cpu().numpy().astype(np.float64)


# ---- 1. the gradient phase against float64
@pytest.mark.parametrize("case", list(CASES))
def test_grads_match_fp64(case, gpu_device):
    ans, n, Lq, H, B_res, n_ic, n_bc = CASES[case]
    n_theta, theta_shape, haar, flat, *batch = TR.case_inputs(*CASES[case])
    coef = batch[-1]
    model, eng = _model(gpu_device, ans, n, Lq, "angle", flat, hidden=H)
    fs = _tt_step(eng, B_res, n_ic, n_bc)
    _load_tt(fs, *batch)
    got = _grads(fs)
    assert np.isfinite(got).all()
    controls = TR.CONTROLS if B_res > 1 else ()
    refs = TR.references_tt(flat, H, n, n_theta, theta_shape, ans, haar, *batch[:-1],
                            [coef] + [TR.variant_table(v, coef) for v in controls])
    err = _errors(got, *refs[0], n, n_theta)
    print(case, "error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    assert np.array_equal(got, _grads(fs))          # two runs, the same bits
    for v, r in zip(controls, refs[1:]):
        bad = _errors(got, *r, n, n_theta)
        assert max(bad.values()) > 1.0, (v, bad)


# ---- 2. a zero d_tt column is the coefficient step
def test_zero_d_tt_agrees_with_the_coefficient_step(gpu_device):
    ans, n, Lq, H, B_res, n_ic, n_bc = CASES["cascade4"]
    n_theta, theta_shape, haar, flat, *batch = TR.case_inputs(*CASES["cascade4"])
    coef = TR.variant_table("dtt_zero", batch[-1])
    model, eng = _model(gpu_device, ans, n, Lq, "angle", flat, hidden=H)
    fs = _tt_step(eng, B_res, n_ic, n_bc)
    _load_tt(fs, *batch[:-1], coef)
    got7 = _grads(fs)
    f6 = _coef_step(eng, B_res, n_ic, n_bc)
    _load_coef(f6, *batch[:-1], coef[:, :7])
    got6 = _grads(f6)
    NP = got6.size - 3
    err = _errors(got7, got6[:NP], got6[NP:], n, n_theta)
    print("seven channels with d_tt = 0 against six, error / tolerance:", err)
    assert max(err.values()) < 1.0, err


# ---- 3. the gather
def test_sample_is_the_dataset_gather_with_eight_columns(gpu_device):
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    st = torch.cuda.current_stream(dev).cuda_stream
    g = np.random.default_rng(9)
    N, (n_res, n_ic, n_bc), offs, seed, step, pad = (300, 40, 50), (130, 33, 31), (64, 5, 7), 12345, 3, 16
    Xs = [g.uniform(0, 1, (m, 3)).astype(np.float32) for m in N]
    Ys = [g.standard_normal(m).astype(np.float32) for m in N]
    tab = g.standard_normal((N[0], 8)).astype(np.float32)
    dX, dY, dT = [torch.from_numpy(a).to(dev) for a in Xs], [torch.from_numpy(a).to(dev) for a in Ys], torch.from_numpy(tab).to(dev)
    data = L.QcStepData(None, None, 0.0, dX[0].data_ptr(), dY[0].data_ptr(), N[0], dX[1].data_ptr(), dY[1].data_ptr(), N[1],
                        dX[2].data_ptr(), dY[2].data_ptr(), N[2])
    nan = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=dev)
    n_val = n_ic + n_bc

    def buffers():
        return nan(n_res + pad, 3), nan(n_res + pad), nan(n_val + pad, 3), nan(n_val + pad)
    Xr, tr, Xv, tv = buffers()
    cr = nan(8 * n_res + pad)
    cf = L.QcStepCoefTT(cr.data_ptr(), dT.data_ptr())
    L.check(lib.qc_sample_dataset_coef_tt(Xr.data_ptr(), tr.data_ptr(), n_res, offs[0], Xv.data_ptr(), tv.data_ptr(), n_ic, offs[1],
                                          n_bc, offs[2], cr.data_ptr(), C.byref(data), C.byref(cf), seed, step, st),
            "qc_sample_dataset_coef_tt")
    Xr0, tr0, Xv0, tv0 = buffers()
    L.check(lib.qc_sample_dataset(Xr0.data_ptr(), tr0.data_ptr(), n_res, offs[0], Xv0.data_ptr(), tv0.data_ptr(), n_ic, offs[1],
                                  n_bc, offs[2], C.byref(data), seed, step, st), "qc_sample_dataset")
    torch.cuda.synchronize(dev)
    for a, b in ((Xr, Xr0), (tr, tr0), (Xv, Xv0), (tv, tv0)):       # NaN-filled tails included: nothing past the batch
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert torch.isnan(Xr[n_res:]).all() and torch.isnan(tr[n_res:]).all() and torch.isnan(Xv[n_val:]).all()
    assert torch.isfinite(Xr[:n_res]).all() and torch.isfinite(tv[:n_val]).all()
    # the eight columns are the dataset's rows at the drawn indices (the dataset's points are distinct: a point names its row)
    key = {x.tobytes(): k for k, x in enumerate(Xs[0])}
    idx = np.array([key[x.tobytes()] for x in Xr.cpu().numpy()[:n_res]])
    assert len(set(idx)) > n_res // 2 and np.array_equal(tr.cpu().numpy()[:n_res], Ys[0][idx])
    c = cr.cpu().numpy()
    assert np.isnan(c[8 * n_res:]).all() and np.array_equal(c[:8 * n_res].reshape(8, n_res), tab[idx].T)


# ---- 4. three training steps on the standing wave against the float64 replay
def test_training_on_the_standing_wave_matches_the_fp64_replay(gpu_device, tmp_path):
    from oracle import solver as osol
    trainer = pkg("trainer.diffusion_train")
    TP = pkg("data.tabulated").TabulatedProblem
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    STEPS, B, NV = 3, 128, 64
    args = base_args(num_qubits=4, classic_network=[3, 8, 1], batch_size=B, epochs=STEPS - 1)

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(args, TmpLog(), device=gpu_device)
    torch.manual_seed(1)
    ref_model = osol.OracleSolver(args, device=torch.device("cpu"))
    Xr, rr, Xi, ui, Xb, ub, rows = (torch.from_numpy(a) for a in TR.wave_dataset())
    ds = TP(Xr, rr, Xi, ui, Xb, ub, coef_res=rows[:, :7].contiguous(), d_tt=rows[:, 7].contiguous())
    assert torch.equal(ds.coef_tt, rows)
    tr = trainer.FusedTrainer(model, B, capacity=STEPS, dataset=ds, n_ic=NV, n_bc=NV)
    assert tr.tt and type(tr.fs).__name__ == "FusedStepTT"
    batches = []
    for _ in range(STEPS):
        tr.sample()
        tr.step()
        fs = tr.fs
        Xv, tv = fs.X_val.cpu().numpy(), fs.target_val.cpu().numpy()
        batches.append((Xv[:NV], Xv[NV:2 * NV], fs.X_res.cpu().numpy()[:B], tv[:NV], tv[NV:2 * NV], fs.target_res.cpu().numpy()[:B],
                        fs.coef_res.cpu().numpy()[:, :B].T.copy()))
    kinds = {tuple(r) for b in batches for r in b[6]}
    assert len(kinds) == 2                         # interior rows and u_t rows were both drawn
    got = np.array(tr.opt.loss_history(STEPS))
    want, flat_ref = TR.replay_tt(ref_model, batches)
    print("loss history", got, want)
    assert got.shape == want.shape == (STEPS,)
    assert np.abs(got - want).max() < 1e-4 * max(1.0, np.abs(want).max()), (got, want)
    flat = model._flat.cpu().numpy().astype(np.float64)
    print("weights: max |difference|", np.abs(flat - flat_ref).max())
    assert np.abs(flat - flat_ref).max() < 2e-3
    # train() routes the same dataset to the same step
    torch.manual_seed(1)
    m2 = Solver(args, TmpLog(), device=gpu_device)
    trainer.train(m2, batch_size=B, dataset=ds)
    assert len(m2.loss_history) == STEPS and np.isfinite(m2.loss_history).all()


# ---- 5. the bits of the step, recorded before it was routed through the step plan of the other entry points
# (B_res, n_ic, n_bc): both streams (two residual tiles, a full and a partial value tile); no side stream; no residual pipeline
BITS_SHAPES = ((128, 64, 5), (128, 0, 0), (0, 64, 5))
BITS_STEPS = 3


def step_bits(gpu_device, B_res, n_ic, n_bc, split_first=False):
    """{"flat", "m", "v" (BITS_STEPS, NP), "loss" (BITS_STEPS, 3)} after each of BITS_STEPS steps SAMPLE | GRADS | UPDATE of
    the cascade model n = 2, H = 3 from the seeded weights of TR.case_inputs, sampler seed 2024, on a resident dataset of
    11 / 4 / 6 rows; ``split_first``: the first step as three calls, one phase each."""
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    _, _, _, flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef = TR.case_inputs("cascade", 2, 1, 3, 11, 4, 6)
    model, eng = _model(gpu_device, "cascade", 2, 1, "angle", flat, hidden=3)
    eng.problem, eng.coeffs, eng.c_u = L.QC_PROBLEM_TABULATED, (NAN,) * 5, NAN
    eng.refresh_gates()
    opt = engine.OptimState(eng.NP, 0.005, eng.device)
    fs = engine.FusedStepTT(eng, B_res, n_ic, n_bc, opt, (max(B_res, 1), max(n_ic, 1), max(n_bc, 1)))
    to = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(gpu_device)
    fs.set_dataset(((to(X_res), to(r_res)), (to(X_ic), to(u_ic)), (to(X_bc), to(u_bc))), to(coef))
    fs.set_sampler(2024)
    phases = (L.QC_PHASE_SAMPLE, L.QC_PHASE_GRADS, L.QC_PHASE_UPDATE)
    out = {"flat": [], "m": [], "v": [], "loss": []}
    for s in range(BITS_STEPS):
        for ph in (phases if split_first and s == 0 else (sum(phases),)):
            fs.run(ph)
        torch.cuda.synchronize()
        for k, t in (("flat", eng.flat), ("m", opt.m), ("v", opt.v), ("loss", opt.state[6:9])):
            out[k].append(t.detach().cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


@pytest.mark.parametrize("shape", BITS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_bits_are_those_of_the_recorded_step(shape, gpu_device):
    """Flat parameters, m, v and the three logged loss sums after each of three steps, bit for bit against
    tests/golden/tt_step_bits.npz (tests/golden/make_tt_step_bits.py: recorded on the GPU from the step as it was before the
    entry point was routed through the step plan; two recorded runs agreed in every bit, the step's reductions being
    fixed-order).  A step issued as three calls, one phase each, gives the bits of the combined call."""
    want = np.load(os.path.join(GOLDEN, "tt_step_bits.npz"))
    key = "x".join(map(str, shape))
    got, split = step_bits(gpu_device, *shape), step_bits(gpu_device, *shape, split_first=True)
    for k in ("flat", "m", "v", "loss"):
        w = want[f"{key}__{k}"]
        assert got[k].shape == w.shape and got[k].dtype == w.dtype == np.float32
        assert np.isfinite(w).all() and not np.array_equal(w[0], w[-1])      # the recorded steps moved
        assert np.array_equal(got[k].view(np.uint32), w.view(np.uint32)), (k, np.abs(got[k] - w).max())
        assert np.array_equal(split[k].view(np.uint32), w.view(np.uint32)), (k, "one call per phase", np.abs(split[k] - w).max())


# ---- 6. the autograd path
def test_jets_tt_and_the_wave_operator(gpu_device):
    pde = pkg("nn.pde")
    ans, n, Lq, H, B = "cascade", 4, 1, 50, 70
    n_theta, theta_shape, haar, flat, _, _, X_res, *_ = TR.case_inputs(ans, n, Lq, H, B, 0, 0)
    model, eng = _model(gpu_device, ans, n, Lq, "angle", flat, hidden=H)
    X = torch.from_numpy(X_res).to(gpu_device)
    before = model.jets(X).detach().clone()
    J = model.jets_tt(X)
    assert J.shape == (B, 7)
    from step_reference import unpack
    P = unpack(flat, H, n, n_theta)
    want = TR.u_jets7(P, torch.from_numpy(X_res).double(), theta_shape, ans, n, haar)
    point = POINT_TOL * max(1.0, want.abs().max().item())      # the bound of a channel of u (tests/test_gpu_tabulated.py)
    e = np.abs(J.detach().cpu().numpy().T - want.detach().numpy()).max() / point
    print("jets_tt error / tolerance:", e)
    assert e < 1.0
    assert torch.equal(model.jets(X).detach(), before)          # jets() is what it was, bit for bit
    assert np.abs((J[:, :6].detach() - before).cpu().numpy()).max() < 2.0 * point      # two results, each within `point` of the truth
    c, damping = 0.7, 0.3
    model.zero_grad()
    u, res = pde.wave_2d_operator(model, X, c=c, damping=damping)
    assert u.shape == res.shape == (B, 1)
    loss = (res ** 2).mean() + (u ** 2).mean()
    loss.backward()
    got = np.concatenate([p.grad.detach().cpu().numpy().reshape(-1) for p in model.parameters()]).astype(np.float64)
    r64 = want[6] + damping * want[1] - c * c * (want[4] + want[5])
    l64 = (r64 ** 2).mean() + (want[0] ** 2).mean()
    g64 = torch.autograd.grad(l64, [P[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "theta")])
    g64 = np.concatenate([g.numpy().reshape(-1) for g in g64])
    assert abs(loss.item() - l64.item()) < TOL_L * max(1.0, abs(l64.item()))
    err = {k: np.abs(got[s] - g64[s]).max() / (TOL_G * max(1.0, np.abs(g64[s]).max())) for k, s in _blocks(n, n_theta, H).items()}
    print("wave_2d_operator gradient, error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    # the operators are sums of channels: their error is at most the channels' bound times the sum of the |coefficients|
    # (the cubic term: |d u^3| <= 3 u^2 |d u|)
    assert np.abs(res.detach().cpu().numpy()[:, 0] - r64.detach().numpy()).max() < point * (1.0 + damping + 2.0 * c * c)
    uk, rk = pde.klein_gordon_2d_operator(model, X)
    k64 = want[6] - (want[4] + want[5]) + want[0] ** 3
    assert np.abs(rk.detach().cpu().numpy()[:, 0] - k64.detach().numpy()).max() < point * (3.0 + 3.0 * want[0].abs().max().item() ** 2)
    assert torch.equal(uk, u)
