"""The coefficient step without a GPU: the three new exports and their host-side refusals, the float64 reference with
per-point operator rows (reduction to the data step's reference, its negative controls, the Klein-Gordon fixture of the
reference's own operator), TabulatedProblem(coef_res=) and coef_table, and train(..., dataset=) on a classical torch
model through the per-point operator."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import coef_reference as CR
import tabulated_reference as T
from conftest import GOLDEN, pkg
from step_reference import haar_for, step_inputs
from test_gpu_coef import _errors
from test_tabulated_cpu import Tiny, _desc, _segments


# ---- 1. ABI
def test_exports_load_and_step_coef_matches_the_header_layout():
    L = pkg("hip.lib")
    lib = L.load()
    for name in ("qc_post_coef", "qc_sample_dataset_coef", "qc_fused_pinn_coef_step"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert L.QC_COEF_COLS == 7 == len(pkg("data.tabulated").COEF_COLUMNS) == len(CR.COLS)
    assert pkg("data.tabulated").COEF_COLUMNS == CR.COLS
    assert C.sizeof(L.QcStepCoef) == 16 and L.QcStepCoef.ds_coef.offset == 8
    assert lib.qc_version() == 4


def test_argument_errors_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    fake = 4096
    data = lambda: L.QcStepData(fake, fake, 0.0, fake, fake, 10, fake, fake, 10, fake, fake, 10)
    pde = L.QcPde()
    pde.problem = L.QC_PROBLEM_TABULATED
    # qc_post_coef: a missing target, table or cotangent buffer; a problem id other than 3
    post = lambda tg=fake, cf=fake, cot=fake: lib.qc_post_coef(fake, 50, 4, 12, C.byref(pde), fake, tg, cf, cot, fake, fake,
                                                               10 ** 4, 0, 64, None)
    assert post(tg=None) == -1 and post(cf=None) == -1 and post(cot=None) == -1
    pde.problem = L.QC_PROBLEM_CONVECTION_DIFFUSION
    assert post() == -1
    # qc_sample_dataset_coef: absent structures, a missing batch or dataset table behind residual points
    full = L.QcStepCoef(fake, fake)
    call = lambda t, c, cr=fake, n=(5, 3, 2): lib.qc_sample_dataset_coef(
        fake, fake, n[0], 0, fake, fake, n[1], 0, n[2], 0, cr, None if t is None else C.byref(t),
        None if c is None else C.byref(c), 1, 1, None)
    assert call(None, full) == -1 and call(data(), None) == -1
    assert call(data(), full, cr=None) == -1 and call(data(), L.QcStepCoef(fake, None)) == -1
    bad = data()
    bad.ds_n_res = 0
    assert call(bad, full) == -1
    # qc_fused_pinn_coef_step: the refusals of its own check, then those of the data step.  The descriptor's program is
    # null (a program needs a device), so a call that passed both checks would be refused all the same;
    # tests/test_gpu_coef.py::test_refusals_name_one_fault_each repeats them on a descriptor that runs.
    d = _desc(L, L.QC_PROBLEM_TABULATED, 5, 3, 2)
    both = L.QC_PHASE_GRADS | L.QC_PHASE_SAMPLE
    step = lambda t, c, ph: lib.qc_fused_pinn_coef_step(C.byref(d), None if t is None else C.byref(t),
                                                        None if c is None else C.byref(c), ph, None)
    assert step(data(), None, L.QC_PHASE_GRADS) == -1 and step(None, full, L.QC_PHASE_GRADS) == -1
    assert step(data(), L.QcStepCoef(None, fake), L.QC_PHASE_GRADS) == -1
    assert step(data(), L.QcStepCoef(fake, None), both) == -1
    t = data()
    t.target_res_dev = None
    assert step(t, full, L.QC_PHASE_GRADS) == -1
    d.pde.problem = 0
    assert step(data(), full, L.QC_PHASE_GRADS) == -1


# ---- 2. the float64 reference
def test_uniform_table_without_cubic_term_is_the_data_reference():
    n, n_theta = 4, 12
    flat, X_ic, X_bc, X_res = step_inputs(50, n, n_theta, 9, 4, 5, salt=4)
    Xs = [x.double() for x in (X_ic, X_bc, X_res)]
    tg = [T.u_star(X_ic), T.u_star(X_bc), T.r_star(X_res)]
    args = (flat, 50, n, n_theta, (1, 12), "cascade", haar_for(n, 1))
    # the table holds float32 roundings of the coefficients: hand the data reference the same values
    tab = CR.uniform_table(9, T.COEFFS, T.C_U)
    g0, p0 = T.reference_loss_data(*args, *Xs, *tg, coeffs=tuple(float(c) for c in tab[0, 1:6]), c_u=float(tab[0, 0]))
    g1, p1 = CR.reference_loss_coef(*args, *Xs, *tg, tab)
    assert np.abs(g1 - g0).max() < 1e-12 * max(1.0, np.abs(g0).max()) and np.abs(p1 - p0).max() < 1e-12
    # the cubic column is live
    g2, p2 = CR.reference_loss_coef(*args, *Xs, *tg, CR.uniform_table(9, T.COEFFS, T.C_U, c_3=1.0))
    assert abs(p2[0] - p0[0]) > 1e-3 and np.abs(g2 - g0).max() > 1e-3


def test_case_tables_are_fields_not_constants():
    for case in CR.CASES:
        tab = CR.case_table(case)
        B = CR.CASES[case][4]
        assert tab.shape == (B, 7) and tab.dtype == np.float32
        if B == 0:
            continue
        flux = np.arange(B) % 5 == 4
        assert (tab[flux] == CR.FLUX_ROW).all() and flux.sum() >= 4
        live = tab[~flux]
        assert (live.std(0) > 0.03).all()                                     # no column constant
        assert (live[:, 0] > 0).any() and (live[:, 0] < 0).any()              # c_u of both signs
        assert (live[:, 6] > 0).any() and (live[:, 6] < 0).any()              # c_3 of both signs
        assert np.abs(live).max() < 3.0
        for k, default in enumerate((0.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0)):
            assert (np.abs(live[:, k] - default) > 1e-3).mean() > 0.9, CR.COLS[k]


@pytest.mark.parametrize("case,variant", [(c, v) for c, vs in CR.CONTROLS.items() for v in vs])
def test_negative_controls_of_the_gpu_cases_are_not_vacuous(case, variant):
    """Reference against reference under the GPU test's own measure (test_gpu_coef._errors: error / tolerance per
    gradient block and for the loss parts): the true reference, taken as a result, must FAIL each control.  Largest
    error / tolerance of the six (case, control) pairs: reg_cascade4 roll 2460, c3zero 1923, swap_d 34.6 (the smallest);
    wave_layered7 roll 502, c3zero 44.6, swap_d 176."""
    ans, n, L, *_ = CR.CASES[case]
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    ref, bad = CR.case_reference(case), CR.case_reference(case, variant)
    err = _errors(np.concatenate([ref["grad"], ref["parts"]]), bad["grad"], bad["parts"], n, n_theta)
    print(case, variant, {k: float(v) for k, v in err.items()})
    assert max(err.values()) > 1.0, err


def test_klein_gordon_rows_reproduce_the_reference_operator():
    """nn/pde.py:28-41 (u_tt - u_xx + u^3) from tests/golden/other_operators.npz, whose outputs the reference's own
    klein_gordon_operator produced: the fixture's two-input model as a [3, 16, 1] model with a zero first column and (t, x)
    on the x / y slots, the rows d_xx = -1, d_yy = 1, c_3 = 1."""
    z = np.load(os.path.join(GOLDEN, "other_operators.npz"))
    flat, X = kg_inputs(z)
    u, res, _ = CR.residual_points(flat, 16, 4, 12, (1, 12), "cascade", haar_for(4, 1), X.double(),
                                   np.tile(CR.KLEIN_GORDON_ROW, (len(X), 1)))
    for got, key in ((u, "klein_gordon__out0"), (res, "klein_gordon__out1")):
        want = z[key][:, 0]
        assert np.abs(got.detach().numpy() - want).max() < 1e-4 * max(1.0, np.abs(want).max()), key
    assert np.abs(z["klein_gordon__out1"]).max() > 0.1 and np.abs(z["klein_gordon__out0"] ** 3).max() > 1e-3


def kg_inputs(z):
    """(flat (NP,) float32 of a [3, 16, 1] model, X (24, 3) float32 torch) of the Klein-Gordon fixture."""
    w = lambda k: np.asarray(z["klein_gordon__w__" + k], dtype=np.float32)
    W1 = np.concatenate([np.zeros((16, 1), np.float32), w("pre__0__weight")], axis=1)
    flat = np.concatenate([a.reshape(-1) for a in (W1, w("pre__0__bias"), w("pre__2__weight"), w("pre__2__bias"),
                                                   w("post__0__weight"), w("post__0__bias"), w("post__2__weight"),
                                                   w("post__2__bias"), w("q__params"))])
    X2 = np.asarray(z["klein_gordon__X"], dtype=np.float32)
    X = torch.from_numpy(np.concatenate([np.zeros((len(X2), 1), np.float32), X2], axis=1))
    return flat, X


# ---- 3. TabulatedProblem(coef_res=), coef_table
def test_tabulated_problem_validates_its_coefficient_table():
    tab = pkg("data.tabulated")
    TP = tab.TabulatedProblem
    (Xr, Xi, Xb), (r, ui, ub) = _segments()
    coef = torch.from_numpy(CR.coef_star(Xr))
    p = TP(Xr, r, Xi, ui, Xb, ub, coef_res=coef)
    assert p.coef_res.shape == (5, 7) and torch.equal(p.coef_res, coef) and p.to("cpu") is p
    assert TP(Xr, r, Xi, ui, Xb, ub).coef_res is None          # existing calls: scalar operator, no table
    assert TP(Xr, r, Xi, ui, Xb, ub).coeffs == (1.0, 1.0, 1.0, 0.01, 0.01)
    with pytest.raises(ValueError, match=r"shape \(N, 7\)"):
        TP(Xr, r, Xi, ui, Xb, ub, coef_res=coef[:, :6])
    with pytest.raises(ValueError, match=r"shape \(N, 7\)"):
        TP(Xr, r, Xi, ui, Xb, ub, coef_res=coef.reshape(-1))
    with pytest.raises(ValueError, match="float32"):
        TP(Xr, r, Xi, ui, Xb, ub, coef_res=coef.double())
    with pytest.raises(ValueError, match="5 residual points but 4 rows"):
        TP(Xr, r, Xi, ui, Xb, ub, coef_res=coef[:4])
    for kw in (dict(c_u=0.0), dict(c_t=1.0), dict(d_yy=0.01), dict(c_x=2.0, c_y=3.0)):
        with pytest.raises(ValueError, match="do not also give"):
            TP(Xr, r, Xi, ui, Xb, ub, coef_res=coef, **kw)
    # the helper: scalars, arrays and callables of X, columns not given are 0
    t = tab.coef_table(Xr, c_t=1.0, c_x=lambda X: -(X[:, 2] - 0.5), c_y=(Xr[:, 1] - 0.5).numpy(), d_xx=0.02)
    assert t.shape == (5, 7) and t.dtype == torch.float32
    assert torch.equal(t[:, 1], torch.ones(5)) and torch.equal(t[:, 2], -(Xr[:, 2] - 0.5)) and torch.equal(t[:, 3], Xr[:, 1] - 0.5)
    assert torch.equal(t[:, 4], torch.full((5,), 0.02)) and not t[:, [0, 5, 6]].any()
    with pytest.raises(ValueError, match="unknown coefficient"):
        tab.coef_table(Xr, c_4=1.0)
    with pytest.raises(ValueError, match="5 points but 3 values"):
        tab.coef_table(Xr, c_u=torch.ones(3))
    # from_functions evaluates the table on its residual points
    g = torch.Generator().manual_seed(5)
    q = TP.from_functions(lambda X: X[:, 1], lambda X: X[:, 2], lambda X: X[:, 0], 40, 20, 30, generator=g,
                          coef=lambda X: torch.from_numpy(CR.coef_star(X)))
    assert q.sizes() == (40, 20, 30) and torch.equal(q.coef_res, torch.from_numpy(CR.coef_star(q.X_res)))


# ---- 4. the trainers
def test_generic_train_on_a_coefficient_dataset_starts_at_the_reference_loss():
    """One step of the generic torch loop on a coefficient dataset: its first loss is the per-point residual's loss on the
    minibatch torch.randint picks (IC -> BC -> residual), formed by hand in float64."""
    trainer = pkg("trainer.diffusion_train")
    TP = pkg("data.tabulated").TabulatedProblem
    g = torch.Generator().manual_seed(3)
    f32 = lambda f: (lambda X: torch.from_numpy(f(X)))
    ds = TP.from_functions(f32(T.u_star), f32(T.u_star), f32(T.r_star), 50, 20, 30, generator=g, coef=f32(CR.coef_star))
    torch.manual_seed(0)
    m = Tiny()
    m.epochs = 0
    ref = Tiny().double()
    ref.load_state_dict(m.state_dict())
    torch.manual_seed(11)
    trainer.train(m, batch_size=12, dataset=ds)
    assert len(m.loss_history) == 1
    torch.manual_seed(11)
    ki, kb, kr = torch.randint(0, 20, (4,)), torch.randint(0, 30, (4,)), torch.randint(0, 50, (12,))
    grad = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    t, x, y = (ds.X_res[kr][:, k:k + 1].double().requires_grad_(True) for k in range(3))
    u = ref(torch.cat((t, x, y), 1))
    u_x, u_y = grad(u, x), grad(u, y)
    jets = torch.stack([u, grad(u, t), u_x, u_y, grad(u_x, x), grad(u_y, y)])[:, :, 0]
    res = CR.residual_coef(jets, ds.coef_res[kr].numpy())
    want = 2.0 * ((res - ds.r[kr].double()) ** 2).mean() + 4.0 * ((ref(ds.X_bc[kb].double())[:, 0] - ds.u_bc[kb].double()) ** 2).mean() \
        + 2.0 * ((ref(ds.X_ic[ki].double())[:, 0] - ds.u_ic[ki].double()) ** 2).mean()
    assert abs(m.loss_history[0] - want.item()) < 1e-5 * max(1.0, want.item()), (m.loss_history, want.item())
    # the table is what was applied: the scalar operator on the same data starts elsewhere
    torch.manual_seed(0)
    m0 = Tiny()
    m0.epochs = 0
    torch.manual_seed(11)
    trainer.train(m0, batch_size=12, dataset=TP(ds.X_res, ds.r, ds.X_ic, ds.u_ic, ds.X_bc, ds.u_bc))
    assert abs(m0.loss_history[0] - m.loss_history[0]) > 1e-3


def test_train_keeps_refusing_two_input_models(tmp_path):
    """A [2, H, 1] DVPDESolver keeps a zero-padded t column that the step would train: train() refuses it, with or without
    a coefficient dataset (INTEGRATION section 1 shows the [3, H, 1] form of a two-coordinate problem)."""
    from test_modules_cpu import Log, base_args
    trainer = pkg("trainer.diffusion_train")
    TP = pkg("data.tabulated").TabulatedProblem
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    model = Solver(base_args(classic_network=[2, 16, 1]), Log(tmp_path), device=torch.device("cpu"))
    (Xr, Xi, Xb), (r, ui, ub) = _segments()
    ds = TP(Xr, r, Xi, ui, Xb, ub, coef_res=torch.from_numpy(CR.coef_star(Xr)))
    with pytest.raises(ValueError, match=r"classic_network = \[3, H, 1\]"):
        trainer.train(model, batch_size=12, dataset=ds)
    with pytest.raises(ValueError, match=r"classic_network = \[3, H, 1\]"):
        trainer.train(model, batch_size=12)
