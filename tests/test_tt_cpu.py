"""The seven-channel stages and step (channel 6 = d2/dt2, operator rows of eight columns) without a GPU: the exports and
their host-side refusals, the float64 reference of tests/tt_reference.py against an independent double autograd.grad of
u(X), its negative controls, TabulatedProblem(d_tt=) and the trainers' refusals."""
import ctypes as C
import tempfile

import numpy as np
import pytest
import torch

import mlp_reference as R
import tt_reference as TR
from conftest import pkg
from step_reference import haar_for, step_inputs, unpack
from test_gpu_fullsize import Log, base_args
from test_tabulated_cpu import _desc

TT_EXPORTS = ("qc_pre_forward_tt", "qc_pre_backward_tt", "qc_forward_jets_tt", "qc_backward_jets_tt", "qc_post_coef_tt",
              "qc_post_jets_tt", "qc_sample_dataset_coef_tt", "qc_fused_pinn_coef_tt_step")
# the bounds the GPU tests apply (tests/test_gpu_tabulated.py), restated: importing that module would mark this one `gpu`
TOL_G, TOL_L = 2e-4, 1e-4


# ---- 1. ABI
def test_exports_load_and_the_records_match_the_header():
    L = pkg("hip.lib")
    lib = L.load()
    for name in TT_EXPORTS:
        assert name in L.EXPORTS and hasattr(lib, name)
    tab = pkg("data.tabulated")
    assert L.QC_NCH_TT == 7 and L.QC_COEF_TT_COLS == 8 == len(tab.COEF_TT_COLUMNS) == len(TR.COLS)
    assert tab.COEF_TT_COLUMNS == tab.COEF_COLUMNS + ("d_tt",) == TR.COLS
    assert C.sizeof(L.QcStepCoefTT) == 16 and L.QcStepCoefTT.ds_coef.offset == 8
    assert lib.qc_version() == 4


def test_argument_errors_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    fake = 4096
    data = lambda: L.QcStepData(fake, fake, 0.0, fake, fake, 10, fake, fake, 10, fake, fake, 10)
    pde = L.QcPde()
    pde.problem = L.QC_PROBLEM_TABULATED
    # the stages: a NULL buffer each; qc_post_coef_tt: a problem id other than 3
    assert lib.qc_pre_forward_tt(None, fake, 50, 4, 12, fake, 64, None) == -1
    assert lib.qc_pre_forward_tt(fake, fake, 50, 4, 12, None, 64, None) == -1
    assert lib.qc_pre_backward_tt(fake, fake, 50, 4, 12, None, fake, 10 ** 4, 0, 64, None) == -1
    assert lib.qc_pre_backward_tt(fake, fake, 50, 4, 12, fake, None, 10 ** 4, 0, 64, None) == -1
    assert lib.qc_forward_jets_tt(None, fake, None, fake, fake, 64, None) == -1
    assert lib.qc_backward_jets_tt(None, fake, None, fake, fake, fake, fake, 64, 0, 64, None) == -1
    post = lambda tg=fake, cf=fake, cot=fake: lib.qc_post_coef_tt(fake, 50, 4, 12, C.byref(pde), fake, tg, cf, cot, fake, fake,
                                                                  10 ** 4, 0, 64, None)
    assert post(tg=None) == -1 and post(cf=None) == -1 and post(cot=None) == -1
    assert lib.qc_post_jets_tt(2, fake, 50, 4, 12, fake, fake, fake, fake, 10 ** 4, 0, 64, None) == -1
    assert lib.qc_post_jets_tt(4, fake, 50, 4, 12, fake, None, None, None, 0, 0, 64, None) == -1
    pde.problem = L.QC_PROBLEM_CONVECTION_DIFFUSION
    assert post() == -1
    # the stages serve 2 <= n <= 5: any other qubit count is refused as unsupported before a launch
    assert lib.qc_pre_forward_tt(fake, fake, 50, 6, 12, fake, 64, None) == -2
    # qc_sample_dataset_coef_tt: absent structures, a missing batch or dataset table behind residual points
    full = L.QcStepCoefTT(fake, fake)
    call = lambda t, c, cr=fake, n=(5, 3, 2): lib.qc_sample_dataset_coef_tt(
        fake, fake, n[0], 0, fake, fake, n[1], 0, n[2], 0, cr, None if t is None else C.byref(t),
        None if c is None else C.byref(c), 1, 1, None)
    assert call(None, full) == -1 and call(data(), None) == -1
    assert call(data(), full, cr=None) == -1 and call(data(), L.QcStepCoefTT(fake, None)) == -1
    bad = data()
    bad.ds_n_res = 0
    assert call(bad, full) == -1
    # qc_fused_pinn_coef_tt_step: absent records, a bad problem id; the descriptor's program is null, so a call that passed
    # these would be refused all the same (tests/test_gpu_tt_stages.py repeats the refusals on programs that exist)
    d = _desc(L, L.QC_PROBLEM_TABULATED, 5, 3, 2)
    step = lambda t, c, ph=L.QC_PHASE_GRADS: lib.qc_fused_pinn_coef_tt_step(C.byref(d), None if t is None else C.byref(t),
                                                                           None if c is None else C.byref(c), ph, None)
    assert step(data(), None) == -1 and step(None, full) == -1 and step(data(), full) == -1
    assert lib.qc_fused_pinn_coef_tt_step(None, C.byref(data()), C.byref(full), L.QC_PHASE_GRADS, None) == -1
    d.pde.problem = 0
    assert step(data(), full) == -1


# ---- 2. the float64 reference
@pytest.mark.parametrize("n,ansatz", [(2, "cascade"), (4, "cascade")])
def test_the_column_swap_gives_the_second_time_derivative(n, ansatz):
    """All seven channels of tt_reference against a double autograd.grad of the composed float64 model u(X) (n = 4 with the
    fixed two-wire unitaries), H = 5, B = 7."""
    H, B, L = 5, 7, 1
    Pl = int(pkg("circuits").params_per_layer(ansatz, n))
    flat, _, _, X = step_inputs(H, n, L * Pl, B, 0, 0, salt=11)
    P = unpack(flat, H, n, L * Pl)
    haar = haar_for(n, 1)
    got = TR.u_jets7(P, X.double(), (L, Pl), ansatz, n, haar).detach().numpy()
    want = TR.autograd_jets7(P, X.double(), (L, Pl), ansatz, n, haar).numpy()
    assert got.shape == want.shape == (7, B)
    err = np.abs(got - want).max(axis=1) / (1e-9 * max(1.0, np.abs(want).max()))
    print("channel errors / bound:", err)
    assert err.max() < 1.0, err
    assert np.abs(want[6]).max() > 1e-3 and np.abs(want[6] - want[4]).max() > 1e-3       # u_tt is there and is not u_xx


def test_negative_controls_move_the_reference_far_beyond_the_gpu_bounds():
    """Every control table changes loss and gradient by many times TOL_L / TOL_G; the ratios are printed."""
    ansatz, n, L, H = "cascade", 2, 1, 5
    n_theta, theta_shape, haar, flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef = TR.case_inputs(ansatz, n, L, H, 7, 2, 3)
    ref = lambda tab: TR.reference_loss_tt(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc,
                                           r_res, tab)
    g0, p0 = ref(coef)
    assert np.isfinite(g0).all() and np.abs(g0).max() > 1e-3
    for v in TR.CONTROLS:
        g, p = ref(TR.variant_table(v, coef))
        rg = np.abs(g - g0).max() / (TOL_G * max(1.0, np.abs(g0).max()))
        rl = np.abs(p - p0).max() / (TOL_L * max(1.0, np.abs(p0).max()))
        print(f"{v}: gradient moves by {rg:.0f} x TOL_G, loss by {rl:.0f} x TOL_L")
        assert rg > 50 and rl > 50, (v, rg, rl)
    # d_tt = 0 reduces the reference to the coefficient step's
    import coef_reference as CR
    z = TR.variant_table("dtt_zero", coef)
    g6, p6 = CR.reference_loss_coef(flat, H, n, n_theta, theta_shape, ansatz, haar, *(torch.as_tensor(x).double() for x in
                                                                                      (X_ic, X_bc, X_res)), u_ic, u_bc, r_res, z[:, :7])
    g7, p7 = ref(z)
    assert np.abs(g6 - g7).max() < 1e-12 and np.abs(p6 - p7).max() < 1e-12


# ---- 3. TabulatedProblem(d_tt=)
def _segs(seed=0, m=(6, 3, 4)):
    g = torch.Generator().manual_seed(seed)
    Xr, Xi, Xb = (torch.rand(k, 3, generator=g) for k in m)
    r, ui, ub = (torch.rand(k, generator=g) for k in m)
    return Xr, r, Xi, ui, Xb, ub


def test_tabulated_problem_takes_d_tt():
    tab = pkg("data.tabulated")
    s = _segs()
    Xr = s[0]
    plain = tab.TabulatedProblem(*s, c_t=0.0, c_x=0.5, c_y=0.0, d_xx=4.0, d_yy=2.0, c_u=0.25)
    assert plain.d_tt is None and plain.coef_tt is None
    scalar = tab.TabulatedProblem(*s, c_t=0.0, c_x=0.5, c_y=0.0, d_xx=4.0, d_yy=2.0, c_u=0.25, d_tt=-1.0)
    assert scalar.coef_tt.shape == (6, 8) and scalar.coef_tt.dtype == torch.float32
    assert torch.equal(scalar.coef_tt, torch.tensor([0.25, 0.0, 0.5, 0.0, 4.0, 2.0, 0.0, -1.0]).repeat(6, 1))
    # d_tt=None leaves the rest as it is, and d_tt changes nothing but itself
    assert scalar.coef_res is None and scalar.coeffs == plain.coeffs and scalar.c_u == plain.c_u
    assert all(torch.equal(a, b) for sa, sb in zip(scalar.segments(), plain.segments()) for a, b in zip(sa, sb))
    col = torch.linspace(-1, 1, 6)
    for given in (col, col.reshape(-1, 1), lambda X: X[:, 0] * 0 + col):
        p = tab.TabulatedProblem(*s, d_tt=given)
        assert torch.equal(p.d_tt, col) and torch.equal(p.coef_tt[:, 7], col)
    rows = tab.coef_table(Xr, c_u=1.0, c_x=lambda X: X[:, 1], d_xx=2.0, c_3=-0.5)
    both = tab.TabulatedProblem(*s, coef_res=rows, d_tt=col)
    assert torch.equal(both.coef_tt[:, :7], rows) and torch.equal(both.coef_tt[:, 7], col) and torch.equal(both.coef_res, rows)
    assert torch.equal(both.to("cpu").coef_tt, both.coef_tt)
    with pytest.raises(ValueError, match="6 points but 5 values"):
        tab.TabulatedProblem(*s, d_tt=col[:5])
    with pytest.raises(ValueError, match="float32"):
        tab.TabulatedProblem(*s, d_tt=col.double())
    with pytest.raises(ValueError, match="float32"):
        tab.TabulatedProblem(*s, d_tt=torch.arange(6))
    with pytest.raises(ValueError, match="shape"):
        tab.TabulatedProblem(*s, d_tt=torch.zeros(6, 2))
    with pytest.raises(ValueError, match="not finite"):
        tab.TabulatedProblem(*s, d_tt=float("nan"))
    ff = tab.TabulatedProblem.from_functions(lambda X: X[:, 1], lambda X: X[:, 2] * 0, lambda X: X[:, 0] * 0, 8, 4, 4,
                                             generator=torch.Generator().manual_seed(1), c_t=0.0, c_x=0.0, c_y=0.0, d_xx=1.0,
                                             d_yy=1.0, d_tt=lambda X: -1.0 - X[:, 0])
    assert ff.coef_tt.shape == (8, 8) and torch.equal(ff.coef_tt[:, 7], -1.0 - ff.X_res[:, 0])


# ---- 4. the trainers refuse what the seven-channel step does not serve
def test_trainers_refuse_with_the_reason():
    tab, DT = pkg("data.tabulated"), pkg("trainer.diffusion_train")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    ds = tab.TabulatedProblem(*_segs(), c_t=0.0, c_x=0.0, c_y=0.0, d_xx=1.0, d_yy=1.0, d_tt=-1.0)
    assert DT.is_tt(ds) and not DT.is_tt(tab.TabulatedProblem(*_segs())) and not DT.is_tt(None)
    AML, GN = pkg("nn.loss_balance").AdaptiveMultiLoss, pkg("nn.loss_balance").GradNormWeighting
    with tempfile.TemporaryDirectory() as d:
        mk = lambda **kw: Solver(base_args(classic_network=[3, 8, 1], **kw), Log(), device=torch.device("cpu"))
        model = mk()
        for kw, what in ((dict(balance=AML()), "balance="), (dict(causal=tab.CausalWeighting(2)), "causal="),
                         (dict(gradnorm=GN()), "gradnorm="), (dict(adaptive=tab.AdaptiveSampling()), "adaptive="),
                         (dict(lbfgs=pkg("trainer.lbfgs_train").LbfgsPhase(3)), "lbfgs=")):
            with pytest.raises(ValueError, match=what + " is not supported for a problem with d_tt"):
                DT.train(model, batch_size=12, dataset=ds, **kw)
        with pytest.raises(ValueError, match="adaptive= is not supported for a problem with d_tt"):
            DT.FusedTrainer(model, 12, 4, dataset=ds, adaptive=tab.AdaptiveSampling())
        with pytest.raises(ValueError, match="InverseTrainer is not supported for a problem with d_tt"):
            pkg("trainer.inverse_train").InverseTrainer(model, 12, ds, tab.LearnedOperator(learn={"d_xx": 1.0}))
        with pytest.raises(ValueError, match="SystemTrainer is not supported for a problem with d_tt"):
            pkg("trainer.system_train").SystemTrainer(model, 12, ds)
        with pytest.raises(ValueError, match="balance= is not supported for a problem with d_tt"):
            pkg("trainer.balanced_train").BalancedTrainer(model, 12, ds, AML())
        with pytest.raises(ValueError, match="causal= is not supported for a problem with d_tt"):
            pkg("trainer.causal_train").CausalTrainer(model, 128, ds, tab.CausalWeighting(2))
        with pytest.raises(ValueError, match="gradnorm= is not supported for a problem with d_tt"):
            pkg("trainer.gradnorm_train").GradNormTrainer(model, 192, GN(), ds)

        class Fused:        # what LbfgsTrainer reads of a FusedTrainer ahead of its first device call
            world, adaptive, tt = 1, None, True
        with pytest.raises(ValueError, match="LbfgsTrainer is not supported for a problem with d_tt"):
            pkg("trainer.lbfgs_train").LbfgsTrainer(Fused())
        # the model: qubit count, Fourier features, re-uploading, more than one process, a model that is no DVPDESolver
        with pytest.raises(ValueError, match="2 .. 5 qubits"):
            DT.FusedTrainer(mk(num_qubits=6), 12, 4, dataset=ds)
        with pytest.raises(ValueError, match="fourier_features"):
            DT.FusedTrainer(mk(fourier_features=4), 12, 4, dataset=ds)
        with pytest.raises(ValueError, match="reupload"):
            DT.FusedTrainer(mk(reupload=True, num_quantum_layers=2), 12, 4, dataset=ds)
        with pytest.raises(ValueError, match="world_size > 1"):
            DT.check_tt(model, ds, 2)
        with pytest.raises(ValueError, match="only supported for DVPDESolver"):
            DT.train(torch.nn.Linear(3, 1), batch_size=12, dataset=ds)
        DT.check_tt(model, ds)          # a model the step serves passes
