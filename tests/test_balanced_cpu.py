"""The balanced step without a GPU: the float64 reference (per-class gradients combined for any p) against the tabulated
step's own record and against central differences of F, the negative controls of the GPU test against the truth under the
GPU test's own measure, AdaptiveMultiLoss (state_dict format, F, weights), the record layout and the argument errors of the
three exports, the trainer's refusals, and the float64 training replay with its held control."""
import ctypes as C

import numpy as np
import pytest
import torch

import balanced_reference as BR
import balanced_training as BT
import tabulated_reference as T
from conftest import pkg

TOL_G, TOL_L = 2e-4, 1e-4          # tests/test_gpu_tabulated.py


def _n_theta(case):
    ans, n, L, *_ = BR.CASES[case]
    return n, L * pkg("circuits").params_per_layer(ans, n)


# ---- the reference
@pytest.mark.parametrize("case", list(BR.CASES))
def test_class_gradients_sum_to_the_tabulated_record(case):
    """2 grad L_r + 4 grad L_bc + 2 grad L_ic and the parts are the data step's committed record (p = 0: e = 1)."""
    rec, tab = BR.class_reference(case), T.case_reference(case)
    g = BR.combine(rec, p=(0.0, 0.0, 0.0))
    assert g.size == tab["grad"].size + 3 and (g[-3:] == 0.0).all()
    assert np.abs(g[:-3] - tab["grad"]).max() < 1e-9 * max(1.0, np.abs(tab["grad"]).max())
    assert np.abs(rec["parts"] - tab["parts"]).max() < 1e-12
    s = BR.log_vars()
    assert np.allclose(s, (0.3, -1.0, 0.4), atol=1e-7) and len(set(np.round(BR.factors(), 6))) == 3


def test_own_gradient_matches_central_differences_of_F():
    parts = BR.class_reference("reg_cascade4")["parts"]
    g = BR.own_gradient(parts)
    h = 2.0 ** -8
    for k in range(3):
        pp, pm = np.array(BR.P0, dtype=np.float64), np.array(BR.P0, dtype=np.float64)
        base = float(np.float32(BR.P0[k]))
        pp[k], pm[k] = np.float32(base + h), np.float32(base - h)
        fd = (BR.objective(parts, pp) - BR.objective(parts, pm)) / (float(pp[k]) - float(pm[k]))
        print(BR.TERMS[k], g[k], fd)
        assert abs(g[k] - fd) < 1e-4 * max(1.0, abs(fd))
    # a frozen term: exactly 0
    assert BR.own_gradient(parts, scale=(1.0, 0.0, 0.5))[1] == 0.0
    # the closed-form fixed point of s_k at fixed L_k: w_k exp(-s_k) L_k = 1
    s_fix = np.log(np.asarray(BR.W) * parts)
    assert np.abs(BR.own_gradient(parts, p=s_fix, scale=(1.0, 1.0, 1.0))).max() < 1e-6


@pytest.mark.parametrize("case,variant", [(c, v) for c, vs in BR.CONTROLS.items() for v in vs])
def test_negative_controls_of_the_gpu_cases_are_not_vacuous(case, variant):
    """Reference against reference under the GPU test's own measure (the block tolerances on the network entries): the
    truth, taken as a result, must FAIL each control in every case it is used on."""
    n, n_theta = _n_theta(case)
    rec = BR.class_reference(case)
    err = BR.block_error(BR.combine(rec), BR.combine(rec, variant=variant), BR.case_H(case), n, n_theta) / TOL_G
    print(case, variant, "error / tolerance", err)
    assert err > 1.0, (case, variant, err)


# ---- AdaptiveMultiLoss
def test_adaptive_multi_loss_state_dict_forward_and_weights():
    AML = pkg("nn.loss_balance").AdaptiveMultiLoss
    assert pkg("nn.loss_balance").TERMS == BR.TERMS
    bal = AML()
    assert sorted(bal.state_dict()) == ["log_vars.bc", "log_vars.ic", "log_vars.residual"]
    assert all(v.shape == (1,) and float(v) == 0.0 for v in bal.state_dict().values())
    assert bal.weights() == {"residual": 1.0, "bc": 1.0, "ic": 1.0}
    # the format a ParameterDict of (1,) parameters saves: keys log_vars.<name>, strict loading
    saved = {"log_vars.residual": torch.tensor([0.25]), "log_vars.bc": torch.tensor([-1.5]), "log_vars.ic": torch.tensor([0.75])}
    bal.load_state_dict(saved, strict=True)
    again = AML()
    again.load_state_dict({k: v.clone() for k, v in bal.state_dict().items()}, strict=True)
    assert all(torch.equal(again.state_dict()[k], v) for k, v in saved.items())
    w = again.weights()
    assert w["residual"] == pytest.approx(np.exp(-0.25)) and w["bc"] == pytest.approx(np.exp(1.5)) and w["ic"] == pytest.approx(np.exp(-0.75))
    # F in float64, with scale and base weights
    bal = AML(scale=BR.SCALE).double()
    bal.scale.data = bal.scale.double()
    with torch.no_grad():
        for name, p in zip(BR.TERMS, BR.P0):
            bal.log_vars[name].fill_(float(np.float32(p)))
    parts = np.array([0.31, 0.052, 0.47])
    losses = {name: torch.tensor(v, dtype=torch.float64) for name, v in zip(BR.TERMS, parts)}
    F = bal(losses, base_weights=dict(zip(BR.TERMS, BR.W)))
    assert float(F.detach()) == pytest.approx(BR.objective(parts), rel=1e-12)
    assert [bal.weights()[k] for k in BR.TERMS] == pytest.approx(list(BR.factors()), rel=1e-12)
    # without base weights: the plain sum exp(-s) L + s; its gradient on p is scale (1 - e L)
    F1 = bal(losses)
    g = torch.autograd.grad(F1, [bal.log_vars[k] for k in BR.TERMS])
    assert [float(x) for x in g] == pytest.approx(list(BR.own_gradient(parts, w=(1.0, 1.0, 1.0))), rel=1e-12)
    for kw, msg in ((dict(names=("a", "a")), "distinct"), (dict(scale=(1.0, 2.0)), "one finite"), (dict(scale=(1.0, float("nan"), 1.0)), "one finite")):
        with pytest.raises(ValueError, match=msg):
            AML(**kw)


# ---- the library
def test_exports_load_and_step_balance_matches_the_header_layout():
    L = pkg("hip.lib")
    lib = L.load()
    for name in ("qc_post_balance", "qc_balance_adam_step", "qc_fused_pinn_balanced_step"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert L.QC_BAL_TERMS == 3 == BR.N_BAL and C.sizeof(L.QcStepBalance) == 32
    assert (L.QcStepBalance.weight_hist_dev.offset, L.QcStepBalance.weight_hist_cap.offset) == (16, 24)
    assert lib.qc_version() == 4
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qcpinn_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*|void)\s+(qc_\w+)\s*\(", header, re.M))
    assert declared == set(L.EXPORTS)


def _bal(L, **kw):
    b = L.QcStepBalance()
    for k in range(3):
        b.scale[k] = BR.SCALE[k]
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(b, k)[v[0]] = v[1]
        else:
            setattr(b, k, v)
    return b


BAD_RECORDS = (dict(scale=(0, float("nan"))), dict(scale=(2, float("inf"))), dict(weight_hist_cap=-1),
               dict(weight_hist_cap=4, weight_hist_dev=None))


def test_argument_errors_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    fake = 4096
    pde = L.QcPde()
    pde.problem = L.QC_PROBLEM_TABULATED
    ref = lambda s: None if s is None else C.byref(s)
    NP_B = pkg("hip.engine").param_layout(50, 4, 12)["__total__"][0] + 3

    def post(bl=_bal(L), tg=fake, stride=NP_B + 3, nch=6):
        return lib.qc_post_balance(fake, 50, 4, 12, C.byref(pde), ref(bl), fake, tg, 0.7, fake, fake, fake, fake, stride, 0, 64,
                                   nch, None)
    assert post(bl=None) == -1 and post(tg=None) == -1
    assert post(stride=NP_B + 2) == -1 and post(nch=1, stride=NP_B + 2) == -1
    for kw in BAD_RECORDS:
        assert post(bl=_bal(L, **kw)) == -1, kw
    pde.problem = L.QC_PROBLEM_CONVECTION_DIFFUSION
    assert post() == -1
    # the optimiser call
    hp = L.QcOptHyper()

    def adam(bl=_bal(L), NP=NP_B, flat=fake, state=fake):
        return lib.qc_balance_adam_step(flat, NP, fake, fake, fake, state, C.byref(hp), ref(bl), None, 0, None, 0, None, None)
    assert adam(bl=None) == -1 and adam(NP=3) == -1 and adam(NP=0) == -1 and adam(flat=None) == -1 and adam(state=None) == -1
    for kw in BAD_RECORDS:
        assert adam(bl=_bal(L, **kw)) == -1, kw
    # (theta_off + n_params > NP_B - 3 needs a program: a device object, tests/test_gpu_balanced.py)
    # the step: a missing or broken record ahead of everything the descriptor is asked
    data = L.QcStepData(fake, fake, 0.0, fake, fake, 10, fake, fake, 10, fake, fake, 10)
    desc = L.QcStepDesc()
    step = lambda d, t, bl: lib.qc_fused_pinn_balanced_step(ref(d), ref(t), ref(bl), L.QC_PHASE_GRADS, None)
    assert step(desc, data, None) == -1 and step(desc, None, _bal(L)) == -1 and step(None, data, _bal(L)) == -1
    for kw in BAD_RECORDS:
        assert step(desc, data, _bal(L, **kw)) == -1, kw
    assert step(desc, data, _bal(L)) == -1           # an empty descriptor


# ---- the trainer's refusals
def test_balanced_trainer_and_train_refuse_what_is_out_of_scope(monkeypatch):
    import tempfile
    from types import SimpleNamespace

    from test_modules_cpu import Log, base_args
    tab = pkg("data.tabulated")
    AML = pkg("nn.loss_balance").AdaptiveMultiLoss
    BTm = pkg("trainer.balanced_train")
    train = pkg("trainer.diffusion_train").train
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    g = torch.Generator().manual_seed(0)
    Xr, Xi, Xb = (torch.rand(m, 3, generator=g) for m in (5, 3, 4))
    r, ui, ub = (torch.rand(m, generator=g) for m in (5, 3, 4))
    ds = tab.TabulatedProblem(Xr, r, Xi, ui, Xb, ub)
    with tempfile.TemporaryDirectory() as d:
        model = Solver(base_args(classic_network=[3, 16, 1]), Log(d), device=torch.device("cpu"))
        bal = AML()
        for call in (lambda **kw: train(model, batch_size=12, balance=kw.pop("balancer", bal), **kw),
                     lambda **kw: BTm.BalancedTrainer(model, 12, kw.pop("dataset", None), kw.pop("balancer", bal), **kw)):
            with pytest.raises(ValueError, match="needs dataset="):
                call()
            with pytest.raises(ValueError, match="coef_res"):
                call(dataset=tab.TabulatedProblem(Xr, r, Xi, ui, Xb, ub, coef_res=torch.zeros(5, 7)))
            with pytest.raises(ValueError, match="exactly the three loss terms"):
                call(dataset=ds, balancer=AML(names=("residual", "bc")))
            with pytest.raises(ValueError, match="exactly the three loss terms"):
                call(dataset=ds, balancer=AML(names=("pde", "bc", "ic")))
            with pytest.raises(ValueError, match="AdaptiveMultiLoss"):
                call(dataset=ds, balancer=torch.nn.Linear(1, 1))
        with pytest.raises(ValueError, match="adaptive="):
            train(model, batch_size=12, dataset=ds, balance=bal, adaptive=tab.AdaptiveSampling())
        with pytest.raises(ValueError, match="lbfgs="):
            train(model, batch_size=12, dataset=ds, balance=bal, lbfgs=pkg("trainer.lbfgs_train").LbfgsPhase(4))
        wide = SimpleNamespace(_engine_for=None, quantum_layer=None, input_dim=3, n_out=2)
        with pytest.raises(ValueError, match=r"\[3, H, 1\]"):
            BTm.check_balance(wide, ds, bal)
        with pytest.raises(ValueError, match="DVPDESolver"):
            BTm.check_balance(torch.nn.Linear(3, 1), ds, bal)
        monkeypatch.setattr(BTm, "_dist_info", lambda: (2, 0))
        with pytest.raises(ValueError, match="world_size"):
            train(model, batch_size=12, dataset=ds, balance=bal)


# ---- the training replay
@pytest.mark.parametrize("case", list(BT.TRAIN_CASES))
def test_fp64_replay_moves_the_weights_and_the_held_control_does_not(case):
    ref, held = BT.training_reference(case), BT.training_reference(case, hold=True)
    assert ref["loss"].shape == (BT.STEPS,) and ref["weights"].shape == (BT.STEPS, 3)
    w0 = np.asarray(BR.W) * BR.factors()
    assert np.abs(ref["weights"][0] - w0).max() < 1e-12 and np.abs(held["weights"] - w0).max() < 1e-12
    assert ref["loss"][0] == pytest.approx(held["loss"][0], rel=1e-12)
    # the GPU test's measure, reference against control: the truth, taken as a result, must FAIL the held weights in every
    # term (Adam moves each p_k by about lr = 0.005 per step, which changes w_k e_k by tenths of a percent and more)
    moved = np.abs(ref["weights"][-1] - held["weights"][-1]) / (1e-4 * np.maximum(1.0, np.abs(held["weights"][-1])))
    print(case, "weights", ref["weights"][0], "->", ref["weights"][-1], "F", ref["loss"], "moved / tolerance", moved)
    assert moved.min() > 1.0, moved
