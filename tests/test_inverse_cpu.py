"""The inverse step without a GPU: LearnedOperator's validation, the float64 reference's operator gradient against central
differences, the negative controls of the GPU test against the truth under the GPU test's own measure, the record layout
and the argument errors of the two exports, and the float64 identification run the GPU test is compared with."""
import ctypes as C

import numpy as np
import pytest
import torch

import inverse_reference as IR
import inverse_training as IT
import tabulated_reference as T
from conftest import pkg
from step_reference import haar_for, step_inputs

TOL_G, TOL_L = 2e-4, 1e-4          # tests/test_gpu_tabulated.py


def test_learned_operator_validates_its_dicts():
    tab = pkg("data.tabulated")
    LO = tab.LearnedOperator
    op = LO(fixed={"c_t": 1.0, "d_xx": 0.05}, learn={"c_x": 0.2, "d_yy": 0.01}, scale={"d_yy": 0.01})
    assert [n for n, _ in op.named_parameters()] == ["p"] and op.p.shape == (7,) and float(op.p.detach().abs().max()) == 0.0
    assert sorted(n for n, _ in op.named_buffers()) == ["base", "scale"]
    assert op.base.tolist() == pytest.approx([0.0, 1.0, 0.2, 0.0, 0.05, 0.01, 0.0])
    assert op.scale.tolist() == pytest.approx([0.0, 0.0, 1.0, 0.0, 0.0, 0.01, 0.0])
    c = op.coefficients()
    assert tuple(c) == tab.COEF_COLUMNS and c["c_x"] == pytest.approx(0.2) and c["c_y"] == 0.0
    with torch.no_grad():
        op.p.copy_(torch.arange(7.0))           # a frozen column ignores its p
    c = op.coefficients()
    assert c["c_t"] == 1.0 and c["c_x"] == pytest.approx(2.2) and c["d_yy"] == pytest.approx(0.01 + 0.05)
    assert LO().coefficients() == dict.fromkeys(tab.COEF_COLUMNS, 0.0)
    for kw, msg in ((dict(fixed={"c_z": 1.0}), "unknown"), (dict(learn={"vx": 1.0}), "unknown"),
                    (dict(fixed={"c_x": 1.0}, learn={"c_x": 0.5}), "fixed and as learned"),
                    (dict(fixed={"c_x": float("nan")}), "not finite"), (dict(learn={"c_x": float("inf")}), "not finite"),
                    (dict(learn={"c_x": 1.0}, scale={"c_x": 0.0}), "> 0"), (dict(learn={"c_x": 1.0}, scale={"c_x": -1.0}), "> 0"),
                    (dict(learn={"c_x": 1.0}, scale={"c_x": float("nan")}), "> 0"),
                    (dict(fixed={"c_t": 1.0}, scale={"c_t": 2.0}), "learned columns only")):
        with pytest.raises(ValueError, match=msg):
            LO(**kw)


def test_exports_load_and_step_learn_matches_the_header_layout():
    L = pkg("hip.lib")
    lib = L.load()
    for name in ("qc_post_learn", "qc_fused_pinn_inverse_step"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert C.sizeof(L.QcStepLearn) == 72
    assert (L.QcStepLearn.scale.offset, L.QcStepLearn.coef_hist_dev.offset, L.QcStepLearn.coef_hist_cap.offset) == (28, 56, 64)
    assert IR.COLS == pkg("data.tabulated").COEF_COLUMNS and lib.qc_version() == 4


def _learn(L, **kw):
    lr = L.QcStepLearn()
    for k in range(7):
        lr.base[k], lr.scale[k] = IR.BASE[k], IR.SCALE[k]
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(lr, k)[v[0]] = v[1]
        else:
            setattr(lr, k, v)
    return lr


def test_argument_errors_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    fake = 4096
    pde = L.QcPde()
    pde.problem = L.QC_PROBLEM_TABULATED
    NP_L = pkg("hip.engine").param_layout(50, 4, 12)["__total__"][0] + 7

    def post(lr=_learn(L), tg=fake, cot=fake, stride=NP_L + 3):
        return lib.qc_post_learn(fake, 50, 4, 12, C.byref(pde), None if lr is None else C.byref(lr), fake, tg, cot, fake, fake,
                                 stride, 0, 64, None)
    assert post(lr=None) == -1 and post(tg=None) == -1 and post(cot=None) == -1
    assert post(stride=NP_L + 2) == -1
    for bad in (_learn(L, base=(2, float("nan"))), _learn(L, scale=(6, float("inf"))), _learn(L, coef_hist_cap=-1),
                _learn(L, coef_hist_cap=4, coef_hist_dev=None)):
        assert post(lr=bad) == -1
    pde.problem = L.QC_PROBLEM_CONVECTION_DIFFUSION
    assert post() == -1
    # the step: a missing record ahead of everything the descriptor is asked
    data = L.QcStepData(fake, fake, 0.0, fake, fake, 10, fake, fake, 10, fake, fake, 10)
    desc = L.QcStepDesc()
    step = lambda d, t, lr: lib.qc_fused_pinn_inverse_step(None if d is None else C.byref(d), None if t is None else C.byref(t),
                                                           None if lr is None else C.byref(lr), L.QC_PHASE_GRADS, None)
    assert step(desc, data, None) == -1 and step(desc, None, _learn(L)) == -1 and step(None, data, _learn(L)) == -1
    assert step(desc, data, _learn(L, base=(0, float("nan")))) == -1 and step(desc, data, _learn(L, coef_hist_cap=-3)) == -1
    assert step(desc, data, _learn(L)) == -1           # an empty descriptor


def _small():
    n, n_theta = 4, 12
    flat, X_ic, X_bc, X_res = step_inputs(50, n, n_theta, 9, 4, 5, salt=4)
    Xs = [x.double() for x in (X_ic, X_bc, X_res)]
    tg = [T.u_star(X_ic), T.u_star(X_bc), T.r_star(X_res)]
    return (flat, 50, n, n_theta, (1, 12), "cascade", haar_for(n, 1)), Xs, tg


def test_operator_gradient_matches_central_differences():
    args, Xs, tg = _small()
    g, parts = IR.reference_loss_inverse(*args, *Xs, *tg)
    NP = g.size - 7
    loss = lambda p: float(np.dot((2.0, 4.0, 2.0), IR.reference_loss_inverse(*args, *Xs, *tg, p=p)[1]))
    h = 2.0 ** -8                      # exactly representable in float32 next to every P0 entry
    for k in range(7):
        pp, pm = np.array(IR.P0, dtype=np.float64), np.array(IR.P0, dtype=np.float64)
        base = float(np.float32(IR.P0[k]))
        pp[k], pm[k] = np.float32(base + h), np.float32(base - h)
        fd = (loss(pp) - loss(pm)) / (float(pp[k]) - float(pm[k]))
        print(IR.COLS[k], g[NP + k], fd)
        assert abs(g[NP + k] - fd) < 1e-5 * max(1.0, abs(fd)), (k, g[NP + k], fd)      # the loss is at most cubic in c: O(h^2)
    assert g[NP + 3] == 0.0 and np.abs(np.delete(g[NP:], 3)).min() > 1e-4
    # the network block is the coefficient reference's on the uniform table of the same operator
    import coef_reference as CR
    c = IR.coefficients()
    table = np.tile(c.astype(np.float32), (9, 1))
    g2, p2 = CR.reference_loss_coef(*args, *Xs, *tg, table)
    assert np.abs(g[:NP] - g2).max() < 1e-5 * max(1.0, np.abs(g2).max()) and np.abs(parts - p2).max() < 1e-6


def _errors(got, want_g, want_p, n, n_theta, hidden):
    """test_gpu_inverse._errors without its GPU imports: error / tolerance of the blocks, the operator block and the parts."""
    lay = pkg("hip.engine").param_layout(hidden, n, n_theta)
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    blocks = {"pre": slice(0, o_post), "theta": slice(o_th, NP), "post": slice(o_post, o_th), "operator": slice(NP, NP + 7)}
    out = {"parts": np.abs(got[NP + 7:] - want_p).max() / (TOL_L * max(1.0, np.abs(want_p).max()))}
    for name, s in blocks.items():
        out[name] = np.abs(got[s] - want_g[s]).max() / (TOL_G * max(1.0, np.abs(want_g[s]).max()))
    return out


@pytest.mark.parametrize("case,variant", [(c, v) for c, vs in IR.CONTROLS.items() for v in vs])
def test_negative_controls_of_the_gpu_cases_are_not_vacuous(case, variant):
    """Reference against reference under the GPU test's own measure: the true reference, taken as a result, must FAIL each
    control on the operator block, on the network gradient and on the loss parts (scale ignored: the loss parts move
    because c itself changes)."""
    ans, n, L, *_ = IR.CASES[case]
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    ref, bad = IR.case_reference(case), IR.case_reference(case, variant)
    err = _errors(np.concatenate([ref["grad"], ref["parts"]]), bad["grad"], bad["parts"], n, n_theta, IR.case_H(case))
    print(case, variant, {k: round(float(v), 1) for k, v in err.items()})
    assert err["operator"] > 1.0 and err["parts"] > 1.0 and max(err["pre"], err["theta"], err["post"]) > 1.0, err


def test_committed_operator_blocks():
    """The operator block of the two smallest merged cases as first computed (three digits); the frozen entry is exactly 0
    and an empty residual batch leaves an operator block that is exactly 0."""
    for case, want in (("reg_cascade4", (7.33, 0.020, 0.022, 0, 0.215, 3.28, 8.17)),
                       ("reg_cascade2", (1.97, 0.004, 0.035, 0, 0.042, 0.170, 1.18))):
        g = IR.case_reference(case)["grad"][-7:]
        print(case, g)
        assert g[3] == 0.0
        assert np.abs(np.abs(g) - np.array(want)).max() < 0.006, (case, g)
    assert (IR.case_reference("reg_cascade3_L2")["grad"][-7:] == 0.0).all()


def test_inverse_trainer_refuses_what_is_out_of_scope():
    from test_modules_cpu import Log, base_args
    tab = pkg("data.tabulated")
    IT_ = pkg("trainer.inverse_train").InverseTrainer
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    g = torch.Generator().manual_seed(0)
    Xr, Xi, Xb = (torch.rand(m, 3, generator=g) for m in (5, 3, 4))
    r, ui, ub = (torch.rand(m, generator=g) for m in (5, 3, 4))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        model = Solver(base_args(classic_network=[3, 16, 1]), Log(d), device=torch.device("cpu"))
        op = tab.LearnedOperator(learn={"c_x": 0.2})
        with pytest.raises(ValueError, match="operator="):
            IT_(model, 12, tab.TabulatedProblem(Xr, r, Xi, ui, Xb, ub, c_x=0.5), op)
        with pytest.raises(ValueError, match="operator="):
            IT_(model, 12, tab.TabulatedProblem(Xr, r, Xi, ui, Xb, ub, coef_res=torch.zeros(5, 7)), op)
        with pytest.raises(ValueError, match="LearnedOperator"):
            IT_(model, 12, tab.TabulatedProblem(Xr, r, Xi, ui, Xb, ub), None)


def test_fp64_identification_run_settles_at_the_true_coefficient():
    """The float64 replay of the GPU test's identification run (committed record: c_x every 100 steps, on the test's own
    float32 dataset and Philox batches) starts at 0.2 and stays within 0.02 of 0.8 over its last 1 000 steps.  The run is
    4 000 steps long: on these batches the replay is still 0.82 .. 0.84 over steps 1 000 .. 2 000 (inverse_training.py)."""
    c = IT.recovery_reference()["c_x"]
    print(c)
    assert c.shape == (IT.REC_STEPS // IT.REC_EVERY,) and c[0] == pytest.approx(IT.REC_START)
    late = c[IT.REC_SETTLED // IT.REC_EVERY:]
    assert IT.REC_STEPS - IT.REC_SETTLED == 1000 and len(late) == 10
    assert np.abs(late - IT.REC_TRUE).max() < 0.02, late
