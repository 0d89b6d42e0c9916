"""L-BFGS as the second training phase on the GPU: ``LbfgsTrainer`` behind Adam steps of a ``FusedTrainer`` against the float64
replay (tests/lbfgs_training.py), ``qc_lbfgs_step`` behind the inverse step at the C ABI, ``train(..., lbfgs=)`` on a small
tabulated problem, and Adam -> L-BFGS against Adam alone.  Tolerances are the project's existing ones for a fused run against
its float64 reference: accept flags equal, per-evaluation loss 1e-4 relative, final x_k 2e-3."""
import ctypes as C

import numpy as np
import pytest
import torch

import lbfgs_training as LT
from conftest import pkg
from test_gpu_fullsize import Log, base_args

pytestmark = pytest.mark.gpu


def _trainer(gpu_device, case, capacity):
    ans, n, L, *_ = LT.case_shape(case)
    flat, X_ic, X_bc, X_res = LT.case_inputs(case)
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, classic_network=[3, LT.H, 1]), Log(),
                   device=gpu_device)
    tr = pkg("trainer.diffusion_train").FusedTrainer(model, LT.B_RES, capacity=capacity)
    with torch.no_grad():
        tr.eng.flat.copy_(torch.from_numpy(flat))
    tr.eng.refresh_gates()
    tr.load_batches(X_ic, X_bc, X_res)
    return model, tr


@pytest.mark.parametrize("case", list(LT.CASES))
def test_adam_then_lbfgs_replays_float64(case, gpu_device):
    """5 Adam steps, then the case's L-BFGS evaluations (14 with m = 4 for cascade n = 4; 6 for layered n = 6, the wave
    family) on one explicit batch of 64 + 21 + 21 points."""
    T = pkg("trainer.lbfgs_train")
    evals, m = LT.case_shape(case)[5:7]
    ref = LT.training_reference(case)
    model, tr = _trainer(gpu_device, case, LT.ADAM)
    for _ in range(LT.ADAM):
        tr.step()
    adam = np.array(tr.opt.loss_history())
    assert np.abs(adam - ref["adam_loss"]).max() <= 1e-4 * max(1.0, np.abs(ref["adam_loss"]).max())
    lb = T.LbfgsTrainer(tr, history=m, capacity=evals)
    for _ in range(evals):
        lb.step()
    rows = lb.history()
    print(case, "loss", rows[:, 0], "want", ref["loss"], "accepted", rows[:, 2])
    assert rows.shape == (evals, 3)
    assert np.array_equal(rows[:, 2], ref["accepted"].astype(np.float32))
    assert (ref["accepted"] == 0).any()                     # the replay rejects a trial: the line search was exercised
    assert np.abs(rows[:, 0] - ref["loss"]).max() <= 1e-4 * max(1.0, np.abs(ref["loss"]).max())
    assert np.allclose(rows[:, 1], ref["t_led"], rtol=1e-3, atol=0)
    rec = lb.state()
    assert rec["n_eval"] == evals and rec["n_pairs"] == int(ref["n_pairs"][0])
    pending = tr.eng.flat.detach().cpu().numpy().copy()
    lb.finish()
    x_k = tr.eng.flat.detach().cpu().numpy()
    assert np.abs(x_k - ref["x_k"]).max() <= 2e-3 * max(1.0, np.abs(ref["x_k"]).max())
    assert np.abs(pending - x_k).max() > 0.0                # without finish() the model sat at a pending trial


def test_lbfgs_step_behind_the_inverse_step(gpu_device):
    """InverseStep (QC_PHASE_GRADS) + qc_lbfgs_step at the C ABI over its NP + 7 entries, 6 evaluations: accepted losses
    decrease, the seven trailing entries move, and the flat vector at the last accepted point matches
    tests/inverse_reference.py evaluated there, at that file's own tolerance (test_gpu_inverse._errors < 1)."""
    import inverse_reference as IR
    import test_gpu_inverse as TI
    from step_reference import haar_for
    from test_gpu_tabulated import _model
    L, E = pkg("hip.lib"), pkg("hip.engine")
    case = "reg_cascade4"
    ans, n, Lq, enc, B_res, n_ic, n_bc = IR.CASES[case]
    flat, *batch = IR.case_inputs(case)
    model, eng = _model(gpu_device, ans, n, Lq, enc, flat, IR.case_H(case))
    fs = TI._inverse_step(eng, B_res, n_ic, n_bc)
    TI._load(fs, *batch)
    st = E.LbfgsState(fs.NP_L, gpu_device, history=4, capacity=6)
    p0 = fs.flat.cpu().numpy().copy()
    for _ in range(6):
        fs.run(L.QC_PHASE_GRADS)
        st.advance(fs.flat_grad, fs.flat, fs.circuit, fs.theta_off)
    rows, rec = st.history(), st.read()
    acc = [float(f) for f, _, a in rows if a > 0.5]
    print("inverse step + L-BFGS: losses", rows[:, 0], "accepted", rows[:, 2])
    assert len(acc) >= 3 and all(b < a for a, b in zip(acc, acc[1:]))
    x_k = st.x_k().cpu().numpy().copy()
    assert (np.abs(x_k[-IR.N_OP:] - p0[-IR.N_OP:])[np.array(IR.SCALE) != 0] > 1e-6).all()     # the live operator entries moved
    assert (x_k[-IR.N_OP:][np.array(IR.SCALE) == 0] == p0[-IR.N_OP:][np.array(IR.SCALE) == 0]).all()   # zero gradient: frozen
    # the gradient phase at the last accepted point against the float64 reference at that point
    with torch.no_grad():
        fs.flat.copy_(st.x_k())
    fs.refresh_gates()
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    got = fs.flat_grad.cpu().numpy().astype(np.float64)
    P = int(pkg("circuits").params_per_layer(ans, n))
    X_ic, X_bc, X_res, u_ic, u_bc, r_res = batch
    g, parts = IR.reference_loss_inverse(x_k[:fs.NP], IR.case_H(case), n, Lq * P, (Lq, P), ans, haar_for(n, 1),
                                         *(torch.as_tensor(x).double() for x in (X_ic, X_bc, X_res)), u_ic, u_bc, r_res,
                                         p=x_k[fs.NP:], encoding=enc)
    err = TI._errors(got, g, parts, n, eng.n_theta)
    print({k: round(float(v), 3) for k, v in err.items()})
    assert max(err.values()) < 1.0, err
    assert abs(float(np.dot((2.0, 4.0, 2.0), parts)) - rec["f0"]) <= 1e-4 * max(1.0, rec["f0"])


def _tab_model(gpu_device, tmp_path, epochs):
    import tabulated_reference as TR
    import tabulated_training as TT
    TP = pkg("data.tabulated").TabulatedProblem
    Solver = pkg("nn.DVPDESolver").DVPDESolver

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    args = TT.base_args("cascade", 4)
    args.update(epochs=epochs, classic_network=[3, 16, 1])
    torch.manual_seed(1)
    model = Solver(args, TmpLog(), device=gpu_device)
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in TT.dataset_arrays())
    co = dict(zip(("c_t", "c_x", "c_y", "d_xx", "d_yy"), TR.COEFFS), c_u=TR.C_U)
    return model, TP(Xr, rr, Xi, ui, Xb, ub, **co), Solver


def test_train_with_an_lbfgs_phase(gpu_device, tmp_path):
    """train(model, ..., lbfgs=LbfgsPhase(evals=30)) on a small TabulatedProblem: the history grows by the accepted
    iterations, the model ends at an accepted point (its loss, recomputed with a GRADS-only call on the phase's batch,
    equals the last accepted history entry to 1e-6 relative), and save_state / load_state round-trips."""
    import os
    L = pkg("hip.lib")
    trainer, T = pkg("trainer.diffusion_train"), pkg("trainer.lbfgs_train")
    model, ds, Solver = _tab_model(gpu_device, tmp_path, epochs=9)
    torch.manual_seed(5)
    trainer.train(model, batch_size=64, dataset=ds, lbfgs=T.LbfgsPhase(evals=30, history=5))
    tr = model._sync_fused_to_torch.__self__                # the FusedTrainer of that call; its L-BFGS phase: tr.lbfgs
    n_adam = 10
    lb_hist = model.loss_history[n_adam:]
    rec = tr.lbfgs.state()
    assert rec["n_eval"] == 30 and len(lb_hist) == rec["n_iter"] > 3
    assert all(b < a for a, b in zip(lb_hist, lb_hist[1:]))
    assert abs(lb_hist[-1] - rec["f0"]) <= 1e-6 * max(1.0, abs(rec["f0"]))
    # the batch of the phase is still resident: the loss at the model's parameters
    tr.fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    parts = tr.fs.flat_grad[-3:].cpu().numpy().astype(np.float64)
    f_now = float(np.dot((2.0, 4.0, 2.0), parts))
    assert abs(f_now - lb_hist[-1]) <= 1e-6 * max(1.0, abs(lb_hist[-1])), (f_now, lb_hist[-1])
    w = model._flat.detach().cpu().clone()
    model.save_state()
    state = Solver.load_state(os.path.join(model.log_path, "model.pth"))
    back = torch.cat([v.reshape(-1).cpu() for part in ("preprocessor", "postprocessor") for v in state[part].values()] +
                     [state["quantum_layer"]["params"].reshape(-1).cpu()])
    assert back.numel() == w.numel() and torch.equal(back, w)          # the saved weights are the accepted point
    assert np.allclose(state["loss_history"], model.loss_history)


def test_without_finish_the_model_sits_at_a_pending_trial(gpu_device, tmp_path):
    trainer, T = pkg("trainer.diffusion_train"), pkg("trainer.lbfgs_train")
    model, ds, _ = _tab_model(gpu_device, tmp_path, epochs=0)
    torch.manual_seed(5)
    tr = trainer.FusedTrainer(model, 64, capacity=1, dataset=ds)
    lb = T.LbfgsTrainer(tr, history=5, capacity=8)
    lb.new_batch()
    for _ in range(8):
        lb.step()
    pending = tr.eng.flat.detach().cpu().clone()
    lb.finish()
    assert not torch.equal(pending, tr.eng.flat.detach().cpu())
    assert torch.equal(tr.eng.flat.detach().cpu(), lb.state_dev.x_k().cpu())


def test_adam_then_lbfgs_beats_adam_alone(gpu_device):
    """The same seeded model on the same fixed batch after the same 200 Adam steps: 100 L-BFGS evaluations must reach a
    lower loss than 100 more Adam steps.  The float64 replay (committed record) shows a factor >= 2 between the two."""
    L = pkg("hip.lib")
    T = pkg("trainer.lbfgs_train")
    ref = LT.usefulness_reference()
    assert float(ref["f_adam"][0]) >= 2.0 * float(ref["f_lbfgs"][0])

    def loss_at(tr):
        tr.fs.run(L.QC_PHASE_GRADS)
        torch.cuda.synchronize()
        return float(np.dot((2.0, 4.0, 2.0), tr.fs.flat_grad[-3:].cpu().numpy().astype(np.float64)))

    model, tr = _trainer(gpu_device, LT.USE_CASE, LT.USE_ADAM + LT.USE_MORE)
    for _ in range(LT.USE_ADAM + LT.USE_MORE):
        tr.step()
    f_adam = loss_at(tr)
    model, tr = _trainer(gpu_device, LT.USE_CASE, LT.USE_ADAM)
    for _ in range(LT.USE_ADAM):
        tr.step()
    lb = T.LbfgsTrainer(tr, history=LT.USE_M, capacity=LT.USE_MORE)
    for _ in range(LT.USE_MORE):
        lb.step()
    lb.finish()
    f_lbfgs = loss_at(tr)
    print("Adam alone %.4e, Adam -> L-BFGS %.4e (float64 replay: %.4e, %.4e)" % (f_adam, f_lbfgs, ref["f_adam"][0], ref["f_lbfgs"][0]))
    assert f_lbfgs < f_adam
