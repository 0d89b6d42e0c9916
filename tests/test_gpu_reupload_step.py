"""The fused step (qc_fused_pinn_residual_step) of a re-uploaded DVPDESolver (args["reupload"]) against the float64 step
reference of tests/reupload_reference.py:

  - QC_PHASE_GRADS, [grad | L_r, L_bc, L_ic] at H = 50 with the checks of tests/test_gpu_fused_families.py: block by block
    at 2e-4 max(1, max |ref block|), loss parts at 1e-4, the theta block of the reference above THETA_MIN.  One case behind
    a Fourier-feature map (fourier_features = 8).  Controls that must fail: the plain circuit's reference, the reference
    without the last residual point.
  - the step takes the two-stream form: qc_fused_step_stage (merged form only) is refused.
  - six training steps at H = 16, n = 2, L = 2 follow the float64 replay to 1e-4 max(1, |want|).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fourier_reference as FR
import reupload_reference as RR
from conftest import pkg
from step_reference import W3, step_inputs
from test_gpu_fullsize import Log, base_args, grads_for

pytestmark = pytest.mark.gpu

H = 50
TOL_G, TOL_L = 2e-4, 1e-4            # tests/test_gpu_fused_families.py
THETA_MIN = 20 * TOL_G
UNSUPPORTED = -2

# id -> (ansatz, n, L, B_res, n_ic, n_bc)
CASES = {"cascade4_L2": ("cascade", 4, 2, 70, 30, 20), "layered3_L3": ("layered", 3, 3, 33, 0, 17),
         "alternate5_L2": ("alternate", 5, 2, 20, 25, 0), "cascade2_L2": ("cascade", 2, 2, 0, 70, 75)}
# negative controls: the plain circuit's reference must fail EVERY block of every case, the reference without the last
# residual point at least one (a lost point moves every block by about 1 / B_res of itself)
CONTROLS = {"cascade4_L2": ("plain", "drop_res"), "layered3_L3": ("plain", "drop_res"), "alternate5_L2": ("plain", "drop_res"),
            "cascade2_L2": ("plain",)}


def _model(dev, ans, n, L, H_, flat=None, Bf=None, **over):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    args = base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, classic_network=[3, H_, 1], reupload=True, **over)
    model = Solver(args, Log(), device=dev)
    assert model.quantum_layer.has_embed_gates
    if Bf is not None:
        with torch.no_grad():
            model.fourier.B.copy_(torch.from_numpy(np.asarray(Bf, np.float32)))
    eng = model._engine_for(dev)
    if flat is not None:
        with torch.no_grad():
            eng.flat.copy_(torch.from_numpy(np.asarray(flat, np.float32)))
    return model, eng


def _blocks(eng):
    lay = eng.layout
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    return {"pre": slice(0, o_post), "theta": slice(o_th, NP), "post": slice(o_post, o_th)}


def _errors(eng, got, want):
    """block -> error / tolerance (< 1 passes)."""
    return {k: np.abs(got[s] - want[s]).max() / (TOL_G * max(1.0, np.abs(want[s]).max())) for k, s in _blocks(eng).items()}


def _check(eng, got, ref):
    err = _errors(eng, got[:-3], ref["grad"])
    print("error / tolerance by block:", err, "parts", got[-3:], ref["parts"])
    assert max(err.values()) < 1.0, err
    parts = ref["parts"]
    assert np.abs(got[-3:] - parts).max() < TOL_L * max(1.0, np.abs(parts).max()), (got[-3:], parts)
    assert np.abs(ref["grad"][_blocks(eng)["theta"]]).max() > THETA_MIN


def _stage_rc(eng, B_res, n_ic, n_bc):
    engine, L = pkg("hip.engine"), pkg("hip.lib")
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, eng.device))
    rc = eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_PRE_FWD, torch.cuda.current_stream(eng.device).cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", list(CASES))
def test_fused_step_matches_fp64(case, gpu_device):
    ans, n, L, B_res, n_ic, n_bc = CASES[case]
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=1)
    ref = RR.step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, H)
    model, eng = _model(gpu_device, ans, n, L, H, flat)
    assert eng.NP == flat.size and eng.n_theta == n_theta
    got = grads_for(model, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    _check(eng, got, ref)
    # the form: two streams, the merged stages are refused
    assert _stage_rc(eng, B_res, n_ic, n_bc) == UNSUPPORTED
    for v in CONTROLS.get(case, ()):
        bad = _errors(eng, got[:-3], RR.step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, H, variant=v)["grad"])
        print("control", v, bad)
        assert (min if v == "plain" else max)(bad.values()) > 1.0, (v, bad)


def test_fused_step_behind_a_fourier_map_matches_fp64(gpu_device):
    ans, n, L, m, scale, B_res, n_ic, n_bc = "cascade", 4, 2, 8, 2.0, 33, 10, 11
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    Bf, flat, X_ic, X_bc, X_res = FR.step_inputs(H, n, n_theta, m, scale, B_res, n_ic, n_bc, salt=3)
    ref = RR.step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, H, Bf=Bf)
    model, eng = _model(gpu_device, ans, n, L, H, flat, Bf, fourier_features=m, fourier_scale=scale)
    assert eng.NP == flat.size and eng.circuit.ff_m == m
    got = grads_for(model, *(torch.from_numpy(x) for x in (X_ic, X_bc, X_res))).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    _check(eng, got, ref)
    bad = _errors(eng, got[:-3], RR.step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, H, variant="plain", Bf=Bf)["grad"])
    assert min(bad.values()) > 1.0, bad


@pytest.mark.parametrize("ans,n", [("cascade", 6), ("farhi", 1)])
def test_fused_step_refuses_other_qubit_counts(ans, n, gpu_device):
    """A program with EMBED gates outside 2 <= n <= 5 has no kernel family: the step entry point returns
    QC_ERR_UNSUPPORTED (DVQuantumLayer refuses to build one, so the program is put in by hand)."""
    circuits, engine, Lb = pkg("circuits"), pkg("hip.engine"), pkg("hip.lib")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=2, q_ansatz=ans, classic_network=[3, 8, 1]), Log(), device=gpu_device)
    ql = model.quantum_layer
    ql.program = circuits.build_program(ans, n, 2, ql.haar_seed1 is not None, reupload=True)
    assert any(g.op == circuits.OP_EMBED for g in ql.program.gates)
    eng = model._engine_for(gpu_device)
    eng.refresh_gates()
    fs = engine.FusedStep(eng, 10, 5, 6, engine.OptimState(eng.NP, 0.005, gpu_device))
    fs.flat_grad.fill_(7.0)
    name, fn, args = fs._entry
    assert name == "qc_fused_pinn_residual_step"
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    for phases in (Lb.QC_PHASE_GRADS, Lb.QC_PHASE_GRADS | Lb.QC_PHASE_UPDATE):
        assert fn(*args, phases, st) == UNSUPPORTED
    assert eng.lib.qc_fused_step_stage(C.byref(fs.desc), Lb.QC_STAGE_PRE_FWD, st) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((fs.flat_grad == 7.0).all())           # nothing ran


def _replay(flat, H_, n, n_theta, theta_shape, ans, batches, lr, reupload):
    """Loss history of float64 training on ``batches``: the reference gradient, clip to norm 1, Adam."""
    prm, mom, var, hist = np.asarray(flat, np.float64), None, None, []
    for k, (X_ic, X_bc, X_res) in enumerate(batches):
        g, parts = RR.step_reference(prm, H_, n, n_theta, theta_shape, ans, None, X_ic, X_bc, X_res, reupload=reupload)
        hist.append(float(np.dot(W3, parts)))
        prm, mom, var = FR.adam_step(prm, g, lr, m=mom, v=var, step=k + 1)
    return np.array(hist)


def test_training_replay(gpu_device):
    from oracle import solver as osol
    trainer = pkg("trainer.diffusion_train")
    ans, n, L, H_, steps = "cascade", 2, 2, 16, 6
    model, eng = _model(gpu_device, ans, n, L, H_, epochs=steps - 1)
    flat0 = eng.flat.detach().cpu().numpy().copy()
    torch.manual_seed(5)
    batches = [tuple(osol.sample_box(b, k) for b, k in ((osol.BOX_IC, 21), (osol.BOX_BC1, 21), (osol.BOX_DOM, 64)))
               for _ in range(steps)]
    trainer.train(model, batch_size=64, batches=batches)
    got = np.array(model.loss_history[:steps])
    theta_shape = tuple(model.quantum_layer.params.shape)
    np_batches = [tuple(x.numpy() for x in b) for b in batches]
    want = _replay(flat0, H_, n, eng.n_theta, theta_shape, ans, np_batches, model.args["lr"], True)
    tol = 1e-4 * np.maximum(1.0, np.abs(want))
    print("loss history", got, want, "error / tolerance", np.abs(got - want) / tol)
    assert (np.abs(got - want) < tol).all(), (got, want)
    # the replay of the plain circuit does not follow
    plain = _replay(flat0, H_, n, eng.n_theta, theta_shape, ans, np_batches, model.args["lr"], False)
    assert (np.abs(got - plain) > tol).all(), (got, plain)
