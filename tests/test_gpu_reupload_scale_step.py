"""The fused step (qc_fused_pinn_residual_step) of a DVPDESolver with trainable input scalings (args["reupload_scale"])
against the float64 step reference of tests/reupload_scale_reference.py:

  - QC_PHASE_GRADS, [grad | L_r, L_bc, L_ic] at H = 50 with the cases and checks of tests/test_gpu_reupload_step.py: block
    by block at 2e-4 max(1, max |ref block|), loss parts at 1e-4; the theta block includes the scalings' slots, which are
    drawn as 1 + 0.4 randn.  The scalings' sub-block is also judged relative to its own size:
    error <= max(2e-4 max |ref sub-block|, 8 g), g the gap on that sub-block between the float64 reference and the same
    reference on a complex64 state (8: what the kernels do in fp32 beyond that restatement, the network stages and
    another summation order).  Control: the reference with every scaling 1 must fail every block.
  - one case behind a Fourier-feature map; the two-stream form is in use; n = 6 is refused by every step entry point.
  - six training steps at H = 16, n = 2, L = 2 follow the float64 replay that trains the scalings too; the replay with
    the scalings frozen at 1 does not.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fourier_reference as FR
import reupload_scale_reference as RS
from conftest import pkg
from step_reference import W3
from test_gpu_fullsize import Log, base_args, grads_for
from test_gpu_reupload_step import CASES, H, THETA_MIN, TOL_G, TOL_L, UNSUPPORTED, _stage_rc

pytestmark = pytest.mark.gpu

FOURIER_CASE = ("cascade", 4, 2, 8, 33, 10, 11)      # ansatz, n, L, m, B_res, n_ic, n_bc


def _model(dev, ans, n, L, H_, flat=None, Bf=None, **over):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    args = base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, classic_network=[3, H_, 1], reupload=True,
                     reupload_scale="wire", **over)
    model = Solver(args, Log(), device=dev)
    assert model.quantum_layer.has_embed_gates and tuple(model.quantum_layer.embed_scale.shape) == (L - 1, n)
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
    o_s = lay["quantum_layer.embed_scale"][0]
    assert o_s + lay["quantum_layer.embed_scale"][1][0] == NP == o_th + eng.n_theta
    return {"pre": slice(0, o_post), "theta": slice(o_th, NP), "post": slice(o_post, o_th), "scale": slice(o_s, NP)}


def _errors(eng, got, want):
    """block -> error / tolerance (< 1 passes); "scale" here under the blocks' common rule."""
    return {k: np.abs(got[s] - want[s]).max() / (TOL_G * max(1.0, np.abs(want[s]).max())) for k, s in _blocks(eng).items()}


def _check(eng, got, ref, ones, c64=None):
    err = _errors(eng, got[:-3], ref["grad"])
    print("error / tolerance by block:", err, "parts", got[-3:], ref["parts"])
    assert max(err.values()) < 1.0, err
    parts = ref["parts"]
    assert np.abs(got[-3:] - parts).max() < TOL_L * max(1.0, np.abs(parts).max()), (got[-3:], parts)
    s = _blocks(eng)["scale"]
    sub = ref["grad"][s]
    print("largest scale-block gradient of the reference:", np.abs(sub).max())
    assert np.abs(sub).max() > THETA_MIN
    assert np.abs(ref["grad"][_blocks(eng)["theta"]]).max() > THETA_MIN
    if c64 is not None:      # the scalings' sub-block relative to its own size
        g = np.abs(c64["grad"][s] - sub).max()
        bound = max(TOL_G * np.abs(sub).max(), 8 * g)
        e = np.abs(got[:-3][s] - sub).max()
        print(f"scale sub-block: fp32-fp64 gap of the restatement g = {g:.3e}, bound = {bound:.3e}, kernel error = {e:.3e}")
        assert e <= bound, (e, bound, g)
    bad = _errors(eng, got[:-3], ones["grad"])
    print("control (every scaling 1), error / tolerance by block:", bad)
    assert min(bad.values()) > 1.0, bad


@pytest.mark.parametrize("case", list(CASES))
def test_fused_step_matches_fp64(case, gpu_device):
    ans, n, L, B_res, n_ic, n_bc = CASES[case]
    _, flat, X_ic, X_bc, X_res = RS.step_case_inputs(ans, n, L, H, B_res, n_ic, n_bc)
    rec = {v: RS.step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, H, variant=v) for v in ("", "ones", "c64")}
    model, eng = _model(gpu_device, ans, n, L, H, flat)
    assert eng.NP == flat.size and eng.n_theta == L * pkg("circuits").params_per_layer(ans, n) + (L - 1) * n
    assert np.array_equal(model.quantum_layer.embed_scale.detach().cpu().numpy().reshape(-1), flat[-(L - 1) * n:])
    got = grads_for(model, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    _check(eng, got, rec[""], rec["ones"], rec["c64"])
    # the form: two streams, the merged stages are refused
    assert _stage_rc(eng, B_res, n_ic, n_bc) == UNSUPPORTED


def test_fused_step_behind_a_fourier_map_matches_fp64(gpu_device):
    ans, n, L, m, B_res, n_ic, n_bc = FOURIER_CASE
    Bf, flat, X_ic, X_bc, X_res = RS.step_case_inputs(ans, n, L, H, B_res, n_ic, n_bc, m=m)
    rec = {v: RS.step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, H, variant=v, Bf=Bf) for v in ("", "ones")}
    model, eng = _model(gpu_device, ans, n, L, H, flat, Bf, fourier_features=m, fourier_scale=2.0)
    assert eng.NP == flat.size and eng.circuit.ff_m == m
    got = grads_for(model, *(torch.from_numpy(x) for x in (X_ic, X_bc, X_res))).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    _check(eng, got, rec[""], rec["ones"])


def test_fused_step_refuses_six_qubits(gpu_device):
    """A scaled program at n = 6 has no kernel family: every step entry point returns QC_ERR_UNSUPPORTED and nothing runs
    (DVQuantumLayer refuses to build one, so program and parameter are put in by hand)."""
    circuits, engine, Lb = pkg("circuits"), pkg("hip.engine"), pkg("hip.lib")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    ans, n = "cascade", 6
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=2, q_ansatz=ans, classic_network=[3, 8, 1]), Log(), device=gpu_device)
    ql = model.quantum_layer
    ql.program = circuits.build_program(ans, n, 2, ql.haar_seed1 is not None, reupload=True, reupload_scale="wire")
    ql.embed_scale = torch.nn.Parameter(torch.ones(1, n))
    ql._circuits = {}
    eng = model._engine_for(gpu_device)
    assert eng.n_theta == ql.program.n_params and eng.circuit.n_scale == n
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


def _replay(flat, H_, n, n_theta, builder, batches, lr, ns, frozen):
    """Loss history of float64 training on ``batches``: the reference gradient, clip to norm 1, Adam; ``frozen``: the
    scalings stay at 1 (their gradient is dropped before the clip)."""
    prm, mom, var, hist = np.asarray(flat, np.float64), None, None, []
    for k, (X_ic, X_bc, X_res) in enumerate(batches):
        g, parts = RS.step_reference(prm, H_, n, n_theta, builder, None, X_ic, X_bc, X_res)
        if frozen:
            g[-ns:] = 0.0
        hist.append(float(np.dot(W3, parts)))
        prm, mom, var = FR.adam_step(prm, g, lr, m=mom, v=var, step=k + 1)
    return np.array(hist), prm


def test_training_replay(gpu_device):
    from oracle import solver as osol
    trainer = pkg("trainer.diffusion_train")
    ans, n, L, H_, steps = "cascade", 2, 2, 16, 6
    ns = (L - 1) * n
    model, eng = _model(gpu_device, ans, n, L, H_, epochs=steps - 1)
    flat0 = eng.flat.detach().cpu().numpy().copy()
    assert np.array_equal(flat0[-ns:], np.ones(ns, np.float32))
    torch.manual_seed(5)
    batches = [tuple(osol.sample_box(b, k) for b, k in ((osol.BOX_IC, 21), (osol.BOX_BC1, 21), (osol.BOX_DOM, 64)))
               for _ in range(steps)]
    trainer.train(model, batch_size=64, batches=batches)
    got = np.array(model.loss_history[:steps])
    np_batches = [tuple(x.numpy() for x in b) for b in batches]
    build = RS.whole_circuit(ans, n, L, "wire")
    want, prm = _replay(flat0, H_, n, eng.n_theta, build, np_batches, model.args["lr"], ns, False)
    tol = 1e-4 * np.maximum(1.0, np.abs(want))
    print("loss history", got, want, "error / tolerance", np.abs(got - want) / tol)
    assert (np.abs(got - want) < tol).all(), (got, want)
    # the replay with the scalings frozen at 1 does not follow
    frozen, _ = _replay(flat0, H_, n, eng.n_theta, build, np_batches, model.args["lr"], ns, True)
    print("frozen replay", frozen, "distance / tolerance", np.abs(got - frozen) / tol)
    assert not (np.abs(got - frozen) < tol).all(), (got, frozen)
    # the scalings were trained
    s = model.quantum_layer.embed_scale.detach().cpu().numpy().reshape(-1)
    print("embed_scale after the run", s, "replay", prm[-ns:])
    assert np.isfinite(s).all() and (np.abs(s - 1.0) > 1e-3).all()
