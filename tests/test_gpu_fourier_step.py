"""The fused step of a DVPDESolver behind a Fourier-feature input map (args["fourier_features"]) against the float64
reference of tests/fourier_reference.py (the map, the pre network and the post network restated in torch, the circuit from
the oracle, the gradient by autograd):

  - QC_PHASE_GRADS, [grad | L_r, L_bc, L_ic]: cascade n = 4, H = 5, m = 3, scale 2 on 65 + 21 + 22 points (the merged form
    with tail tiles in both pipelines; the two-stream form under QC_NO_MERGE=1 in a child process), and layered n = 6 on
    64 + 21 + 21 points (the lanes family, always two streams).  Tolerances: those of tests/test_gpu_fused_families.py,
    block by block.  Control: the reference without the last frequency must fail them.
  - QC_PHASE_SAMPLE: the batches drawn in the step's first stage are bit-identical to the plain step's.
  - six training steps at H = 16, m = 8 against the float64 replay (1e-4 max(1, |want|)); the replay of the plain network on
    the first three columns must miss by 100 tolerances.
  - the tabulated step (FusedTrainer(dataset=)): the map does not depend on the target kind.
  - H = 50, m = 32 (NP + 3 > 3072: the two-launch optimiser tail): GRADS | UPDATE in one call against float64 Adam.
  - the module: forward with requires_grad inputs under nn.pde.diffusion_operator, residual() and jets() at B = 5.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fourier_reference as FR
import mlp_reference as R
import step_reference as S
from conftest import pkg
from test_gpu_fullsize import Log, base_args, grads_for

pytestmark = pytest.mark.gpu

TOL_G, TOL_L = 2e-4, 1e-4            # tests/test_gpu_fused_families.py
ADAM_FAST_MAX = 3072

# id -> (ansatz, n, H, m, scale, B_res, n_ic, n_bc)
CASES = {"reg_cascade4": ("cascade", 4, 5, 3, 2.0, 65, 21, 22), "wave_layered6": ("layered", 6, 5, 3, 2.0, 64, 21, 21)}


def _model(dev, ans, n, H, m, scale, flat=None, Bf=None, **over):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    args = base_args(num_qubits=n, q_ansatz=ans, classic_network=[3, H, 1], **over)
    if m:
        args.update(fourier_features=m, fourier_scale=scale)
    model = Solver(args, Log(), device=dev)
    if Bf is not None:
        with torch.no_grad():
            model.fourier.B.copy_(torch.from_numpy(np.asarray(Bf, np.float32)))
    eng = model._engine_for(dev)
    if flat is not None:
        with torch.no_grad():
            eng.flat.copy_(torch.from_numpy(np.asarray(flat, np.float32)))
    return model, eng


def _oracle_args(model):
    from oracle import statevector as sv
    ql = model.quantum_layer
    haar = sv.haar_pair(ql.haar_seed1, ql.haar_seed2) if model.num_qubits >= 4 else None
    return tuple(ql.params.shape), haar


def _blocks(eng):
    lay = eng.layout
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    return {"pre": slice(0, o_post), "theta": slice(o_th, NP), "post": slice(o_post, o_th)}


def _errors(eng, got, want):
    return {k: np.abs(got[s] - want[s]).max() / (TOL_G * max(1.0, np.abs(want[s]).max())) for k, s in _blocks(eng).items()}


@pytest.mark.parametrize("case", list(CASES))
def test_fused_step_matches_fp64(case, gpu_device):
    ans, n, H, m, scale, B_res, n_ic, n_bc = CASES[case]
    P = pkg("circuits").params_per_layer(ans, n)
    Bf, flat, X_ic, X_bc, X_res = FR.step_inputs(H, n, P, m, scale, B_res, n_ic, n_bc, salt=1)
    model, eng = _model(gpu_device, ans, n, H, m, scale, flat, Bf)
    assert eng.NP == flat.size and eng.circuit.ff_m == m
    got = grads_for(model, *(torch.from_numpy(x) for x in (X_ic, X_bc, X_res))).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    theta_shape, haar = _oracle_args(model)
    want_g, want_p = FR.reference_loss(flat, H, n, P, theta_shape, ans, haar, Bf, X_ic, X_bc, X_res)
    err = _errors(eng, got[:-3], want_g)
    print(case, "error / tolerance by block:", err, "parts", got[-3:], want_p)
    assert max(err.values()) < 1.0, err
    assert np.abs(got[-3:] - want_p).max() < TOL_L * max(1.0, np.abs(want_p).max()), (got[-3:], want_p)
    assert np.abs(want_g[_blocks(eng)["theta"]]).max() > 20 * TOL_G
    # the form the step took
    engine, L = pkg("hip.engine"), pkg("hip.lib")
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, gpu_device))
    rc = eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_PRE_FWD, torch.cuda.current_stream(gpu_device).cuda_stream)
    torch.cuda.synchronize()
    assert (rc == 0) == (2 <= n <= 5 and os.environ.get("QC_NO_MERGE") != "1")
    # control: a lost frequency fails the same tolerance in the pre-network block
    bad_g, _ = FR.reference_loss(flat, H, n, P, theta_shape, ans, haar, Bf, X_ic, X_bc, X_res, drop_freq=True)
    assert _errors(eng, got[:-3], bad_g)["pre"] > 1.0


def test_two_stream_form_passes_the_same_check():
    """QC_NO_MERGE is read once at library load, hence a child process."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "matches_fp64 and reg_cascade4"], env=dict(os.environ, QC_NO_MERGE="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]


def test_sampled_batches_are_the_plain_steps(gpu_device):
    """QC_PHASE_SAMPLE | QC_PHASE_GRADS: the merged first stage draws the points itself, with the plain stage's counters."""
    engine, L = pkg("hip.engine"), pkg("hip.lib")
    out = []
    for m in (0, 3):
        model, eng = _model(gpu_device, "cascade", 4, 5, m, 2.0)
        eng.refresh_gates()
        fs = engine.FusedStep(eng, 130, 21, 45, engine.OptimState(eng.NP, 0.005, gpu_device))
        fs.set_sampler(1234567, 64, 7, 11)
        fs.desc.sample_step = 4
        fs.X_res.fill_(float("nan"))
        fs.X_val.fill_(float("nan"))
        fs.run(L.QC_PHASE_SAMPLE | L.QC_PHASE_GRADS)
        torch.cuda.synchronize()
        assert torch.isfinite(fs.flat_grad).all()
        out.append((fs.X_res.cpu().numpy().copy(), fs.X_val.cpu().numpy().copy()))
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def _replay(flat, H, n, P, theta_shape, ans, haar, Bf, batches, lr):
    """Loss history of float64 training on ``batches``: the reference gradient, clip to norm 1, Adam."""
    prm, mom, var, hist = np.asarray(flat, np.float64), None, None, []
    for k, (X_ic, X_bc, X_res) in enumerate(batches):
        g, parts = FR.reference_loss(prm, H, n, P, theta_shape, ans, haar, Bf, X_ic, X_bc, X_res)
        hist.append(float(np.dot(S.W3, parts)))
        prm, mom, var = FR.adam_step(prm, g, lr, m=mom, v=var, step=k + 1)
    return np.array(hist)


def test_training_replay(gpu_device):
    from oracle import solver as osol
    trainer = pkg("trainer.diffusion_train")
    ans, n, H, m, scale, steps = "cascade", 4, 16, 8, 1.0, 6
    model, eng = _model(gpu_device, ans, n, H, m, scale, epochs=steps - 1)
    P = eng.n_theta
    flat0 = eng.flat.detach().cpu().numpy().copy()
    Bf = model.fourier.B.detach().cpu().numpy().copy()
    torch.manual_seed(5)
    batches = [tuple(osol.sample_box(b, k) for b, k in ((osol.BOX_IC, 21), (osol.BOX_BC1, 21), (osol.BOX_DOM, 64)))
               for _ in range(steps)]
    trainer.train(model, batch_size=64, batches=batches)
    got = np.array(model.loss_history[:steps])
    theta_shape, haar = _oracle_args(model)
    np_batches = [tuple(x.numpy() for x in b) for b in batches]
    want = _replay(flat0, H, n, P, theta_shape, ans, haar, Bf, np_batches, model.args["lr"])
    tol = 1e-4 * np.maximum(1.0, np.abs(want))
    print("loss history", got, want, "error / tolerance", np.abs(got - want) / tol)
    assert (np.abs(got - want) < tol).all(), (got, want)
    # the same replay with the map removed: the plain pre network on the first three columns of W1
    lay, _ = FR.layout(H, n, P, 2 * m)
    W1 = flat0[:H * 2 * m].reshape(H, 2 * m)[:, :3].reshape(-1)
    plain = _replay(np.concatenate([W1, flat0[lay["b1"][0]:]]), H, n, P, theta_shape, ans, haar, None, np_batches, model.args["lr"])
    assert (np.abs(got - plain) > 100 * tol).all(), (got, plain)


def test_tabulated_step_reads_the_map(gpu_device):
    trainer = pkg("trainer.diffusion_train")
    tab = pkg("data.tabulated")
    ans, n, H, m, scale, B_res, n_ic, n_bc = CASES["reg_cascade4"]
    B_res, n_ic, n_bc = 66, 22, 22
    P = pkg("circuits").params_per_layer(ans, n)
    Bf, flat, X_ic, X_bc, X_res = FR.step_inputs(H, n, P, m, scale, B_res, n_ic, n_bc, salt=2)
    rng = np.random.default_rng(3)
    r, u_bc, u_ic = (rng.standard_normal(k).astype(np.float32) for k in (B_res, n_bc, n_ic))
    model, eng = _model(gpu_device, ans, n, H, m, scale, flat, Bf)
    t = torch.from_numpy
    ds = tab.TabulatedProblem(t(X_res), t(r), t(X_ic), t(u_ic), t(X_bc), t(u_bc))
    tr = trainer.FusedTrainer(model, B_res, capacity=2, dataset=ds)
    assert (tr.B_res, tr.n_ic, tr.n_bc) == (B_res, n_ic, n_bc)
    tr.load_batches(t(X_ic), t(X_bc), t(X_res), targets=(u_ic, u_bc, r))
    tr.fs.run(pkg("hip.lib").QC_PHASE_GRADS)
    torch.cuda.synchronize()
    got = tr.fs.flat_grad.cpu().numpy().astype(np.float64)
    theta_shape, haar = _oracle_args(model)
    want_g, want_p = FR.reference_loss(flat, H, n, P, theta_shape, ans, haar, Bf, X_ic, X_bc, X_res, targets=(r, u_bc, u_ic))
    err = _errors(eng, got[:-3], want_g)
    assert max(err.values()) < 1.0, err
    assert np.abs(got[-3:] - want_p).max() < TOL_L * max(1.0, np.abs(want_p).max()), (got[-3:], want_p)


def test_large_layout_takes_the_two_launch_tail(gpu_device):
    """H = 50, m = 32: NP + 3 > 3072, so GRADS | UPDATE in one call ends in the row reduction and k_adam.  The parameters
    after it against float64 Adam on the float64 gradient, within the bounds of tests/test_gpu_fused_widths.py (H = 1024)."""
    from oracle import solver as osol
    L = pkg("hip.lib")
    trainer = pkg("trainer.diffusion_train")
    ans, n, H, m, batch = "cascade", 4, 50, 32, 65
    model, eng = _model(gpu_device, ans, n, H, m, 1.0)
    tr = trainer.FusedTrainer(model, batch, capacity=4)
    NP, P = eng.NP, eng.n_theta
    assert NP + 3 > ADAM_FAST_MAX and NP == FR.layout(H, n, P, 2 * m)[1]
    g = torch.Generator().manual_seed(H)
    X_ic, X_bc, X_res = [(torch.tensor(b[0]) + (torch.tensor(b[1]) - torch.tensor(b[0])) * torch.rand(k, 3, generator=g))
                         .to(torch.float32) for b, k in ((osol.BOX_IC, tr.n_ic), (osol.BOX_BC1, tr.n_bc), (osol.BOX_DOM, tr.B_res))]
    tr.load_batches(X_ic, X_bc, X_res)
    flat0 = eng.flat.detach().cpu().numpy().copy()
    Bf = model.fourier.B.detach().cpu().numpy()
    tr.fs.run(L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE)
    torch.cuda.synchronize()
    theta_shape, haar = _oracle_args(model)
    want_g, want_parts = FR.reference_loss(flat0, H, n, P, theta_shape, ans, haar, Bf, X_ic.numpy(), X_bc.numpy(), X_res.numpy())
    coef = min(1.0, 1.0 / (np.linalg.norm(want_g) + 1e-6))
    got = tr.fs.flat_grad.cpu().numpy()
    assert np.abs(got[:NP] - coef * want_g).max() < 2e-4 * max(1.0, coef * np.abs(want_g).max())
    assert np.abs(got[NP:] - want_parts).max() < 1e-4 * max(1.0, np.abs(want_parts).max())
    want_p, _, _ = FR.adam_step(flat0, want_g, model.args["lr"])
    new = eng.flat.detach().cpu().numpy()
    clear = np.abs(want_g) > 1e-2 * np.abs(want_g).max()
    assert clear.sum() > NP // 20
    assert np.abs(new - want_p)[clear].max() < 2e-6
    assert np.abs(new - flat0).max() < model.args["lr"] * (1 + 1e-5) + 1e-6
    assert abs(tr.opt.read()["loss"] - float(np.dot([2.0, 4.0, 2.0], want_parts))) < 1e-4 * max(1.0, float(want_parts.max()))


def test_module_paths_match_the_float64_module(gpu_device):
    """forward with requires_grad inputs under nn.pde.diffusion_operator (the generic autograd branch), the fused
    residual(), jets() and the value forward, against the float64 restatement at B = 5; and the parameter gradient of a
    loss through the second derivatives."""
    pde = pkg("nn.pde")
    ans, n, H, m, scale, B = "cascade", 4, 7, 4, 2.0, 5
    model, eng = _model(gpu_device, ans, n, H, m, scale)
    P = eng.n_theta
    flat0 = eng.flat.detach().cpu().numpy().copy()
    Bf = torch.tensor(model.fourier.B.detach().cpu().numpy(), dtype=torch.float64)
    X = torch.rand(B, 3, generator=torch.Generator().manual_seed(9))
    theta_shape, haar = _oracle_args(model)

    from oracle import jets as oj
    Pm = FR.unpack(flat0, H, n, P, m)
    q = oj.qjets_from_ajets(FR.pre_jets_ff(Pm, Bf, X.double(), 6), Pm["theta"].reshape(theta_shape), ans, n, haar, "angle")
    uj = R.post_jets(Pm, q)                                                   # (6, B)
    res = R.residual(uj, (1.0, 1.0, 1.0, 0.01, 0.01))
    cot = torch.randn(B, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want_grad = torch.autograd.grad((cot * res).sum() + uj[0].sum(), [Pm[k] for k in R.NAMES])
    want_grad = np.concatenate([g.numpy().reshape(-1) for g in want_grad])
    uj, res = uj.detach().numpy(), res.detach().numpy()
    scale_j = np.maximum(1.0, np.abs(uj).max(1))

    Xd = X.to(gpu_device)
    assert np.abs(model(Xd).detach().cpu().numpy()[:, 0] - uj[0]).max() < 2e-5
    got_j = model.jets(Xd).detach().cpu().numpy().T
    assert (np.abs(got_j - uj).max(1) < 1e-4 * scale_j).all(), np.abs(got_j - uj).max(1) / scale_j
    u1, r1 = model.residual(Xd)
    assert np.abs(r1.detach().cpu().numpy()[:, 0] - res).max() < 1e-4 * max(1.0, np.abs(res).max())
    t, x, y = (Xd[:, k:k + 1].clone() for k in range(3))
    plain = lambda inp: model(inp)              # hides .residual / .quantum_layer: the generic autograd branch
    u2, r2 = pde.diffusion_operator(plain, t, x, y)
    assert np.abs(u2.detach().cpu().numpy()[:, 0] - uj[0]).max() < 2e-5
    assert np.abs(r2.detach().cpu().numpy()[:, 0] - res).max() < 1e-4 * max(1.0, np.abs(res).max())
    for u_k, r_k in ((u1, r1), (u2, r2)):
        model.zero_grad()
        ((cot.to(gpu_device).float()[:, None] * r_k).sum() + u_k.sum()).backward()
        got = np.concatenate([p.grad.detach().cpu().numpy().reshape(-1) for p in model.parameters()])
        assert np.abs(got - want_grad).max() < 2e-4 * max(1.0, np.abs(want_grad).max()), np.abs(got - want_grad).max()


def test_system_step_refuses_a_map(gpu_device):
    engine, L = pkg("hip.engine"), pkg("hip.lib")
    model, eng = _model(gpu_device, "cascade", 4, 5, 3, 1.0)
    sysrec = L.system_record(1, 1, [(0, 0, 1, -1, -1, 1.0)], [1.0], [1.0])
    with pytest.raises(ValueError):
        engine.SystemStep(eng.circuit, 5, eng.flat, sysrec, 64, 21, 21, engine.OptimState(eng.NP, 0.005, gpu_device))
