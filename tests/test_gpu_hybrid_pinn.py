"""Third workload (the reference's trainer/train.py) on the GPU: the pre network's output map a = pi tanh(v) in both
directions against float64 autograd, the model's forward and residual, one fused step in every circuit family, a
training history, the random-face device sampler and the command-line run, each against the float64 restatement of
tests/hybrid_pinn_reference.py.  Gradient tolerances as in tests/test_gpu_fused_families.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hybrid_pinn_reference as R
import mlp_reference as M
from conftest import GOLDEN, pkg

pytestmark = pytest.mark.gpu

TOL_G, TOL_L = 2e-4, 1e-4


def _lib():
    return pkg("hip.lib")


# ---------------------------------------------------------------- 1. pre network with the map
def _pre_case(H, n, B, saturate, seed):
    g = torch.Generator().manual_seed(seed + 31 * H + 7 * n + B)
    lay, NP = M.layout(H, n, 0)
    flat = np.zeros(NP, dtype=np.float32)
    scale = {"W1": 1.0, "b1": 0.3, "W2": 3.0 / np.sqrt(H), "b2": 0.5}
    for k in ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4"):
        o, s = lay[k]
        m = int(np.prod(s))
        flat[o:o + m] = (torch.randn(m, generator=g, dtype=torch.float64) * scale.get(k, 0.1)).numpy()
    if saturate:      # |v| up to ~20: tanh saturates, the map's derivative vanishes
        o, s = lay["b2"]
        flat[o:o + n] = np.linspace(-20.0, 20.0, n) if n > 1 else 20.0
    X = torch.rand(B, 3, generator=g).to(torch.float32)
    return flat, X


def _ref_pre(flat, X, H, n, nch):
    P = M.unpack(flat, H, n, 0)
    v = M.pre_jets(P, X.double(), nch)
    return P, R.angle_map_fwd(v)


@pytest.mark.parametrize("H", [1, 50, 64, 257])
@pytest.mark.parametrize("n", [1, 4, 16])
@pytest.mark.parametrize("B", [1, 63, 65, 1000])
def test_pre_network_map_matches_float64(H, n, B, gpu_device):
    L = _lib()
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    for saturate in (False, True):
        flat, X = _pre_case(H, n, B, saturate, 1)
        fd, Xd = torch.from_numpy(flat).to(gpu_device), X.to(gpu_device)
        NP = flat.size
        for nch in (6, 1):
            P, a_ref = _ref_pre(flat, X, H, n, nch)
            aj = torch.empty(nch, n, B, dtype=torch.float32, device=gpu_device)
            L.check(lib.qc_pre_forward_map(Xd.data_ptr(), fd.data_ptr(), H, n, 0, L.QC_ANGLE_MAP_TANH_PI, aj.data_ptr(), B, nch,
                                           st), "qc_pre_forward_map")
            got = aj.cpu().double()
            assert torch.isfinite(got).all()
            for c in range(nch):
                err = (got[c] - a_ref[c].detach()).abs().max().item()
                assert err < TOL_L * max(1.0, a_ref[c].abs().max().item()), (saturate, nch, c, err)
            # reverse: a random cotangent of the angle jets -> parameter rows of W1 b1 W2 b2
            ab = torch.randn(nch, n, B, generator=torch.Generator().manual_seed(B + n), dtype=torch.float64)
            grads = torch.autograd.grad((a_ref * ab).sum(), [P[k] for k in ("W1", "b1", "W2", "b2")])
            want = M.flatten(dict(zip(("W1", "b1", "W2", "b2"), grads)), H, n, 0)
            rows = (B + 63) // 64
            part = torch.zeros(rows, NP, dtype=torch.float32, device=gpu_device)
            abd = ab.to(torch.float32).to(gpu_device).contiguous()
            L.check(lib.qc_pre_backward_map(Xd.data_ptr(), fd.data_ptr(), H, n, 0, L.QC_ANGLE_MAP_TANH_PI, aj.data_ptr(),
                                            abd.data_ptr(), part.data_ptr(), NP, 0, B, nch, st), "qc_pre_backward_map")
            d = torch.empty(NP, dtype=torch.float32, device=gpu_device)
            L.check(lib.qc_reduce_rows(part.data_ptr(), rows, NP, NP, d.data_ptr(), st), "qc_reduce_rows")
            d = d.cpu().double().numpy()
            assert np.isfinite(d).all()
            lay, _ = M.layout(H, n, 0)
            # near saturation s = 1 - tau^2 comes from the stored fp32 angle a0 = pi tau, whose resolution limits s to
            # ~1e-7 absolute (the forward pass's tanh is no better): those cases are checked for finiteness and to 1e-3
            tol = 1e-3 if saturate else TOL_G
            for k in ("W1", "b1", "W2", "b2"):
                o, s = lay[k]
                sl = slice(o, o + int(np.prod(s)))
                err = np.abs(d[sl] - want[sl]).max()
                assert err < tol * max(1.0, np.abs(want[sl]).max()), (saturate, nch, k, err)


def test_map_entry_points_check_their_arguments(gpu_device):
    L = _lib()
    lib = L.load()
    X = torch.zeros(4, 3, device=gpu_device)
    p = torch.zeros(1000, device=gpu_device)
    aj = torch.zeros(6, 2, 4, device=gpu_device)
    assert lib.qc_pre_forward_map(X.data_ptr(), p.data_ptr(), 8, 2, 0, 7, aj.data_ptr(), 4, 6, None) == -1
    # the map's reverse pass needs the angle jets
    assert lib.qc_pre_backward_map(X.data_ptr(), p.data_ptr(), 8, 2, 0, L.QC_ANGLE_MAP_TANH_PI, None, aj.data_ptr(),
                                   p.data_ptr(), 1000, 0, 4, 6, None) == -1


# ---------------------------------------------------------------- model helpers
def _model(gpu_device, n, L, seed, monkeypatch, H=50):
    t = pkg("trainer.train")
    monkeypatch.setattr(t.Config, "N_QUBITS", n)
    monkeypatch.setattr(t.Config, "N_LAYERS", L)
    monkeypatch.setattr(t.Config, "CLASSICAL_HIDDEN", H)
    torch.manual_seed(seed)
    model = t.HybridPINN(gpu_device)
    ref = R.standin(n, L, H, seed, {k: v.clone() for k, v in model.state_dict().items()})
    model.to(gpu_device)
    return t, model, ref


def _points(seed, m, face=None):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(m, 3, generator=g)
    if face == "ic":
        X[:, 0] = 0.0
    elif face == "bc":
        side = torch.randint(0, 4, (m,), generator=g)
        X[:, 1] = torch.where(side == 0, 0.0, torch.where(side == 1, 1.0, X[:, 1]))
        X[:, 2] = torch.where(side == 2, 0.0, torch.where(side == 3, 1.0, X[:, 2]))
    return X


# ---------------------------------------------------------------- 2. forward
def test_forward_and_residual_match_the_restatement(gpu_device, monkeypatch):
    t, model, ref = _model(gpu_device, 4, 2, 42, monkeypatch)
    X = _points(5, 90)
    Xd = X.to(gpu_device)
    with torch.no_grad():
        u = model(Xd).cpu().double()
    f_ref, u_ref = R.residual(ref, X.double())
    assert (u - u_ref.detach()).abs().max() < 2e-5
    cols = [Xd[:, k:k + 1].clone() for k in range(3)]
    f, u2 = t.get_pde_residual(model, *cols)                 # fused channels
    tol = TOL_L * max(1.0, f_ref.abs().max().item())
    assert (u2.detach().cpu().double() - u_ref.detach()).abs().max() < 2e-5
    assert (f.detach().cpu().double() - f_ref.detach()).abs().max() < tol
    # the reference's own autograd formulation through the module (forward differentiable in its inputs)
    f3, _ = R.residual(model, Xd)
    assert (f3.detach().cpu().double() - f_ref.detach()).abs().max() < tol


# ---------------------------------------------------------------- 3. one fused step in every circuit family
STEP_CASES = {"merged_n4_L2": (4, 2, 130, 40, 40), "lanes_n6_L1": (6, 1, 70, 20, 20), "hbm_n10_L1": (10, 1, 5, 3, 3)}


def _trainer(t, model, B_res, n_ic, n_bc, capacity=1):
    opt = torch.optim.Adam(model.parameters(), lr=t.Config.LR)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=200)
    L = _lib()
    return pkg("trainer.diffusion_train").FusedTrainer(
        model, B_res, capacity, sampler="torch", n_ic=n_ic, n_bc=n_bc, bc_faces="random",
        pde={"D": t.Config.D, "vx": t.Config.VX, "vy": t.Config.VY, "problem": L.QC_PROBLEM_GAUSSIAN_PULSE},
        loss_weights=(1.0, 5.0, 5.0), max_norm=None, optimizer=opt, scheduler=sch)


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_fused_step_matches_the_restatement(case, gpu_device, monkeypatch):
    n, L, B_res, n_ic, n_bc = STEP_CASES[case]
    t, model, ref = _model(gpu_device, n, L, 11, monkeypatch)
    X_ic, X_bc, X_res = _points(1, n_ic, "ic"), _points(2, n_bc, "bc"), _points(3, B_res)
    tr = _trainer(t, model, B_res, n_ic, n_bc)
    tr.load_batches(X_ic, X_bc, X_res)
    lib = _lib()
    tr.fs.run(lib.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    got = tr.fs.flat_grad.cpu().double().numpy()
    want = R.step_gradient(ref, X_ic, X_bc, X_res)
    NP = got.size - 3
    lay = pkg("hip.engine").param_layout(50, n, 3 * n * L)
    o_post, o_th = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0]
    for name, s in {"pre": slice(0, o_post), "post": slice(o_post, o_th), "theta": slice(o_th, NP)}.items():
        err = np.abs(got[s] - want[s]).max()
        assert err < TOL_G * max(1.0, np.abs(want[s]).max()), (case, name, err)
    # BC targets are ~1e-11 on most of the faces: L_bc needs an absolute floor
    for k in range(3):
        assert abs(got[NP + k] - want[NP + k]) < TOL_L * max(1.0, abs(want[NP + k])), (case, k, got[NP:], want[NP:])
    if case.startswith("merged"):
        # the merged one-launch-per-stage form serves this workload (QC_ERR_UNSUPPORTED otherwise)
        st = torch.cuda.current_stream(gpu_device).cuda_stream
        assert lib.load().qc_fused_step_stage(C.byref(tr.fs.desc), lib.QC_STAGE_PRE_FWD, st) == 0


# ---------------------------------------------------------------- 4. training history
def _fixture():
    return np.load(os.path.join(GOLDEN, "hybrid_pinn_train.npz"))


def _fixture_model(gpu_device):
    """HybridPINN at Config's defaults with the fixture's initial weights (the reference's trainer/train.py run)."""
    z = _fixture()
    t = pkg("trainer.train")
    model = t.HybridPINN(gpu_device)
    model.load_state_dict({k[len("init__"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init__")})
    return t, model.to(gpu_device), z


def test_training_history_matches_the_reference_fixture(gpu_device):
    """The fixture's initial weights and every iteration's batches through load_batches: the loss history and final
    weights of the reference's own train_model (tests/golden/make_golden_hybrid_pinn.py)."""
    t, model, z = _fixture_model(gpu_device)
    want = z["loss_history"]
    steps, B = want.size, t.Config.BATCH_SIZE
    tr = _trainer(t, model, B, B // 2, B // 2, capacity=steps)
    for e in range(steps):
        tr.load_batches(*(torch.from_numpy(z[k][e]) for k in ("ic", "bc", "res")))
        tr.step()
    hist = np.array(tr.opt.loss_history(steps))
    assert np.abs(hist - want).max() < 1e-4 * max(1.0, np.abs(want).max()), (hist, want)
    tr.sync_to_torch()
    for k, p in model.state_dict().items():
        diff = np.abs(p.cpu().double().numpy() - z["final__" + k])
        if k == "q_layer.weights":
            # the last layer's RZ(omega) sits right before the CNOT ring and the Z measurements, which it commutes with:
            # its gradient is zero, so Adam steps on rounding noise in either precision
            diff[-1, :, 2] = 0.0
        assert diff.max() < 2e-3, k      # 21 Adam steps of lr 5e-3: sign-level noise only


def test_residual_matches_the_reference_fixture(gpu_device):
    """get_pde_residual (fused channels) with the initial weights on the fixture's first residual batch."""
    t, model, z = _fixture_model(gpu_device)
    X = torch.from_numpy(z["pde_X"]).to(gpu_device)
    f, u = t.get_pde_residual(model, X[:, 0:1].clone(), X[:, 1:2].clone(), X[:, 2:3].clone())
    assert np.abs(u.detach().cpu().double().numpy() - z["pde_u"]).max() < 2e-5
    assert np.abs(f.detach().cpu().double().numpy() - z["pde_f"]).max() < TOL_L * max(1.0, np.abs(z["pde_f"]).max())


def test_input_derivative_path_does_not_write_the_parameters(gpu_device):
    """The reference-style path (forward differentiable in its inputs) keeps its parameter snapshot in a scratch vector:
    a parameter update between its forward and backward pass survives the backward pass."""
    t, model, _ = _fixture_model(gpu_device)
    X = _points(9, 20).to(gpu_device).requires_grad_(True)
    u = model(X)
    b = model.encoder[0].bias
    with torch.no_grad():
        b.add_(0.5)
    after = b.detach().clone()
    u.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(b.detach(), after)
    assert b.grad is not None and torch.isfinite(b.grad).all()


# ---------------------------------------------------------------- 5. device sampler
def test_device_sampler_random_faces(gpu_device, monkeypatch):
    t, model, _ = _model(gpu_device, 4, 2, 3, monkeypatch)
    B = 1 << 16
    tr = _trainer(t, model, B, B, B)
    tr.sampler = "device"
    tr.sample()
    tr.fs.run(_lib().QC_PHASE_SAMPLE | _lib().QC_PHASE_GRADS)      # merged form: the pre stage draws the points
    torch.cuda.synchronize()
    Xv = tr.fs.X_val.cpu()
    ic, bc = Xv[:B], Xv[B:]
    assert (ic[:, 0] == 0).all() and ic[:, 1:].std() > 0.2
    on = torch.stack([bc[:, 1] == 0, bc[:, 1] == 1, bc[:, 2] == 0, bc[:, 2] == 1], 1)
    # exactly one coordinate on a face; the only other case allowed is a free coordinate drawn as exactly 0.0 (u01 of a
    # word whose top 24 bits are zero: ~2^-24 per point, ~2^-8 for the batch), which then also reads as "on a face"
    bad = on.sum(1) != 1
    zero_free = (on.sum(1) == 2) & (((bc[:, 1] == 0) & (bc[:, 2] == 1)) | ((bc[:, 1] == 1) & (bc[:, 2] == 0)) |
                                    ((bc[:, 1] == 0) & (bc[:, 2] == 0)))
    assert (bad == zero_free).all() and int(bad.sum()) <= 2, bc[bad]
    frac = on.double().mean(0)
    assert ((frac - 0.25).abs() < 0.01).all(), frac
    assert bc[:, 0].min() >= 0 and bc[:, 0].max() < 1 and bc[:, 0].std() > 0.2
    # k_sample (the two-stream form's sampler) draws the same points, and a draw at a rank offset is a slice of it
    L = _lib()
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    d = tr.fs.desc
    full = torch.empty(2 * B, 3, device=gpu_device)
    L.check(lib.qc_sample_collocation_faces(None, 0, 0, full.data_ptr(), B, 0, B, 0, L.QC_BC_RANDOM_FACE, d.sample_seed,
                                            d.sample_step, st), "qc_sample_collocation_faces")
    off, m = 1000, 3001
    part = torch.empty(2 * m, 3, device=gpu_device)
    L.check(lib.qc_sample_collocation_faces(None, 0, 0, part.data_ptr(), m, off, m, off, L.QC_BC_RANDOM_FACE, d.sample_seed,
                                            d.sample_step, st), "qc_sample_collocation_faces")
    torch.cuda.synchronize()
    full, part = full.cpu(), part.cpu()
    assert torch.equal(full, Xv)
    assert torch.equal(part[:m], full[off:off + m]) and torch.equal(part[m:], full[B + off:B + off + m])


# ---------------------------------------------------------------- 6. end to end
def test_main_end_to_end(gpu_device, tmp_path, capsys, monkeypatch):
    t = pkg("trainer.train")
    monkeypatch.setattr(t.Config, "EPOCHS", t.Config.EPOCHS)
    model, hist = t.main(["--epochs", "60", "--out-dir", str(tmp_path)])
    assert len(hist) == 61 and hist[-1] < hist[0]
    sd = torch.load(tmp_path / "hybrid_pinn_diffusion.pth", weights_only=True)
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.REFERENCE_KEYS
    out = capsys.readouterr().out
    assert "Epoch: 0 |" in out and "Validation MSE at t=0.5:" in out
    assert (tmp_path / "hybrid_pinn_result.png").exists()
