"""Third workload (trainer/train.py) without a GPU: the circuit lowering, the output map of the pre network against
torch.autograd in float64, the model's parameters and registration order, the refusal of IBM / shot-based
configurations, and - against ``tests/golden/hybrid_pinn_train.npz``, written by the reference's own trainer/train.py
(tests/golden/make_golden_hybrid_pinn.py) - the sampler's batches, the initial weights, exact_u, get_pde_residual and
the float64 restatement's training history."""
import math
import os

import numpy as np
import pytest
import torch

import hybrid_pinn_reference as R
from conftest import GOLDEN, pkg


def fixture():
    return np.load(os.path.join(GOLDEN, "hybrid_pinn_train.npz"))


def _expected_rows(n, L):
    RZ, RY, CNOT = 2, 1, 4
    rows = []
    for layer in range(L):
        base = 3 * n * layer
        for i in range(n):
            rows += [(RZ, i, -1, base + 3 * i), (RY, i, -1, base + 3 * i + 1), (RZ, i, -1, base + 3 * i + 2)]
        rows += [(CNOT, i, (i + 1) % n, -1) for i in range(n)]
    return rows


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("L", [1, 2])
def test_lowering_gate_rows(n, L):
    c = pkg("circuits")
    prog = c.build_rot_ring_program(n, L)
    assert [tuple(r) for r in prog.rows().tolist()] == _expected_rows(n, L)
    assert prog.n_params == 3 * n * L and not prog.use_haar
    assert c.ROT_RING not in c.ANSATZ_NAMES           # not a DVQuantumLayer ansatz


def test_lowering_hand_written_n2_L1():
    prog = pkg("circuits").build_rot_ring_program(2, 1)
    assert [tuple(r) for r in prog.rows().tolist()] == [
        (2, 0, -1, 0), (1, 0, -1, 1), (2, 0, -1, 2), (2, 1, -1, 3), (1, 1, -1, 4), (2, 1, -1, 5), (4, 0, 1, -1),
        (4, 1, 0, -1)]


def test_lowering_needs_two_wires():
    with pytest.raises(ValueError):
        pkg("circuits").build_rot_ring_program(1, 1)


def _v_of_inputs(X, scale):
    """A smooth scalar network output v(t, x, y) (B,) with |v| up to ~scale, differentiable in X."""
    t, x, y = X[:, 0], X[:, 1], X[:, 2]
    return scale * torch.tanh(1.3 * t - 0.7 * x + 0.9 * y * x) + 0.4 * torch.sin(3 * x) * y + 0.2 * y ** 2


def _jets_by_autograd(fn, X):
    """{value, t, x, y, xx, yy} of fn(X) (B,) by autograd in X."""
    X = X.clone().requires_grad_(True)
    f = fn(X)
    g = torch.autograd.grad(f.sum(), X, create_graph=True)[0]
    gxx = torch.autograd.grad(g[:, 1].sum(), X, create_graph=True)[0][:, 1]
    gyy = torch.autograd.grad(g[:, 2].sum(), X, create_graph=True)[0][:, 2]
    return torch.stack([f, g[:, 0], g[:, 1], g[:, 2], gxx, gyy])


@pytest.mark.parametrize("scale", [0.5, 3.0, 20.0])
def test_angle_map_forward_matches_autograd(scale):
    g = torch.Generator().manual_seed(7)
    X = torch.rand(200, 3, generator=g, dtype=torch.float64)
    v = _jets_by_autograd(lambda Z: _v_of_inputs(Z, scale), X).detach()
    want = _jets_by_autograd(lambda Z: math.pi * torch.tanh(_v_of_inputs(Z, scale)), X).detach()
    got = R.angle_map_fwd(v)
    assert torch.isfinite(got).all()
    assert (got - want).abs().max() < 1e-9 * max(1.0, want.abs().max().item())
    assert (R.angle_map_fwd(v[:1]) - want[:1]).abs().max() < 1e-12


@pytest.mark.parametrize("vmax", [0.5, 4.0, 20.0])
def test_angle_map_reverse_matches_autograd(vmax):
    g = torch.Generator().manual_seed(3)
    v = torch.randn(6, 300, generator=g, dtype=torch.float64)
    v[0] = torch.linspace(-vmax, vmax, 300, dtype=torch.float64)
    ab = torch.randn(6, 300, generator=g, dtype=torch.float64)
    vv = v.clone().requires_grad_(True)
    a = R.angle_map_fwd(vv)
    want = torch.autograd.grad((a * ab).sum(), vv)[0]
    got = R.angle_map_bwd(ab, a.detach())
    assert torch.isfinite(got).all()
    assert (got - want).abs().max() < 1e-9 * max(1.0, want.abs().max().item())
    w1 = torch.autograd.grad((R.angle_map_fwd(vv[:1]) * ab[:1]).sum(), vv)[0][:1]
    assert (R.angle_map_bwd(ab[:1], a.detach()[:1]) - w1).abs().max() < 1e-12


def test_state_dict_keys_shapes_and_kernel_order():
    t = pkg("trainer.train")
    t.set_seed(42)
    model = t.HybridPINN(torch.device("cpu"))
    sd = model.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.REFERENCE_KEYS
    assert [n for n, _ in model.named_parameters()] == list(R.KERNEL_ORDER)
    lay = pkg("hip.engine").param_layout(50, 4, 24)
    assert sum(p.numel() for p in model.parameters()) == lay["__total__"][0]


def test_initial_values_follow_the_reference_creation_order():
    t = pkg("trainer.train")
    t.set_seed(42)
    model = t.HybridPINN(torch.device("cpu"))
    torch.manual_seed(42)
    ref = R.StandIn(4, 2, 50)           # created encoder, q_layer, decoder like the reference
    got, want = model.state_dict(), ref.state_dict()
    for k in R.REFERENCE_KEYS:
        assert torch.equal(got[k], want[k]), k
    w = got["q_layer.weights"]
    assert w.min() >= 0 and w.max() < 2 * math.pi
    model.load_state_dict(want)         # a reference-ordered state_dict loads by key


def test_sampler_draw_order():
    t = pkg("trainer.train")
    s = t.PDESampler(torch.device("cpu"))
    t.set_seed(42)
    tr, xr, yr = s.sample_domain(8)
    ti, xi, yi, ui = s.sample_initial(4)
    tb, xb, yb, ub = s.sample_boundary(4)
    torch.manual_seed(42)
    want = [torch.rand(8, 1) for _ in range(3)]
    want_i = [torch.rand(4, 1) for _ in range(2)]
    want_t = torch.rand(4, 1)
    side = torch.randint(0, 4, (4, 1))
    bx, by = torch.rand(4, 1), torch.rand(4, 1)
    assert all(torch.equal(a, b) for a, b in zip((tr, xr, yr), want))
    assert torch.equal(ti, torch.zeros(4, 1)) and torch.equal(xi, want_i[0]) and torch.equal(yi, want_i[1])
    assert torch.equal(tb, want_t)
    assert torch.equal(xb, torch.where(side == 0, 0.0, torch.where(side == 1, 1.0, bx)))
    assert torch.equal(yb, torch.where(side == 2, 0.0, torch.where(side == 3, 1.0, by)))
    assert torch.allclose(ui, t.exact_u(ti, xi, yi)) and torch.allclose(ub, t.exact_u(tb, xb, yb))


def test_autograd_residual_of_a_plain_model():
    t = pkg("trainer.train")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)).double()
    X = torch.rand(10, 3, dtype=torch.float64)
    f, u = t.get_pde_residual(net, X[:, 0:1].clone(), X[:, 1:2].clone(), X[:, 2:3].clone())
    f2, u2 = R.residual(net, X)
    assert torch.allclose(f, f2) and torch.allclose(u, u2)


def test_initial_state_dict_matches_the_reference_fixture():
    z = fixture()
    t = pkg("trainer.train")
    t.set_seed(t.Config.SEED)
    sd = t.HybridPINN(torch.device("cpu")).state_dict()
    assert set(sd) == {k[len("init__"):] for k in z.files if k.startswith("init__")}
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), z["init__" + k]), k


def test_sampler_batches_and_targets_match_the_reference_fixture():
    """set_seed, model construction, then 21 x (domain, initial, boundary) draws: the reference's train_model order."""
    z = fixture()
    t = pkg("trainer.train")
    B = t.Config.BATCH_SIZE
    t.set_seed(t.Config.SEED)
    t.HybridPINN(torch.device("cpu"))
    s = t.PDESampler(torch.device("cpu"))
    for e in range(z["loss_history"].size):
        tr, xr, yr = s.sample_domain(B)
        ti, xi, yi, ui = s.sample_initial(B // 2)
        tb, xb, yb, ub = s.sample_boundary(B // 2)
        assert np.array_equal(torch.cat([tr, xr, yr], 1).numpy(), z["res"][e]), e
        assert np.array_equal(torch.cat([ti, xi, yi], 1).numpy(), z["ic"][e]), e
        assert np.array_equal(torch.cat([tb, xb, yb], 1).numpy(), z["bc"][e]), e
        assert np.array_equal(ui.numpy(), z["u_ic"][e]) and np.array_equal(ub.numpy(), z["u_bc"][e]), e
        X = torch.from_numpy(z["bc"][e])
        assert np.array_equal(t.exact_u(X[:, 0:1], X[:, 1:2], X[:, 2:3]).numpy(), z["u_bc"][e])


def _fixture_standin(z):
    return R.standin(4, 2, 50, 0, {k[len("init__"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init__")})


def test_restated_residual_matches_the_reference_fixture():
    """The reference's get_pde_residual (autograd through its float32 inputs) on the stand-in with the initial weights."""
    z = fixture()
    f, u = R.residual(_fixture_standin(z), torch.from_numpy(z["pde_X"]).double())
    assert np.abs(u.detach().numpy() - z["pde_u"]).max() < 1e-12
    assert np.abs(f.detach().numpy() - z["pde_f"]).max() < 1e-6 * max(1.0, np.abs(z["pde_f"]).max())


def test_restatement_reproduces_the_reference_training_history():
    """tests/hybrid_pinn_reference.train (the float64 loop the GPU tests compare with) against the reference's own
    train_model on the same model and batches."""
    z = fixture()
    m = _fixture_standin(z)
    batches = [tuple(torch.from_numpy(z[k][e]).double() for k in ("ic", "bc", "res")) for e in range(z["loss_history"].size)]
    hist = np.array(R.train(m, batches))
    want = z["loss_history"]
    assert np.abs(hist - want).max() < 1e-6 * max(1.0, np.abs(want).max()), (hist, want)
    for k, p in m.state_dict().items():
        diff = np.abs(p.numpy() - z["final__" + k])
        if k == "q_layer.weights":
            diff[-1, :, 2] = 0.0       # zero-gradient angles: Adam steps on rounding noise (tests/test_gpu_hybrid_pinn.py)
        assert diff.max() < 1e-6, k


@pytest.mark.parametrize("attr,value", [("BACKEND", "ibm_brisbane"), ("SHOTS", 1024)])
def test_ibm_and_shots_are_refused(attr, value, monkeypatch):
    t = pkg("trainer.train")
    monkeypatch.setattr(t.Config, attr, value)
    with pytest.raises(NotImplementedError):
        t.HybridPINN(torch.device("cpu"))
