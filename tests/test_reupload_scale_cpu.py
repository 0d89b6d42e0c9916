"""Trainable input scalings of the re-uploaded angles (args["reupload_scale"], gate EMBEDS) without a GPU: the gate
program (EMBEDS rows and their slots), the layer's second Parameter, the solver's layout and checkpoint, the refusals, and
the float64 restatement of tests/reupload_scale_reference.py against closed forms."""

import numpy as np
import pytest
import torch

import reupload_reference as RR
import reupload_scale_reference as RS
from conftest import pkg
from test_reupload_cpu import _args, rx_only

circuits = pkg("circuits")


def test_opcode():
    assert circuits.OP_EMBED_S == 9 and circuits.OP_NAMES[9] == "EMBEDS"
    assert circuits.OP_EMBED_S in circuits.PARAMETRIC and circuits.OP_EMBED not in circuits.PARAMETRIC
    assert circuits.OP_EMBED == 8 and circuits.OP_NAMES[8] == "EMBED"


@pytest.mark.parametrize("mode", ["wire", "layer"])
@pytest.mark.parametrize("ans", circuits.ANSATZ_NAMES)
@pytest.mark.parametrize("L", [1, 2, 3])
def test_program_rows(ans, L, mode):
    n = 5 if ans in ("alternate", "sim_circ_15") else 4
    P = circuits.params_per_layer(ans, n)
    re = circuits.build_program(ans, n, L, True, reupload=True)
    sc = circuits.build_program(ans, n, L, True, reupload=True, reupload_scale=mode)
    assert sc.n_layers == L and sc.use_haar
    if L == 1:
        plain = circuits.build_program(ans, n, L, True)
        assert np.array_equal(sc.rows(), plain.rows()) and sc.n_params == plain.n_params
        return
    assert sc.n_params == L * P + (L - 1) * (n if mode == "wire" else 1)
    rows = sc.rows()
    is_s = rows[:, 0] == circuits.OP_EMBED_S
    # opcode 9 -> 8 and its slots -> -1: the reupload=True program, row for row
    mapped = rows.copy()
    mapped[is_s, 0] = circuits.OP_EMBED
    mapped[is_s, 3] = -1
    assert np.array_equal(mapped, re.rows())
    assert not (rows[:, 0] == circuits.OP_EMBED).any() and is_s.sum() == (L - 1) * n
    # the slots: behind the ansatz slots, which do not move
    got = rows[is_s]
    want = [(9, w, -1, L * P + (l - 1) * n + w if mode == "wire" else L * P + (l - 1)) for l in range(1, L) for w in range(n)]
    assert np.array_equal(got, np.array(want))
    assert sc.algorithmic_flops() == re.algorithmic_flops()
    assert sc.algorithmic_flops() == circuits.build_program(ans, n, L, True).algorithmic_flops() + (L - 1) * n * 6 * (1 << n)


def test_program_none_is_todays_and_scale_needs_reupload():
    for L in (1, 2, 3):
        a = circuits.build_program("cascade", 4, L, True, reupload=True)
        b = circuits.build_program("cascade", 4, L, True, reupload=True, reupload_scale=None)
        assert np.array_equal(a.rows(), b.rows()) and a.n_params == b.n_params
    with pytest.raises(ValueError, match="reupload"):
        circuits.build_program("cascade", 4, 2, True, reupload_scale="wire")
    with pytest.raises(ValueError, match="reupload_scale"):
        circuits.build_program("cascade", 4, 2, True, reupload=True, reupload_scale="axis")


@pytest.mark.parametrize("flag,mode,cols", [(True, "wire", 3), ("wire", "wire", 3), ("layer", "layer", 1)])
def test_layer_parameters(flag, mode, cols):
    Layer = pkg("nn.DVQuantumLayer").DVQuantumLayer
    layer = Layer(_args(num_qubits=3, num_quantum_layers=3, reupload_scale=flag))
    assert layer.reupload_scale == mode and layer.has_embed_gates
    names = [k for k, _ in layer.named_parameters()]
    assert names == ["params", "embed_scale"] and list(layer.state_dict()) == ["params", "embed_scale"]
    assert tuple(layer.embed_scale.shape) == (2, cols) and layer.embed_scale.dtype == torch.float32
    assert torch.equal(layer.embed_scale.detach(), torch.ones(2, cols))
    assert tuple(layer.params.shape) == (3, 9)
    th = layer.theta()
    assert th.shape == (layer.program.n_params,) and th.requires_grad
    assert torch.equal(th.detach(), torch.cat([layer.params.detach().reshape(-1), torch.ones(2 * cols)]))
    # the same ansatz parameters as the layer without scalings (the second Parameter draws nothing)
    torch.manual_seed(7)
    a = Layer(_args(num_qubits=3, num_quantum_layers=3, reupload_scale=flag))
    torch.manual_seed(7)
    b = Layer(_args(num_qubits=3, num_quantum_layers=3))
    assert torch.equal(a.params.detach(), b.params.detach()) and b.embed_scale is None and b.reupload_scale is None
    assert list(b.state_dict()) == ["params"]


def test_layer_with_one_layer_has_no_scalings():
    Layer = pkg("nn.DVQuantumLayer").DVQuantumLayer
    layer = Layer(_args(num_qubits=3, num_quantum_layers=1, reupload_scale="wire"))
    assert layer.embed_scale is None and [k for k, _ in layer.named_parameters()] == ["params"]
    assert not layer.has_embed_gates and layer.theta() is layer.params
    for off in (None, False):
        assert Layer(_args(num_qubits=3, reupload_scale=off)).embed_scale is None


def test_layer_construction_errors():
    Layer = pkg("nn.DVQuantumLayer").DVQuantumLayer
    with pytest.raises(ValueError, match="reupload=True"):
        Layer(_args(reupload=False, reupload_scale="wire"))
    a = _args(reupload_scale=True)
    del a["reupload"]
    with pytest.raises(ValueError, match="reupload=True"):
        Layer(a)
    with pytest.raises(ValueError, match="amplitude"):
        Layer(_args(encoding="amplitude", reupload_scale="wire"))
    for n in (1, 6):
        with pytest.raises(ValueError, match="2 <= num_qubits <= 5"):
            Layer(_args(num_qubits=n, reupload_scale="layer"))
    with pytest.raises(ValueError, match="reupload_scale"):
        Layer(_args(reupload_scale="axis"))


def test_describe_lists_the_scaled_gates():
    Layer = pkg("nn.DVQuantumLayer").DVQuantumLayer
    text = Layer(_args(num_qubits=3, q_ansatz="cascade", reupload_scale="wire")).describe()
    assert "EMBEDS[0] p18 | EMBEDS[1] p19 | EMBEDS[2] p20" in text and text.count("EMBEDS[") == 3
    text = Layer(_args(num_qubits=3, q_ansatz="cascade", reupload_scale="layer")).describe()
    assert "EMBEDS[0] p18 | EMBEDS[1] p18 | EMBEDS[2] p18" in text
    assert "EMBEDS" not in Layer(_args(num_qubits=3)).describe()


def test_trig_interpolant_is_refused():
    Layer = pkg("nn.DVQuantumLayer").DVQuantumLayer
    with pytest.raises(ValueError, match="degree"):
        Layer(_args(reupload_scale="wire")).trig_interpolant(torch.zeros(2, 4))


def test_solver_layout_checkpoint_and_system_trainer(tmp_path):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    engine = pkg("hip.engine")
    n, L, H = 3, 3, 8
    model = Solver(_args(num_qubits=n, num_quantum_layers=L, classic_network=[3, H, 1], reupload_scale="wire"), None,
                   device=torch.device("cpu"))
    ql = model.quantum_layer
    P = circuits.params_per_layer("cascade", n)
    n_theta = L * P + (L - 1) * n
    assert ql.program.n_params == n_theta
    slots = model._slots()
    assert slots[-2][0] is ql.params and slots[-1][0] is ql.embed_scale
    assert [k for _, k, _ in slots[-2:]] == [L * P, (L - 1) * n]
    NP = sum(k for _, k, _ in slots)
    lay = engine.param_layout(H, n, n_theta, n_scale=(L - 1) * n)
    assert lay["__total__"][0] == NP
    assert lay["quantum_layer.params"] == (NP - n_theta, (n_theta,))            # spans all of theta
    assert lay["quantum_layer.embed_scale"] == (NP - (L - 1) * n, ((L - 1) * n,))
    assert "quantum_layer.embed_scale" not in engine.param_layout(H, n, L * P)
    # the flat vector the jet path builds: [.. | params | embed_scale]
    with torch.no_grad():
        ql.embed_scale.copy_(torch.tensor([[0.5, -1.25, 2.0], [1.5, 0.0, 0.75]]))
    flat = model._flat_for_output(0)
    assert flat.numel() == NP
    assert torch.equal(flat[-n_theta:].detach(), ql.theta().detach())
    assert torch.equal(flat[-(L - 1) * n:].detach(), ql.embed_scale.detach().reshape(-1))
    # save_state / load_state round trip with non-trivial scalings
    path = str(tmp_path / "model.pth")
    model.save_state(path)
    state = Solver.load_state(path)
    assert state["args"]["reupload_scale"] == "wire"
    for key in ("quantum_layer", "quantum_params"):
        assert list(state[key]) == ["params", "embed_scale"]
        assert torch.equal(state[key]["embed_scale"], ql.embed_scale.detach())
    other = Solver(_args(num_qubits=n, num_quantum_layers=L, classic_network=[3, H, 1], reupload_scale="wire"), None,
                   device=torch.device("cpu"))
    assert torch.equal(other.quantum_layer.embed_scale.detach(), torch.ones(L - 1, n))
    other.quantum_layer.load_state_dict(state["quantum_layer"])
    assert torch.equal(other.quantum_layer.embed_scale.detach(), ql.embed_scale.detach())
    assert torch.equal(other.quantum_layer.params.detach(), ql.params.detach())
    tab = pkg("data.tabulated")
    ST = pkg("trainer.system_train").SystemTrainer
    ds = tab.TabulatedSystem.__new__(tab.TabulatedSystem)
    with pytest.raises(ValueError, match="re-uploaded"):
        ST(model, 64, ds)


# ---------------------------------------------------------------- the restatement against closed forms
def _scaled_rx_only(sim, theta, x):
    """n = 2, L = 2, one trainable RX per wire, no entangler: RX(a) RX(th0) RX(s a) RX(th1) = RX((1 + s) a + th0 + th1).
    theta = (th0[0], th0[1], th1[0], th1[1], s[0], s[1])."""
    rx_only(sim, theta[0:2])
    for w in range(2):
        sim.RX(theta[4 + w] * x[:, w], w)
    rx_only(sim, theta[2:4])


_scaled_rx_only.takes_angles = True


def _draw(seed, B):
    g = torch.Generator().manual_seed(seed)
    aj = torch.randn(6, 2, B, generator=g, dtype=torch.float64)
    th = torch.randn(4, generator=g, dtype=torch.float64)
    s = 1.0 + 0.4 * torch.randn(2, generator=g, dtype=torch.float64)
    return aj, torch.cat([th, s])


def test_restatement_value_and_scale_gradient_closed_form():
    aj, theta = _draw(3, 7)
    a = aj[0].T.contiguous()
    theta = theta.clone().requires_grad_(True)
    q = RS.expvals(a, theta, _scaled_rx_only, 2)
    s = theta[4].detach()
    phi = (1 + s) * a[:, 0] + theta[0].detach() + theta[2].detach()
    assert np.abs((q[0].detach() - torch.cos(phi)).numpy()).max() < 1e-14
    assert np.abs(q[1].detach().numpy()).max() < 1e-14
    # d<Z_0>/ds = -a sin(phi), point by point
    for b in range(a.shape[0]):
        g, = torch.autograd.grad(q[0, b], theta, retain_graph=True)
        assert abs(g[4].item() + (a[b, 0] * torch.sin(phi[b])).item()) < 1e-13
        assert abs(g[5].item()) < 1e-13


def test_restatement_jets_closed_form():
    aj, theta = _draw(4, 6)
    q = RS.qjets(aj, theta, _scaled_rx_only, 2).detach()
    s = theta[4]
    phi = (1 + s) * aj[0, 0] + theta[0] + theta[2]
    assert np.abs((q[0, 0] - torch.cos(phi)).numpy()).max() < 1e-14
    for k in (1, 2, 3):                                          # phi' = (1 + s) a_k
        assert np.abs((q[k, 0] + torch.sin(phi) * (1 + s) * aj[k, 0]).numpy()).max() < 1e-13
    for k in (2, 3):                                             # phi'' = (1 + s) a_kk
        want = -torch.cos(phi) * ((1 + s) * aj[k, 0]) ** 2 - torch.sin(phi) * (1 + s) * aj[k + 2, 0]
        assert np.abs((q[k + 2, 0] - want).numpy()).max() < 1e-13
    assert np.abs(q[:, 1].numpy()).max() < 1e-13


@pytest.mark.parametrize("ans,n,L,mode", [("cascade", 3, 2, "wire"), ("layered", 4, 3, "layer"), ("farhi", 5, 3, "wire")])
def test_restatement_at_ones_is_the_reuploaded_circuit(ans, n, L, mode):
    params, x, _ = RR.vjp_inputs(ans, n, L, 5)
    theta = torch.cat([params.reshape(-1).double(), torch.ones(RS.n_scales(n, L, mode), dtype=torch.float64)])
    haar = RS.haar_for(n, 1)
    a = RS.expvals(x, theta, RS.whole_circuit(ans, n, L, mode), n, haar)
    b = RR.expvals(x, params, ans, n, haar, reupload=True)
    assert torch.equal(a, b)
    theta[-1] = 1.3
    assert (RS.expvals(x, theta, RS.whole_circuit(ans, n, L, mode), n, haar) - b).abs().max() > 1e-3
