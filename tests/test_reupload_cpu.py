"""Data re-uploading without a GPU: the gate program (EMBED positions, unchanged slots), the Python surface's refusals and
the float64 restatement of tests/reupload_reference.py against closed forms."""

import numpy as np
import pytest
import torch

import reupload_reference as RR
from conftest import pkg

circuits = pkg("circuits")


def _args(**over):
    a = {"batch_size": 64, "epochs": 1, "lr": 0.005, "seed": 1, "print_every": 100, "num_qubits": 4,
         "num_quantum_layers": 2, "classic_network": [3, 50, 1], "q_ansatz": "cascade", "shots": 1024,
         "problem": "diffusion", "solver": "DV", "encoding": "None", "use_ibm_hardware": False, "reupload": True}
    a.update(over)
    return a


def test_opcode():
    assert circuits.OP_EMBED == 8 and circuits.OP_NAMES[8] == "EMBED" and circuits.OP_EMBED not in circuits.PARAMETRIC


@pytest.mark.parametrize("ans", circuits.ANSATZ_NAMES)
@pytest.mark.parametrize("L", [1, 2, 3])
def test_program_rows(ans, L):
    n = 5 if ans in ("alternate", "sim_circ_15") else 4          # (alternate over-indexes for even n, as the reference)
    plain = circuits.build_program(ans, n, L, True)
    re = circuits.build_program(ans, n, L, True, reupload=True)
    assert re.n_params == plain.n_params and re.n_layers == L and re.use_haar
    if L == 1:
        assert np.array_equal(re.rows(), plain.rows())
        return
    rows, prow = re.rows(), plain.rows()
    per = (len(prow) - 3) // L                                   # gates of one ansatz layer (two U4 and the H follow)
    assert len(rows) == len(prow) + (L - 1) * n
    # without the EMBED rows the program is the plain one, slots included
    assert np.array_equal(rows[rows[:, 0] != circuits.OP_EMBED], prow)
    # an EMBED layer on wires 0..n-1, ascending, in front of every layer after the first
    at = np.flatnonzero(rows[:, 0] == circuits.OP_EMBED)
    want = np.concatenate([np.arange(n) + l * per + (l - 1) * n for l in range(1, L)])
    assert np.array_equal(at, want)
    for l in range(1, L):
        blk = rows[l * per + (l - 1) * n:l * per + l * n]
        assert np.array_equal(blk, np.array([(circuits.OP_EMBED, w, -1, -1) for w in range(n)]))
    assert re.algorithmic_flops() == plain.algorithmic_flops() + (L - 1) * n * 6 * (1 << n)


def test_describe_lists_the_embed_gates():
    Layer = pkg("nn.DVQuantumLayer").DVQuantumLayer
    text = Layer(_args(num_qubits=3, q_ansatz="cascade")).describe()
    assert text.count("EMBED[") == 3 and "EMBED[0] | EMBED[1] | EMBED[2]" in text
    assert "EMBED" not in Layer(_args(num_qubits=3, reupload=False)).describe()
    assert "EMBED" not in Layer(_args(num_qubits=3, num_quantum_layers=1)).describe()


def test_construction_errors():
    Layer = pkg("nn.DVQuantumLayer").DVQuantumLayer
    with pytest.raises(ValueError, match="amplitude"):
        Layer(_args(encoding="amplitude"))
    for n in (1, 6):
        with pytest.raises(ValueError, match="2 <= num_qubits <= 5"):
            Layer(_args(num_qubits=n))
    assert Layer(_args()).reupload and not Layer(_args(reupload=False)).reupload
    a = _args()
    del a["reupload"]
    assert not Layer(a).reupload


def test_trig_interpolant_is_refused():
    Layer = pkg("nn.DVQuantumLayer").DVQuantumLayer
    with pytest.raises(ValueError, match="degree"):
        Layer(_args()).trig_interpolant(torch.zeros(2, 4))


def test_solver_carries_the_flag_and_system_trainer_refuses(tmp_path):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    model = Solver(_args(), None, device=torch.device("cpu"))
    assert model.quantum_layer.reupload and model.args["reupload"]
    assert any(g.op == circuits.OP_EMBED for g in model.quantum_layer.program.gates)
    # save_state / load_state carry the key in args, like every other key
    path = str(tmp_path / "model.pth")
    model.save_state(path)
    assert Solver.load_state(path)["args"]["reupload"] is True
    tab = pkg("data.tabulated")
    ST = pkg("trainer.system_train").SystemTrainer
    ds = tab.TabulatedSystem.__new__(tab.TabulatedSystem)           # (refused before the dataset is looked at)
    with pytest.raises(ValueError, match="re-uploaded"):
        ST(model, 64, ds)


# ---------------------------------------------------------------- the restatement against closed forms
def rx_only(sim, p):
    """n = 2, one trainable RX per wire and no entangler: RX(a) RX(th0) RX(a) RX(th1) = RX(2a + th0 + th1) on each wire."""
    for q in range(sim.n):
        sim.RX(p[q], q)


def _closed(a, th):
    """<Z_w> of |0> -> RX(a) RX(th0) RX(a) RX(th1) [-> H on the last wire]: wire 0: cos(2a + th0 + th1); the last wire after H
    measures <X> of an RX-rotated |0>, which is 0."""
    return torch.cos(2 * a[:, 0] + th[0, 0] + th[1, 0])


def test_restatement_value_closed_form():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(7, 2, generator=g, dtype=torch.float64)
    th = torch.randn(2, 2, generator=g, dtype=torch.float64)
    q = RR.expvals(a, th, rx_only, 2, None, True)
    assert np.abs((q[0] - _closed(a, th)).numpy()).max() < 1e-14
    assert np.abs(q[1].numpy()).max() < 1e-14
    # without re-uploading: cos(a + th0 + th1), and the two differ
    qp = RR.expvals(a, th, rx_only, 2, None, False)
    assert np.abs((qp[0] - torch.cos(a[:, 0] + th[0, 0] + th[1, 0])).numpy()).max() < 1e-14
    assert np.abs((q[0] - qp[0]).numpy()).max() > 0.1
    # single precision state: close, not equal
    q32 = RR.expvals(a, th, rx_only, 2, None, True, dtype=torch.complex64)
    gap = np.abs((q32 - q).numpy()).max()
    assert 0 < gap < 1e-5


def test_restatement_jets_closed_form():
    g = torch.Generator().manual_seed(4)
    B = 6
    aj = torch.randn(6, 2, B, generator=g, dtype=torch.float64)
    th = torch.randn(2, 2, generator=g, dtype=torch.float64)
    q = RR.qjets(aj, th, rx_only, 2, None, True).detach()
    phi = 2 * aj[0, 0] + th[0, 0] + th[1, 0]
    assert np.abs((q[0, 0] - torch.cos(phi)).numpy()).max() < 1e-14
    for k in (1, 2, 3):                                          # d/de cos(phi(e)), phi' = 2 a_k
        assert np.abs((q[k, 0] + torch.sin(phi) * 2 * aj[k, 0]).numpy()).max() < 1e-13
    for k in (2, 3):                                             # -cos(phi) phi'^2 - sin(phi) phi'',  phi'' = 2 a_kk
        want = -torch.cos(phi) * (2 * aj[k, 0]) ** 2 - torch.sin(phi) * 2 * aj[k + 2, 0]
        assert np.abs((q[k + 2, 0] - want).numpy()).max() < 1e-13
    assert np.abs(q[:, 1].numpy()).max() < 1e-13


def test_restatement_with_one_layer_is_the_oracle():
    from oracle import statevector as sv
    params, x, _ = RR.vjp_inputs("cascade", 3, 1, 5)
    a = RR.expvals(x, params, "cascade", 3, None, True)
    b = sv.circuit_expvals(x.double(), params.double(), "cascade", 3, None)
    assert torch.equal(a, b)
    params, x, _ = RR.vjp_inputs("layered", 4, 2, 5)
    haar = sv.haar_pair(1, 2)
    assert torch.equal(RR.expvals(x, params, "layered", 4, haar, False), sv.circuit_expvals(x.double(), params.double(), "layered", 4, haar))
    assert (RR.expvals(x, params, "layered", 4, haar, True) - RR.expvals(x, params, "layered", 4, haar, False)).abs().max() > 0.1
