"""The Fourier-feature input encoding without a GPU: the closed-form channels of tests/fourier_reference.py against torch
double autograd, the flat layout with ``n_in`` input columns, the ``FourierFeatures`` module, what the ``args`` keys do to a
``DVPDESolver`` (and that a model without them is the parent's, bit for bit), the checkpoint, and the argument errors of the
new entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fourier_reference as FR
import mlp_reference as R
from conftest import pkg
from test_gpu_fullsize import Log, base_args


def _case(m, H, n, B, scale, seed):
    g = torch.Generator().manual_seed(seed)
    Bf = torch.randn(3, m, generator=g, dtype=torch.float64) * scale
    X = torch.rand(B, 3, generator=g, dtype=torch.float64)
    lay, NP = FR.layout(H, n, 2, 2 * m)
    flat = torch.randn(NP, generator=g, dtype=torch.float64).numpy() / math.sqrt(2 * m)
    return Bf, X, FR.unpack(flat, H, n, 2, m)


@pytest.mark.parametrize("m,H,scale", [(1, 1, 1.0), (3, 5, 2.0), (8, 4, 10.0)])
def test_closed_form_channels_match_double_autograd(m, H, scale):
    """h, h_t, h_x, h_y, h_xx, h_yy of every hidden unit, and the angle jets built on them, against autograd through
    the formula gamma(X) = [sin(2 pi X B), cos(2 pi X B)]."""
    n, B = 3, 7
    Bf, X, P = _case(m, H, n, B, scale, seed=11 * m + H)
    Xg = X.clone().requires_grad_(True)

    def channels(f):                   # f: (B, K) differentiable in Xg -> (6, K, B) by autograd
        out = [f.T]
        K = f.shape[1]
        first = [torch.stack([torch.autograd.grad(f[:, k].sum(), Xg, create_graph=True)[0][:, c] for k in range(K)]) for c in range(3)]
        out += first
        for c in (1, 2):
            out.append(torch.stack([torch.autograd.grad(first[c][k].sum(), Xg, retain_graph=True)[0][:, c] for k in range(K)]))
        return torch.stack(out).detach()

    h = FR.features(Bf, Xg) @ P["W1"].T + P["b1"]
    want_h = channels(h)
    got_h = FR.hidden_pre_jets(P, Bf, X, 6).detach()
    assert (got_h - want_h).abs().max() < 1e-10 * max(1.0, want_h.abs().max()), (got_h - want_h).abs().max()
    a = torch.tanh(h) @ P["W2"].T + P["b2"]
    want_a = channels(a)
    got_a = FR.pre_jets_ff(P, Bf, X, 6).detach()
    assert (got_a - want_a).abs().max() < 1e-10 * max(1.0, want_a.abs().max())
    assert (FR.pre_jets_ff(P, Bf, X, 1).detach() - want_a[:1]).abs().max() < 1e-12
    # the angle map on top, against autograd through pi tanh
    want_m = channels(math.pi * torch.tanh(a))
    got_m = FR.pre_jets_ff(P, Bf, X, 6, angle_map=True).detach()
    assert (got_m - want_m).abs().max() < 1e-10 * max(1.0, want_m.abs().max())
    # the control of the GPU tests changes the result
    assert (FR.pre_jets_ff(P, Bf, X, 6, drop_freq=True).detach() - want_a).abs().max() > 1e-3


def test_reverse_formulas_match_double_autograd():
    """dP_j = sum (s_j alpha_j + c_j beta_j), dQ_j = sum (c_j alpha_j - s_j beta_j) with alpha_j = hb - w_jx^2 hb_xx - w_jy^2
    hb_yy and beta_j = w_jt hb_t + w_jx hb_x + w_jy hb_y: the reverse pass of the kernel, stated here, against autograd."""
    m, H, B = 5, 3, 9
    Bf, X, P = _case(m, H, 2, B, 3.0, seed=5)
    hb = torch.randn(6, H, B, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    hj = FR.hidden_pre_jets(P, Bf, X, 6)
    want = torch.autograd.grad((hb * hj).sum(), P["W1"])[0]
    r = (X @ Bf).T
    s, c, w = torch.sin(2 * math.pi * r), torch.cos(2 * math.pi * r), 2 * math.pi * Bf
    al = hb[0][:, None] - (w[1] ** 2)[None, :, None] * hb[4][:, None] - (w[2] ** 2)[None, :, None] * hb[5][:, None]      # (H, m, B)
    be = w[0][None, :, None] * hb[1][:, None] + w[1][None, :, None] * hb[2][:, None] + w[2][None, :, None] * hb[3][:, None]
    got = torch.cat([(s * al + c * be).sum(-1), (c * al - s * be).sum(-1)], dim=1)
    assert (got - want).abs().max() < 1e-10 * max(1.0, want.abs().max())


def test_param_layout_with_input_columns():
    engine = pkg("hip.engine")
    H, n, n_theta = 7, 3, 5
    plain = engine.param_layout(H, n, n_theta)
    assert engine.param_layout(H, n, n_theta, n_in=3) == plain
    for m in (1, 8, 64):
        lay = engine.param_layout(H, n, n_theta, n_in=2 * m)
        shift = (2 * m - 3) * H
        assert lay["preprocessor.0.weight"] == (0, (H, 2 * m))
        for k, (off, shape) in plain.items():
            if k != "preprocessor.0.weight":
                assert lay[k] == (off + shift, shape), k
        ref, NP = FR.layout(H, n, n_theta, 2 * m)
        assert NP == lay["__total__"][0]
        names = [k for k in plain if k != "__total__"]
        assert [lay[k][0] for k in names] == [ref[k][0] for k in R.NAMES]
    K2 = engine.param_layout(H, n, n_theta, 2, n_in=10)
    assert K2["postprocessor.2.weight"][1] == (2, H) and K2["__total__"][0] == plain["__total__"][0] + 7 * H + H + 1


def test_fourier_features_module_is_the_formula():
    FF = pkg("nn.fourier").FourierFeatures
    torch.manual_seed(3)
    ff = FF(3, 6, scale=2.5)
    torch.manual_seed(3)
    want_B = torch.randn(3, 6) * 2.5
    assert torch.equal(ff.B, want_B) and "B" in dict(ff.named_buffers()) and not list(ff.parameters())
    X = torch.rand(10, 3)
    got = ff(X)
    proj = 2 * math.pi * (X.double() @ want_B.double())
    want = torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1)
    assert got.shape == (10, 12) and (got.double() - want).abs().max() < 1e-5
    assert (ff(X.double()) - want).abs().max() < 1e-12
    assert (FR.features(want_B, X.double()) - want).abs().max() < 1e-12
    with pytest.raises(ValueError):
        FF(3, 0)


def _parent_flat(args, seed):
    """The flat vector of the model as the code before this feature built it: the same modules in the same order."""
    DVQ = pkg("nn.DVQuantumLayer").DVQuantumLayer
    nn = torch.nn
    torch.manual_seed(seed)
    cn, H, n = args["classic_network"], args["classic_network"][-2], args["num_qubits"]
    pre = nn.Sequential(nn.Linear(cn[0], H), nn.Tanh(), nn.Linear(H, n))
    post = nn.Sequential(nn.Linear(n, H), nn.Tanh(), nn.Linear(H, cn[-1]))
    q = DVQ(args)
    for layer in pre:
        if isinstance(layer, nn.Linear):
            nn.init.xavier_normal_(layer.weight)
            nn.init.zeros_(layer.bias)
    return torch.cat([p.detach().reshape(-1) for mod in (pre, post, q) for p in mod.parameters()])


@pytest.mark.parametrize("extra", [{}, {"fourier_features": 0}, {"fourier_features": 0, "fourier_scale": 7.0}])
def test_model_without_the_key_is_the_parents(extra):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    args = base_args(classic_network=[3, 9, 1], **extra)
    torch.manual_seed(4)
    model = Solver(args, Log(), device=torch.device("cpu"))
    assert model.fourier is None and not list(model.buffers())
    want = _parent_flat(args, 4)
    assert model._flat is not None and torch.equal(model._flat, want)
    assert [k for k in model.state_dict() if "fourier" in k] == []


def test_model_with_the_key():
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    engine = pkg("hip.engine")
    m, H = 5, 9
    args = base_args(classic_network=[3, H, 1], fourier_features=m, fourier_scale=3.0)
    torch.manual_seed(4)
    model = Solver(args, Log(), device=torch.device("cpu"))
    torch.manual_seed(4)
    assert torch.equal(model.fourier.B, torch.randn(3, m) * 3.0)          # created before the preprocessor
    assert model.preprocessor[0].weight.shape == (H, 2 * m)
    n_theta = model.quantum_layer.params.numel()
    assert model._flat.numel() == engine.param_layout(H, 4, n_theta, n_in=2 * m)["__total__"][0]
    assert model._packed_ok()
    assert "fourier.B" in model.state_dict() and "fourier.B" not in dict(model.named_parameters())
    # two inputs: in_dim stays 3 with a zero t row; the first layer is not padded
    two = Solver(base_args(classic_network=[2, H, 1], fourier_features=m), Log(), device=torch.device("cpu"))
    assert two.fourier.B.shape == (3, m) and (two.fourier.B[0] == 0).all() and (two.fourier.B[1:] != 0).all()
    assert two._flat.numel() == model._flat.numel()
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            Solver(base_args(fourier_features=bad), Log(), device=torch.device("cpu"))


def test_state_dict_round_trip_keeps_B(tmp_path):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    args = base_args(classic_network=[3, 6, 1], fourier_features=4, fourier_scale=2.0)
    torch.manual_seed(1)
    a = Solver(args, Log(), device=torch.device("cpu"))
    torch.manual_seed(2)
    b = Solver(args, Log(), device=torch.device("cpu"))
    assert not torch.equal(a.fourier.B, b.fourier.B)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.fourier.B, b.fourier.B)
    a.log_path = str(tmp_path)
    a.save_state()
    ck = Solver.load_state(str(tmp_path / "model.pth"))
    assert torch.equal(ck["fourier"]["B"], a.fourier.B)
    assert ck["preprocessor"]["0.weight"].shape == (6, 8)
    # a model without a map: no key in the checkpoint, and its state loads as before
    plain = Solver(base_args(classic_network=[3, 6, 1]), Log(), device=torch.device("cpu"))
    plain.log_path = str(tmp_path)
    plain.save_state(str(tmp_path / "plain.pth"))
    ck = Solver.load_state(str(tmp_path / "plain.pth"))
    assert "fourier" not in ck
    other = Solver(base_args(classic_network=[3, 6, 1]), Log(), device=torch.device("cpu"))
    other.load_state_dict(plain.state_dict())


def test_argument_errors_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    QC_ERR_ARG = -1
    assert L.QC_FF_MAX == 64
    freq = (ctypes.c_float * (3 * 70))()
    assert lib.qc_program_set_input_map(None, freq, 4) == QC_ERR_ARG
    assert lib.qc_program_set_input_map(None, None, 0) == QC_ERR_ARG
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    f = ctypes.addressof(freq)
    fwd = lambda H, n, m, B, nch, fq=f, X=p: lib.qc_pre_forward_ff(X, p, H, n, 0, 0, fq, m, p, B, nch, None)
    bwd = lambda H, n, m, B, nch, stride, fq=f: lib.qc_pre_backward_ff(p, p, H, n, 0, 0, fq, m, None, p, p, stride, 0, B, nch, None)
    for m in (0, -1, 65):
        assert fwd(4, 2, m, 8, 6) == QC_ERR_ARG
        assert bwd(4, 2, m, 8, 6, 4096) == QC_ERR_ARG
    assert fwd(4, 2, 4, 8, 6, fq=None) == QC_ERR_ARG and fwd(4, 2, 4, 8, 6, X=None) == QC_ERR_ARG
    for H, n, B, nch in ((0, 2, 8, 6), (1025, 2, 8, 6), (4, 17, 8, 6), (4, 2, 0, 6), (4, 2, 8, 3)):      # the _map forms' limits
        assert fwd(H, n, 4, B, nch) == QC_ERR_ARG
        assert bwd(H, n, 4, B, nch, 4096) == QC_ERR_ARG
    NP = FR.layout(4, 2, 0, 8)[1]
    assert bwd(4, 2, 4, 8, 6, NP - 1) == QC_ERR_ARG          # a row shorter than the layout with 2m input columns
    assert lib.qc_pre_backward_ff(p, p, 4, 2, 0, 1, f, 4, None, p, p, 4096, 0, 8, 6, None) == QC_ERR_ARG   # map without angle jets
