"""The float64 reference of the network stages (tests/mlp_reference.py) against plain autograd through torch.nn modules:
its jets against torch.autograd.grad(create_graph=True) derivatives of the modules w.r.t. (t, x, y), its layout against
hip/engine.py:param_layout, and its gradients against loss.backward() through the modules.  The GPU tests of
qc_pre_* / qc_post* rest on this helper."""
import numpy as np
import pytest
import torch

import mlp_reference as R
from conftest import pkg


def _modules(H, n, seed):
    torch.manual_seed(seed)
    pre = torch.nn.Sequential(torch.nn.Linear(3, H), torch.nn.Tanh(), torch.nn.Linear(H, n)).double()
    post = torch.nn.Sequential(torch.nn.Linear(n, H), torch.nn.Tanh(), torch.nn.Linear(H, 1)).double()
    return pre, post


def _flat(pre, post, theta):
    return torch.cat([p.detach().reshape(-1) for p in (*pre.parameters(), *post.parameters())] + [theta]).numpy()


def _autograd_jets(f, X):
    """Six channels of f: (B, 3) -> (B, k) per point, by autograd.grad(create_graph=True) as nn/pde.py:59-70 does."""
    X = X.clone().requires_grad_(True)
    out = f(X)
    chans = [out]
    d1 = [torch.stack([torch.autograd.grad(out[:, j].sum(), X, create_graph=True)[0][:, k] for j in range(out.shape[1])], 1)
          for k in range(3)]
    chans += d1
    for k in (1, 2):
        chans.append(torch.stack([torch.autograd.grad(d1[k][:, j].sum(), X, create_graph=True)[0][:, k]
                                  for j in range(out.shape[1])], 1))
    return torch.stack(chans)                                    # (6, B, k)


@pytest.mark.parametrize("H,n", [(1, 1), (5, 3), (50, 4), (65, 16)])
def test_reference_jets_and_gradients_match_torch_modules(H, n):
    pre, post = _modules(H, n, seed=H + n)
    n_theta = 3
    theta = torch.randn(n_theta, dtype=torch.float64)
    flat = _flat(pre, post, theta)
    lay = pkg("hip.engine").param_layout(H, n, n_theta)
    mine, NP = R.layout(H, n, n_theta)
    assert NP == lay["__total__"][0] == flat.size
    assert [v[0] for v in mine.values()] == [lay[k][0] for k in lay if k != "__total__"]
    P = R.unpack(flat, H, n, n_theta)
    g = torch.Generator().manual_seed(7)
    X = torch.rand(37, 3, generator=g, dtype=torch.float64)

    # pre network: angle jets, 6 and 1 channels
    want = _autograd_jets(pre, X).permute(0, 2, 1)               # (6, n, B)
    got = R.pre_jets(P, X, 6)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    assert torch.allclose(R.pre_jets(P, X, 1), want[:1], rtol=0, atol=1e-12)

    # post network on the composition: u(t, x, y) = post(pre(X)) (a stand-in circuit: the identity)
    want_u = _autograd_jets(lambda Z: post(pre(Z)), X)[:, :, 0]   # (6, B)
    got_u = R.post_jets(P, R.pre_jets(P, X, 6))
    assert torch.allclose(got_u, want_u, rtol=0, atol=1e-11)

    # gradients of a loss of the residual and the value through the modules vs the reference's autograd
    pde = dict(c_t=1.3, c_x=0.7, c_y=-0.4, d_xx=0.02, d_yy=0.05, D=0.01, vx=1.0, vy=1.0, problem=0)
    coeffs = (pde["c_t"], pde["c_x"], pde["c_y"], pde["d_xx"], pde["d_yy"])
    for m in (*pre.parameters(), *post.parameters()):
        m.grad = None
    res_t = R.residual(want_u, coeffs)
    loss_t = ((res_t - R.analytic_r(X, 0.01, 1.0, 1.0)) ** 2).mean() + (want_u[0] ** 2).sum()
    loss_t.backward()
    want_g = np.concatenate([p.grad.reshape(-1).numpy() for p in (*pre.parameters(), *post.parameters())] + [np.zeros(n_theta)])
    u = R.post_jets(P, R.pre_jets(P, X, 6))
    e = R.point_errors(u, X, pde, 6)
    loss = (e ** 2).mean() + (u[0] ** 2).sum()
    names = R.NAMES[:-1]
    grads = torch.autograd.grad(loss, [P[k] for k in names])
    got_g = R.flatten(dict(zip(names, grads)), H, n, n_theta)
    assert np.abs(got_g - want_g).max() < 1e-10 * max(1.0, np.abs(want_g).max())

    # the mutations of the GPU tests' negative controls change the outputs
    assert (R.post_jets(P, R.pre_jets(P, X, 6), drop_unit=True) - got_u).abs().max() > 1e-6


def test_solver_refuses_network_shapes_the_kernels_do_not_serve(tmp_path):
    """The network kernels serve 1 <= n <= 16 qubits and 1 <= H <= 1024 hidden units (check_mlp); the circuit families
    go to 20 qubits.  A DVPDESolver outside the network range must fail at construction, naming the limit."""
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    from test_modules_cpu import Log, base_args
    with pytest.raises(ValueError, match="at most 16 qubits"):
        Solver(base_args(num_qubits=17, q_ansatz="cross_mesh"), Log(tmp_path), device=torch.device("cpu"))
    with pytest.raises(ValueError, match=r"1 \.\. 1024 hidden units"):
        Solver(base_args(classic_network=[3, 1025, 1]), Log(tmp_path), device=torch.device("cpu"))
    Solver(base_args(num_qubits=16, q_ansatz="cross_mesh", classic_network=[3, 1024, 1]), Log(tmp_path),
           device=torch.device("cpu"))
