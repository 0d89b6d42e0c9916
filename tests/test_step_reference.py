"""The fused step's float64 reference (tests/step_reference.py) against fixtures the REFERENCE's own nn/pde.py and
trainer produced (tests/golden/make_golden.py): before any GPU test trusts the composed reference, it must reproduce
them.

operator_*: 2 x MSE of the diffusion operator's residual on one batch, so residual points only, and loss = 2 L_r.
train_cascade_n4_b64: the first step's raw gradient and loss parts on its first batch, all three point sets.

The fixtures are float32 (the reference model runs in fp32).  Observed max |ref - fixture| / max(1, max |fixture|):
2e-8 to 6e-8 on the gradients, 4e-8 to 7e-8 on the losses; the bound below is 1e-5."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg
from step_reference import haar_for, layout_from_fixture, reference_loss

TOL = 1e-5

OPERATORS = [("cascade_n4", "cascade", 4, 1), ("cross_mesh_n4", "cross_mesh", 4, 1), ("layered_n8", "layered", 8, 2)]


def _case(ansatz, n, L):
    P = pkg("circuits").params_per_layer(ansatz, n)
    return L * P, (L, P)


@pytest.mark.parametrize("tag,ansatz,n,L", OPERATORS, ids=[o[0] for o in OPERATORS])
def test_reference_reproduces_operator_fixture(tag, ansatz, n, L):
    z = np.load(os.path.join(GOLDEN, f"operator_{tag}.npz"))
    n_theta, theta_shape = _case(ansatz, n, L)
    flat = layout_from_fixture(z, "w__", 50, n, n_theta)
    X = torch.from_numpy(z["X"]).double()
    none = X[:0]
    g, parts = reference_loss(flat, 50, n, n_theta, theta_shape, ansatz, haar_for(n, 1), none, none, X)
    scale = max(1.0, np.abs(z["grad"]).max())
    assert np.abs(g - z["grad"]).max() < TOL * scale, np.abs(g - z["grad"]).max() / scale
    assert abs(2.0 * parts[0] - float(z["loss"])) < TOL * max(1.0, float(z["loss"]))
    assert parts[1] == 0.0 and parts[2] == 0.0
    # the reference with the last point dropped is told apart at this tolerance
    gd, _ = reference_loss(flat, 50, n, n_theta, theta_shape, ansatz, haar_for(n, 1), none, none, X[:-1])
    assert np.abs(gd - z["grad"]).max() > 100 * TOL * scale


def test_reference_reproduces_first_training_step():
    z = np.load(os.path.join(GOLDEN, "train_cascade_n4_b64.npz"))
    n_theta, theta_shape = _case("cascade", 4, 1)
    flat = layout_from_fixture(z, "w0__", 50, 4, n_theta)
    Xs = [torch.from_numpy(z[k][0]).double() for k in ("X_ic", "X_bc", "X_res")]
    g, parts = reference_loss(flat, 50, 4, n_theta, theta_shape, "cascade", haar_for(4, 1), *Xs)
    scale = max(1.0, np.abs(z["grad_raw0"]).max())
    assert np.abs(g - z["grad_raw0"]).max() < TOL * scale, np.abs(g - z["grad_raw0"]).max() / scale
    ref = z["parts"][0]                                          # loss, l_r, l_bc, l_ic
    assert np.abs(parts - ref[1:]).max() < TOL * max(1.0, np.abs(ref).max())
    assert abs(float(np.dot([2.0, 4.0, 2.0], parts)) - ref[0]) < TOL * max(1.0, ref[0])


def test_empty_point_sets_contribute_nothing():
    """An empty set adds 0 to the loss and its part: the three pipelines add up to the whole step."""
    from step_reference import step_inputs
    n_theta, theta_shape = _case("cascade", 4, 1)
    flat, X_ic, X_bc, X_res = step_inputs(50, 4, n_theta, 5, 3, 4, 0)
    Xs = [x.double() for x in (X_ic, X_bc, X_res)]
    none = Xs[0][:0]
    args = (flat, 50, 4, n_theta, theta_shape, "cascade", haar_for(4, 1))
    g, p = reference_loss(*args, *Xs)
    parts = [reference_loss(*args, *(x if i == k else none for i, x in enumerate(Xs))) for k in range(3)]
    assert np.abs(sum(q[0] for q in parts) - g).max() < 1e-12 * np.abs(g).max()
    assert np.abs(sum(q[1] for q in parts) - p).max() < 1e-14
    assert parts[0][1][0] == 0 and parts[0][1][1] == 0 and parts[2][1][1] == 0 and parts[2][1][2] == 0
