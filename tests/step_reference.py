"""Float64 reference of the fused training step's [grad | L_r, L_bc, L_ic] vector (qc_fused_pinn_residual_step,
QC_PHASE_GRADS): the classical stages of tests/mlp_reference.py composed with the circuit oracle (oracle/jets.py for the
residual points' six channels, oracle/statevector.py for the value points), differentiated by torch.autograd.

The loss is the trainer's 2 L_r + 4 L_bc + 2 L_ic (trainer/diffusion_train.py:47) on the convection-diffusion operator
with D = 0.01, v = (1, 1) and unit sigmas, the problem the library's step solves by default.  An empty point set
contributes 0 to the loss and to its part, as the step reports it.

``cached_step_reference`` wraps the reference in conftest.cached_oracle: the records of the seeded GPU cases are
committed under tests/golden/oracle/ (tests/golden/make_oracle_cache.py regenerates them), so no GPU run pays for the
oracle.  ``step_inputs`` draws the weights and points of those cases from a seeded CPU generator, so the inputs, and
with them the records' digests, do not depend on a device.
"""
import numpy as np
import torch

import mlp_reference as R
from conftest import cached_oracle, pkg

PDE = dict(c_t=1.0, c_x=1.0, c_y=1.0, d_xx=0.01, d_yy=0.01, D=0.01, vx=1.0, vy=1.0, problem=0)


def reference_loss(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, drop_unit=False,
                   encoding="angle"):
    """flat (NP,) weights in model.parameters() order and three (B, 3) point sets -> (grad (NP,), parts (3,)) float64:
    the gradient of 2 L_r + 4 L_bc + 2 L_ic and (L_r, L_bc, L_ic)."""
    from oracle import jets as oj
    from oracle import statevector as sv
    P = R.unpack(flat, H, n, n_theta)
    theta = P["theta"].reshape(theta_shape)
    zero = torch.zeros((), dtype=R.F64)
    l_r = zero
    if len(X_res):
        a = R.pre_jets(P, X_res, 6, drop_unit)
        q = oj.qjets_from_ajets(a, theta, ansatz, n, haar, encoding)
        u = R.post_jets(P, q, drop_unit)
        l_r = (R.point_errors(u, X_res, PDE, 6) ** 2).mean()
    out = []
    for Xv in (X_bc, X_ic):
        if not len(Xv):
            out.append(zero)
            continue
        av = R.pre_jets(P, Xv, 1, drop_unit)
        qv = sv.circuit_expvals(av[0].T, theta, ansatz, n, haar, encoding)[None]
        uv = R.post_jets(P, qv, drop_unit)
        out.append(((uv[0] - R.analytic_u(Xv)) ** 2).mean())
    l_bc, l_ic = out
    loss = 2.0 * l_r + 4.0 * l_bc + 2.0 * l_ic
    grads = torch.autograd.grad(loss, [P[k] for k in R.NAMES], allow_unused=True)
    return R.flatten(dict(zip(R.NAMES, grads)), H, n, n_theta), np.array([l_r.item(), l_bc.item(), l_ic.item()])


def layout_from_fixture(z, prefix, H, n, n_theta):
    """The flat weight vector of a reference fixture's ``<prefix>`` state (model.parameters() order)."""
    names = ("preprocessor__0__weight", "preprocessor__0__bias", "preprocessor__2__weight", "preprocessor__2__bias",
             "postprocessor__0__weight", "postprocessor__0__bias", "postprocessor__2__weight", "postprocessor__2__bias",
             "quantum_layer__params")
    flat = np.concatenate([np.asarray(z[prefix + k], dtype=np.float32).reshape(-1) for k in names])
    assert flat.size == R.layout(H, n, n_theta)[1]
    return flat


def step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt):
    """Seeded CPU draw of one case: flat float32 weights (initialiser-like scales; theta wide enough that the circuit
    gradient is not small) and float32 IC / BC / domain points in the trainer's boxes."""
    from oracle import solver as osol
    g = torch.Generator().manual_seed(1000 * salt + 7 * n + B_res + 3 * n_ic + 5 * n_bc)
    lay, NP = R.layout(H, n, n_theta)
    scale = {"W1": np.sqrt(2.0 / (H + 3)), "b1": 0.1, "W2": np.sqrt(2.0 / (H + n)), "b2": 0.1,
             "W3": 1.0 / np.sqrt(n), "b3": 0.3, "W4": 1.0 / np.sqrt(H), "b4": 0.1, "theta": 0.8}
    flat = np.zeros(NP, dtype=np.float32)
    for k, (o, s) in lay.items():
        m = int(np.prod(s))
        flat[o:o + m] = (torch.randn(m, generator=g, dtype=torch.float64) * scale[k]).numpy()
    X_ic, X_bc, X_res = [(torch.tensor(b[0]) + (torch.tensor(b[1]) - torch.tensor(b[0])) * torch.rand(m, 3, generator=g))
                         .to(torch.float32)
                         for b, m in ((osol.BOX_IC, n_ic), (osol.BOX_BC1, n_bc), (osol.BOX_DOM, B_res))]
    return flat, X_ic, X_bc, X_res


def haar_for(n, seed):
    """The oracle's fixed two-wire unitaries of a seeded layer (present for n >= 4), or None."""
    from oracle import statevector as sv
    return sv.haar_pair(seed, seed + 1) if (seed is not None and n >= 4) else None


def step_key(ansatz, n, L, seed, encoding, B_res, n_ic, n_bc, variant=""):
    return f"step_{ansatz}_n{n}_L{L}_s{seed}_{encoding}_r{B_res}_i{n_ic}_b{n_bc}" + (f"_{variant}" if variant else "")


def cached_step_reference(ansatz, n, L, seed, encoding, flat, X_ic, X_bc, X_res, H=50, variant=""):
    """reference_loss of one case through conftest.cached_oracle -> {"grad": (NP,), "parts": (3,)}.

    ``variant``: a negative control of the GPU tests.  "drop_res" / "drop_val" drop the last residual / value point
    (the value point is the last BC point, or the last IC point when there are no BC points); "swap_haar" swaps the
    two fixed unitaries."""
    P = int(pkg("circuits").params_per_layer(ansatz, n))
    n_theta, theta_shape = L * P, (L, P)
    haar = haar_for(n, seed)
    Xi, Xb, Xr = X_ic, X_bc, X_res
    if variant == "drop_res":
        Xr = X_res[:-1]
    elif variant == "drop_val":
        if len(X_bc):
            Xb = X_bc[:-1]
        else:
            Xi = X_ic[:-1]
    elif variant == "swap_haar":
        haar = (haar[1], haar[0])
    elif variant:
        raise ValueError(variant)

    def compute():
        g, parts = reference_loss(flat, H, n, n_theta, theta_shape, ansatz, haar,
                                  *(torch.as_tensor(x).double() for x in (Xi, Xb, Xr)), encoding=encoding)
        return {"grad": g, "parts": parts}
    flat = np.asarray(flat, dtype=np.float32)
    theta = flat[R.layout(H, n, n_theta)[0]["theta"][0]:]
    inputs = (flat, theta) + tuple(np.asarray(x, dtype=np.float32) for x in (X_ic, X_bc, X_res))
    return cached_oracle(step_key(ansatz, n, L, seed, encoding, len(X_res), len(X_ic), len(X_bc), variant), inputs,
                         compute)
