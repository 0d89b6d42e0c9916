"""Float64 reference of the classical stages of the step (csrc/qc_mlp.hip): the pre network's angle jets, the post
network's u jets, the PDE residual, the loss parts and, by torch.autograd, the gradient of any cotangent with respect
to every parameter and to the input jets.

Plain torch arithmetic on float64 tensors; nothing here calls the library or the oracle's float32 paths.  Jets are the
six channels {value, d/dt, d/dx, d/dy, d2/dx2, d2/dy2} of the public header, propagated by the chain rule through
Linear -> Tanh -> Linear (tests/test_mlp_reference.py checks them against autograd through torch.nn modules).

Mutations for the negative controls of the GPU tests: ``drop_unit`` removes hidden unit H - 1 from both networks,
``point_mask`` (B,) zeroes the contribution of masked points to every output and gradient.
"""
import numpy as np
import torch

F64 = torch.float64
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "theta")


def layout(H, n, n_theta):
    """name -> (offset, shape) of the flat vector W1[H][3] b1[H] W2[n][H] b2[n] W3[H][n] b3[H] W4[H] b4 theta."""
    out, off = {}, 0
    for name, shape in zip(NAMES, ((H, 3), (H,), (n, H), (n,), (H, n), (H,), (H,), (1,), (n_theta,))):
        out[name] = (off, shape)
        off += int(np.prod(shape))
    return out, off


def unpack(flat, H, n, n_theta):
    """flat (NP,) float32/64 array -> dict of float64 leaf tensors that require grad."""
    lay, NP = layout(H, n, n_theta)
    flat = np.asarray(flat, dtype=np.float64)
    assert flat.shape == (NP,)
    return {k: torch.tensor(flat[o:o + int(np.prod(s))].reshape(s), dtype=F64, requires_grad=True)
            for k, (o, s) in lay.items()}


def flatten(grads, H, n, n_theta, names=NAMES):
    """dict name -> gradient tensor (missing names are zero) -> flat (NP,) float64 numpy vector."""
    lay, NP = layout(H, n, n_theta)
    out = np.zeros(NP)
    for k in names:
        if k in grads and grads[k] is not None:
            o, s = lay[k]
            out[o:o + int(np.prod(s))] = grads[k].detach().numpy().reshape(-1)
    return out


def _unit_mask(H, drop_unit):
    m = torch.ones(H, 1, dtype=F64)
    if drop_unit:
        m[H - 1] = 0.0
    return m


def tanh_jets(g):
    """g: (nch, H, B) jets of the pre-activations -> jets of tanh(g) (second channels: d2 g_k^2 + d1 g_kk)."""
    z = torch.tanh(g[0])
    if g.shape[0] == 1:
        return z[None]
    d1 = 1.0 - z * z
    d2 = -2.0 * z * d1
    return torch.stack([z, d1 * g[1], d1 * g[2], d1 * g[3], d2 * g[2] ** 2 + d1 * g[4], d2 * g[3] ** 2 + d1 * g[5]])


def pre_jets(P, X, nch, drop_unit=False):
    """X (B, 3) float64 -> angle jets (nch, n, B) of Linear(3, H) -> Tanh -> Linear(H, n)."""
    X = torch.as_tensor(X, dtype=F64)
    H = P["b1"].shape[0]
    h0 = P["W1"] @ X.T + P["b1"][:, None]                                       # (H, B)
    if nch == 1:
        g = h0[None]
    else:
        zero = torch.zeros_like(h0)
        g = torch.stack([h0] + [P["W1"][:, k:k + 1].expand_as(h0) for k in range(3)] + [zero, zero])
    z = tanh_jets(g) * _unit_mask(H, drop_unit)
    a = torch.einsum("ih,chb->cib", P["W2"], z)
    return torch.cat([a[:1] + P["b2"][None, :, None], a[1:]])


def hidden_jets(P, qjets, drop_unit=False):
    """qjets (nch, n, B) -> jets of the post network's hidden layer tanh(W3 q + b3), (nch, H, B)."""
    H = P["b3"].shape[0]
    g = torch.einsum("hi,cib->chb", P["W3"], qjets)
    g = torch.cat([g[:1] + P["b3"][None, :, None], g[1:]])
    return tanh_jets(g) * _unit_mask(H, drop_unit)


def post_jets(P, qjets, drop_unit=False, w4=None, b4=None):
    """qjets (nch, n, B) -> u jets (nch, B); w4 (K, H) / b4 (K,) give K outputs, (K, nch, B)."""
    z = hidden_jets(P, qjets, drop_unit)
    if w4 is None:
        u = torch.einsum("h,chb->cb", P["W4"], z)
        return torch.cat([u[:1] + P["b4"], u[1:]])
    u = torch.einsum("kh,chb->kcb", w4, z)
    return torch.cat([u[:, :1] + b4[:, None, None], u[:, 1:]], dim=1)


def residual(ujets, coeffs):
    """c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy) (nn/pde.py:71 with the sigma scalings folded in)."""
    c_t, c_x, c_y, d_xx, d_yy = coeffs
    return c_t * ujets[1] + c_x * ujets[2] + c_y * ujets[3] - (d_xx * ujets[4] + d_yy * ujets[5])


def analytic_u(X):
    X = torch.as_tensor(X, dtype=F64)
    t, x, y = X[:, 0], X[:, 1], X[:, 2]
    return torch.exp(-100.0 * ((x - 0.5) ** 2 + (y - 0.5) ** 2)) * torch.exp(-t)


def analytic_r(X, D, vx, vy):
    X = torch.as_tensor(X, dtype=F64)
    u = analytic_u(X)
    dx, dy = X[:, 1] - 0.5, X[:, 2] - 0.5
    uxx = (40000.0 * dx * dx - 400.0) * u
    uyy = (40000.0 * dy * dy - 400.0) * u
    return -u + vx * (-200.0 * dx * u) + vy * (-200.0 * dy * u) - D * (uxx + uyy)


def analytic_u_diffusion(X, D):
    X = torch.as_tensor(X, dtype=F64)
    t, x, y = X[:, 0], X[:, 1], X[:, 2]
    return torch.sin(np.pi * x) * torch.sin(np.pi * y) * torch.exp(-2.0 * np.pi ** 2 * D * t)


def point_errors(ujets, X, pde, nch):
    """Per-point error e against the analytic target of qc_pde.problem (0 convection-diffusion, 1 pure diffusion)."""
    if nch == 6:
        res = residual(ujets, (pde["c_t"], pde["c_x"], pde["c_y"], pde["d_xx"], pde["d_yy"]))
        target = torch.zeros_like(res) if pde["problem"] == 1 else analytic_r(X, pde["D"], pde["vx"], pde["vy"])
        return res - target
    B = ujets.shape[1]
    seg_a = torch.arange(B) < pde["n_seg_a"]
    if pde["problem"] == 1:
        target = torch.where(seg_a, analytic_u_diffusion(X, pde["D"]), torch.zeros(B, dtype=F64))
    else:
        target = analytic_u(X)
    return ujets[0] - target


def loss_parts(e, pde, nch):
    """(L_r, L_bc, L_ic) of one batch from its per-point errors (segment a = IC points, b = BC points)."""
    e2 = e * e
    if nch == 6:
        return torch.stack([pde["inv_n_res"] * e2.sum(), e2.new_zeros(()), e2.new_zeros(())])
    seg_a = torch.arange(e.shape[0]) < pde["n_seg_a"]
    return torch.stack([e2.new_zeros(()), pde["inv_n_b"] * e2[~seg_a].sum(), pde["inv_n_a"] * e2[seg_a].sum()])


def point_weights(B, pde, nch):
    """d loss / d e per unit error (the 2 * weight / N of qc_pde): w_res, or w_val_a / w_val_b by segment."""
    if nch == 6:
        return torch.full((B,), pde["w_res"], dtype=F64)
    seg_a = torch.arange(B) < pde["n_seg_a"]
    return torch.where(seg_a, torch.tensor(pde["w_val_a"], dtype=F64), torch.tensor(pde["w_val_b"], dtype=F64))


def tile_grads(objective_per_point, wrt, B, tile=64):
    """Gradients of the per-tile sums of a per-point objective (B,): a list, one entry per 64-point tile, of the
    gradients w.r.t. each tensor of ``wrt`` (None -> zeros)."""
    out = []
    tiles = (B + tile - 1) // tile
    for k in range(tiles):
        s = objective_per_point[k * tile:(k + 1) * tile].sum()
        g = torch.autograd.grad(s, wrt, retain_graph=True, allow_unused=True)
        out.append([torch.zeros_like(w) if gi is None else gi for gi, w in zip(g, wrt)])
    return out
