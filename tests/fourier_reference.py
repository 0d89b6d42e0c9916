"""Reference of the pre network behind a Fourier-feature input map (csrc/qc_mlp.hip, k_pre_ff_*) and of the fused step
that trains it: gamma(X) = [sin(2 pi X B), cos(2 pi X B)] -> Linear(2m, H) -> Tanh -> Linear(H, n) -> circuit -> post network.

Plain torch arithmetic in the dtype of its inputs: float64 is the reference, and the same functions on float32 tensors are
the yardstick of the tolerance (``gap_tolerance``): a correct fp32 kernel differs from another correct fp32 evaluation by a
small multiple of their common distance to the truth.  Nothing here calls the library.

Jets are the six channels {value, d/dt, d/dx, d/dy, d2/dx2, d2/dy2} of the public header.  ``feature_jets`` states them in
closed form (tests/test_fourier_cpu.py checks the closed form against double autograd); from the pre-activations on the
code is tests/mlp_reference.py (``tanh_jets``, the W2 step).

``drop_freq``: the negative control of the GPU tests, the last frequency's two weight columns (sine and cosine) zeroed."""
import math

import numpy as np
import torch

import mlp_reference as R
import step_reference as S

F64 = torch.float64
NAMES = R.NAMES
ULP32 = 2.0 ** -23


def layout(H, n, n_theta, n_in=3, K=1):
    """name -> (offset, shape) of the flat vector W1[H][n_in] b1 W2 b2 | W3 b3 W4[K][H] b4[K] | theta, and its length."""
    out, off = {}, 0
    shapes = ((H, n_in), (H,), (n, H), (n,), (H, n), (H,), (H,) if K == 1 else (K, H), (K,), (n_theta,))
    for name, shape in zip(NAMES, shapes):
        out[name] = (off, shape)
        off += int(np.prod(shape))
    return out, off


def unpack(flat, H, n, n_theta, m, dtype=F64, grad=True):
    """flat (NP,) -> dict of leaf tensors of ``dtype`` (W1 is (H, 2m))."""
    lay, NP = layout(H, n, n_theta, 2 * m)
    flat = np.asarray(flat)
    assert flat.shape == (NP,)
    return {k: torch.tensor(np.asarray(flat[o:o + int(np.prod(s))].reshape(s), dtype=np.float64), dtype=dtype, requires_grad=grad)
            for k, (o, s) in lay.items()}


def features(Bf, X):
    """gamma(X) (B, 2m) by the formula, in the dtype of X."""
    turns = X @ Bf.to(X.dtype)
    return torch.cat([torch.sin(2.0 * math.pi * turns), torch.cos(2.0 * math.pi * turns)], dim=-1)


def feature_jets(Bf, X, nch):
    """Closed-form jets of gamma, (nch, 2m, B): with r_j = sum_k B_kj X_k, s = sin 2 pi r, c = cos 2 pi r, w_jk = 2 pi B_kj,
    value [s; c], first derivatives [w_k c; -w_k s], second derivatives [-w_k^2 s; -w_k^2 c]."""
    Bf = Bf.to(X.dtype)
    r = (X @ Bf).T                                              # (m, B), turns
    s, c = torch.sin(2.0 * math.pi * r), torch.cos(2.0 * math.pi * r)
    g = [torch.cat([s, c])]
    if nch == 6:
        w = 2.0 * math.pi * Bf                                  # (3, m)
        for k in range(3):
            g.append(torch.cat([w[k][:, None] * c, -w[k][:, None] * s]))
        for k in (1, 2):
            g.append(torch.cat([-(w[k] ** 2)[:, None] * s, -(w[k] ** 2)[:, None] * c]))
    return torch.stack(g)


def hidden_pre_jets(P, Bf, X, nch, drop_freq=False):
    """Jets of the pre-activations h = W1 gamma + b1, (nch, H, B): h = b1 + sum_j A_j, h_k = sum_j w_jk D_j, h_kk = -sum_j
    w_jk^2 A_j with A_j = P_j s_j + Q_j c_j and D_j = P_j c_j - Q_j s_j."""
    W1 = P["W1"]
    m = W1.shape[1] // 2
    if drop_freq:
        keep = torch.ones(2 * m, dtype=W1.dtype)
        keep[m - 1] = keep[2 * m - 1] = 0.0
        W1 = W1 * keep
    h = torch.einsum("hf,cfb->chb", W1, feature_jets(Bf, X, nch))
    return torch.cat([h[:1] + P["b1"][None, :, None], h[1:]])


def pre_jets_ff(P, Bf, X, nch, drop_freq=False, angle_map=False):
    """X (B, 3) -> angle jets (nch, n, B) of gamma -> Linear(2m, H) -> Tanh -> Linear(H, n) [-> pi tanh]."""
    z = R.tanh_jets(hidden_pre_jets(P, Bf, X, nch, drop_freq))
    a = torch.einsum("ih,chb->cib", P["W2"], z)
    a = torch.cat([a[:1] + P["b2"][None, :, None], a[1:]])
    if angle_map:
        tau = torch.tanh(a[0])
        ps = math.pi * (1.0 - tau * tau)
        out = [math.pi * tau]
        if nch == 6:
            out += [ps * a[1], ps * a[2], ps * a[3], ps * (a[4] - 2.0 * tau * a[2] ** 2), ps * (a[5] - 2.0 * tau * a[3] ** 2)]
        a = torch.stack(out)
    return a


def gap_tolerance(f32, f64, want=None, factor=4.0, floor_ulps=4.0):
    """The tolerance of one compared quantity: ``factor`` x the largest distance between the float32 restatement and the
    float64 reference, and never less than ``floor_ulps`` fp32 ulps of the quantity's largest magnitude."""
    f32, f64 = np.asarray(f32, np.float64), np.asarray(f64, np.float64)
    want = f64 if want is None else np.asarray(want, np.float64)
    gap = float(np.abs(f32 - f64).max()) if f64.size else 0.0
    floor = floor_ulps * ULP32 * (float(np.abs(want).max()) if want.size else 0.0)
    return max(factor * gap, floor), gap


class FStep(S.Step):
    """``step_reference.Step`` with the map in front of the pre network: the same composition (circuit oracle, post
    network, ``losses`` / ``grad`` / ``weighted``), restated because ``Step`` lays W1 out as [H][3].  ``Bf`` None: the plain
    pre network on the plain layout (the control of the training replay)."""

    def __init__(self, flat, H, n, n_theta, theta_shape, ansatz, haar, Bf, X_ic, X_bc, X_res, drop_freq=False, encoding="angle"):
        from oracle import jets as oj
        from oracle import statevector as sv
        if Bf is None:
            self.P = P = S.unpack(flat, H, n, n_theta)
            pre = lambda X, nch: R.pre_jets(P, X, nch)
        else:
            Bf = torch.as_tensor(np.asarray(Bf), dtype=F64)
            self.P = P = unpack(flat, H, n, n_theta, Bf.shape[1])
            pre = lambda X, nch: pre_jets_ff(P, Bf, torch.as_tensor(np.asarray(X), dtype=F64), nch, drop_freq)
        self.leaves = [P[k] for k in NAMES]
        theta = P["theta"].reshape(theta_shape)
        self.u_res = None
        if len(X_res):
            q = oj.qjets_from_ajets(pre(X_res, 6), theta, ansatz, n, haar, encoding)
            self.u_res = R.post_jets(P, q)
        vals = []
        for Xv in (X_bc, X_ic):
            if not len(Xv):
                vals.append(None)
                continue
            qv = sv.circuit_expvals(pre(Xv, 1)[0].T, theta, ansatz, n, haar, encoding)[None]
            vals.append(R.post_jets(P, qv)[0])
        self.u_bc, self.u_ic = vals


def reference_loss(flat, H, n, n_theta, theta_shape, ansatz, haar, Bf, X_ic, X_bc, X_res, drop_freq=False, targets=None):
    """(grad (NP,), parts (3,)) float64 of 2 L_r + 4 L_bc + 2 L_ic like ``step_reference.reference_loss``, the map in
    front.  ``targets`` = (r, u_bc, u_ic) arrays: the tabulated step's loss on the same operator (c_u = 0)."""
    X_ic, X_bc, X_res = (torch.as_tensor(np.asarray(x), dtype=F64) for x in (X_ic, X_bc, X_res))
    s = FStep(flat, H, n, n_theta, theta_shape, ansatz, haar, Bf, X_ic, X_bc, X_res, drop_freq)
    if targets is None:
        X_val = {"bc": X_bc, "ic": X_ic}
        return s.weighted(s.losses(lambda u: (R.point_errors(u, X_res, S.PDE, 6) ** 2).mean(),
                                   lambda u, which: ((u - R.analytic_u(X_val[which])) ** 2).mean()))
    co = (S.PDE["c_t"], S.PDE["c_x"], S.PDE["c_y"], S.PDE["d_xx"], S.PDE["d_yy"])
    return s.weighted(s.losses(lambda u: ((R.residual(u, co) - S.as64(targets[0])) ** 2).mean(), S.mse_to(targets[1], targets[2])))


def step_inputs(H, n, n_theta, m, scale, B_res, n_ic, n_bc, salt):
    """Seeded CPU draw of one case: the frequency matrix (3, m) float32, flat float32 weights on the layout with 2m input
    columns (initialiser-like scales) and float32 IC / BC / domain points in the trainer's boxes."""
    from oracle import solver as osol
    g = torch.Generator().manual_seed(5000 * salt + 11 * n + 13 * m + B_res + 3 * n_ic + 5 * n_bc)
    Bf = (torch.randn(3, m, generator=g, dtype=torch.float64) * scale).to(torch.float32).numpy()
    lay, NP = layout(H, n, n_theta, 2 * m)
    sc = {"W1": np.sqrt(2.0 / (H + 2 * m)), "b1": 0.1, "W2": np.sqrt(2.0 / (H + n)), "b2": 0.1,
          "W3": 1.0 / np.sqrt(n), "b3": 0.3, "W4": 1.0 / np.sqrt(H), "b4": 0.1, "theta": 0.8}
    flat = np.zeros(NP, dtype=np.float32)
    for k, (o, s) in lay.items():
        cnt = int(np.prod(s))
        flat[o:o + cnt] = (torch.randn(cnt, generator=g, dtype=torch.float64) * sc[k]).numpy()
    X_ic, X_bc, X_res = [((torch.tensor(b[0]) + (torch.tensor(b[1]) - torch.tensor(b[0])) * torch.rand(k, 3, generator=g))
                          .to(torch.float32)).numpy()
                         for b, k in ((osol.BOX_IC, n_ic), (osol.BOX_BC1, n_bc), (osol.BOX_DOM, B_res))]
    return Bf, flat, X_ic, X_bc, X_res


def adam_step(prm, grad, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, m=None, v=None, step=1):
    """One float64 Adam step of the trainer (gradient clipped to ``max_norm`` first, torch's bias corrections); returns the
    new parameters and moments."""
    g = np.asarray(grad, np.float64)
    if max_norm is not None:          # torch.nn.utils.clip_grad_norm_
        g = g * min(1.0, max_norm / (float(np.sqrt((g * g).sum())) + 1e-6))
    m = (np.zeros_like(g) if m is None else m) * beta1 + (1.0 - beta1) * g
    v = (np.zeros_like(g) if v is None else v) * beta2 + (1.0 - beta2) * g * g
    step_size = lr / (1.0 - beta1 ** step)
    denom = np.sqrt(v) / math.sqrt(1.0 - beta2 ** step) + eps
    return np.asarray(prm, np.float64) - step_size * m / denom, m, v
