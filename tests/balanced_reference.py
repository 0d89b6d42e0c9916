"""Float64 references of the balanced step (qc_fused_pinn_balanced_step, qc_post_balance, qc_balance_adam_step,
include/qcpinn_hip.h): the tabulated step under learned loss weights,

    F = sum_k ( w_k e_k L_k + s_k ),   s_k = scale_k p_k,   e_k = exp(-s_k),   k = residual, BC, IC,   w = (2, 4, 2).

The network gradient of F is linear in the three per-class gradients, sum_k w_k e_k grad L_k, so ``class_reference`` caches
grad L_r, grad L_bc, grad L_ic and the three parts of every case of tests/tabulated_reference.py once (same weights,
points, targets and operator), and ``combine`` forms the gradient for any p, scale or control without a new oracle run.
Entry NP + k of the gradient is scale_k (1 - w_k e_k L_k); after a GRADS-only call the device holds 0 there (the entries
are formed in the optimiser launch), which ``combine(..., own=False)`` states.

Fixed test values: SCALE = (1.0, 2.0, 0.5), P0 = (0.3, -0.5, 0.8), so s = (0.3, -1.0, 0.4): three distinct factors on both
sides of 1.  Negative controls: "exp_plus" (e_k = exp(+s_k)), "noscale" (s_k = p_k), "swap" (the BC and IC factors
exchanged).
"""
import numpy as np
import torch

import tabulated_reference as T
from step_reference import Step, mse_to

TERMS = ("residual", "bc", "ic")
N_BAL = 3
W = (2.0, 4.0, 2.0)
SCALE = (1.0, 2.0, 0.5)
P0 = (0.3, -0.5, 0.8)
CASES, case_H, case_inputs = T.CASES, T.case_H, T.case_inputs
VARIANTS = ("exp_plus", "noscale", "swap")
CONTROLS = {"reg_cascade4": VARIANTS, "wave_layered7": VARIANTS}

_F32 = lambda a: np.asarray(a, dtype=np.float32)


def log_vars(p=P0, scale=SCALE, variant=""):
    """s_k in float64 from the float32 values the device holds."""
    s = _F32(p).astype(np.float64)
    return s if variant == "noscale" else _F32(scale).astype(np.float64) * s


def factors(p=P0, scale=SCALE, variant=""):
    """(3,) float64 e_k under a control's rule."""
    s = log_vars(p, scale, variant)
    e = np.exp(s if variant == "exp_plus" else -s)
    return e[[0, 2, 1]] if variant == "swap" else e


def weights_f32(p=P0, scale=SCALE, w=W):
    """The device's effective weights to the bit, given its expf: w_k * expf(-(scale_k * p_k)), every step in float32.
    ``expf`` here is torch's float32 exp on the CPU; the GPU tests take the device's own (``torch.exp`` on the device)."""
    s = torch.tensor(_F32(scale)) * torch.tensor(_F32(p))
    return (torch.tensor(_F32(w)) * torch.exp(-s)).numpy()


def objective(parts, p=P0, scale=SCALE, w=W):
    """F in float64 from the raw parts (L_r, L_bc, L_ic)."""
    return float(np.sum(np.asarray(w) * factors(p, scale) * np.asarray(parts, dtype=np.float64) + log_vars(p, scale)))


def own_gradient(parts, p=P0, scale=SCALE, w=W):
    """(3,) float64 d F / d p_k = scale_k (1 - w_k e_k L_k)."""
    sc = _F32(scale).astype(np.float64)
    return sc * (1.0 - np.asarray(w) * factors(p, scale) * np.asarray(parts, dtype=np.float64))


def combine(rec, p=P0, scale=SCALE, w=W, variant="", own=False):
    """(NP + 3,) float64 gradient of F from a ``class_reference`` record; the last three entries are the balancer's
    (``own``) or the zeros a GRADS-only call leaves."""
    e = factors(p, scale, variant)
    g = sum(w[k] * e[k] * rec["g_" + TERMS[k]] for k in range(N_BAL))
    tail = own_gradient(rec["parts"], p, scale, w) if own else np.zeros(N_BAL)
    return np.concatenate([g, tail])


def class_gradients(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res,
                    coeffs=T.DEFAULT_COEFFS, c_u=0.0, encoding="angle"):
    """tabulated_reference.reference_loss_data with the three losses differentiated one by one ->
    (grad L_r, grad L_bc, grad L_ic) each (NP,), parts (3,), float64."""
    s = Step(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, encoding=encoding)
    parts = s.losses(T.data_residual(r_res, coeffs, c_u), mse_to(u_bc, u_ic))
    g_r, g_b, g_i = (s.grad(l) if l.requires_grad else np.zeros(len(flat)) for l in parts)     # an empty class: zeros
    return g_r, g_b, g_i, np.array([l.item() for l in parts])


def class_job(case):
    def loss(*a, **k):
        g_r, g_b, g_i, parts = class_gradients(*a, coeffs=T.COEFFS, c_u=T.C_U, **k)
        return {"g_residual": g_r, "g_bc": g_b, "g_ic": g_i, "parts": parts}
    return T.case_record("bal", case, case_inputs(case)[4:], (T.COEFFS + (T.C_U,),), loss)


def class_reference(case):
    """class_gradients of one case through conftest.cached_oracle ->
    {"g_residual", "g_bc", "g_ic": (NP,), "parts": (3,)}."""
    return class_job(case).get()


def oracle_jobs():
    return [class_job(c) for c in CASES]


def block_error(got, ref, H, n, n_theta):
    """Largest block-relative deviation |got - ref| / max(1, max |ref block|) over the blocks of the layout (the network
    entries; the rule of the block tolerances of tests/test_gpu_tabulated.py)."""
    worst, off = 0.0, 0
    for k in (3 * H, H, n * H, n, H * n, H, H, 1, n_theta):
        a, b = np.asarray(got[off:off + k], dtype=np.float64), np.asarray(ref[off:off + k], dtype=np.float64)
        if k:
            worst = max(worst, float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max()))))
        off += k
    return worst


def adam_reference(flat, p, m, v, NP, scale=SCALE, w=W, lr=0.005, step=1, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0):
    """One float64 step of the balanced update on ``flat`` = [grad[NP + 3] | L_r, L_bc, L_ic] (the three balancer slots of
    flat are ignored), ``p`` (NP + 3,) parameters with the balancer's in the tail, moments m, v (NP + 3,).
    -> dict(grad (NP + 3,), p, m, v, F, norm, weights (3,))."""
    flat = np.asarray(flat, dtype=np.float64)
    p, m, v = (np.asarray(a, dtype=np.float64).copy() for a in (p, m, v))
    parts = flat[NP + 3:NP + 6]
    pb = p[NP:NP + 3]
    sc = _F32(scale).astype(np.float64)
    e = np.exp(-(sc * pb))
    we = np.asarray(w, dtype=np.float64) * e
    norm = float(np.sqrt(np.sum(flat[:NP] ** 2)))
    coef = min(1.0, max_norm / (norm + 1e-6))
    g = np.concatenate([flat[:NP] * coef, sc * (1.0 - we * parts)])
    F = float(np.sum(we * parts + sc * pb))
    m = m + (1.0 - betas[0]) * (g - m)
    v = betas[1] * v + (1.0 - betas[1]) * g * g
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return {"grad": g, "p": p, "m": m, "v": v, "F": F, "norm": norm, "weights": we}
