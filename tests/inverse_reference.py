"""Float64 references of the inverse step (qc_fused_pinn_inverse_step, qc_post_learn, include/qcpinn_hip.h): the tabulated
step with a trainable global operator,

    res_p = c_u u + c_3 u^3 + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy),   c_k = scale_k p_k + base_k,

k in the column order (c_u, c_t, c_x, c_y, d_xx, d_yy, c_3).  ``reference_loss_inverse`` is
coef_reference.reference_loss_coef with that one operator for every residual point and ``p`` as a leaf of the graph: its
gradient has NP + 7 entries, the operator block last.  The value points are those of the tabulated step.

The seeded cases are the cases of tests/tabulated_reference.py (same weights, points and targets) under BASE, SCALE and
P0 below: no coefficient at a default, c_u and c_3 non-zero, scales on both sides of 1, and a frozen c_y (scale 0) that
carries a non-zero p on purpose.  Negative controls: +d_xx u_xx in place of -, scale ignored (c = p + base and no factor
on the gradient), base ignored (c = scale p).
"""
import numpy as np
import torch

import tabulated_reference as T
from step_reference import Step, as64, mse_to

COLS = ("c_u", "c_t", "c_x", "c_y", "d_xx", "d_yy", "c_3")
N_OP = len(COLS)
BASE = (0.7, 0.9, 1.3, -0.6, 0.02, 0.015, 0.4)
SCALE = (1.0, 0.5, 2.0, 0.0, 0.25, 4.0, 1.5)
P0 = (0.3, -0.4, 0.2, 0.9, 0.8, -0.05, 0.6)
CASES, case_H, case_inputs = T.CASES, T.case_H, T.case_inputs
CONTROLS = {"reg_cascade4": ("sign_dxx", "noscale", "nobase"), "wave_layered7": ("sign_dxx", "noscale", "nobase")}

_F32 = lambda a: np.asarray(a, dtype=np.float32)


def coefficients(p=P0, base=BASE, scale=SCALE):
    """The seven effective coefficients in float64 from the float32 values the device holds."""
    return _F32(scale).astype(np.float64) * _F32(p).astype(np.float64) + _F32(base).astype(np.float64)


def coefficients_f32(p=P0, base=BASE, scale=SCALE):
    """fmaf(scale, p, base) in float32: one rounding of the exact float64 sum (products of two float32 are exact there)."""
    return coefficients(p, base, scale).astype(np.float32)


def operator(p, base=BASE, scale=SCALE, variant=""):
    """(7,) float64 tensor c of the leaf ``p`` under a control's rule."""
    b, s = (torch.as_tensor(_F32(a).astype(np.float64)) for a in (base, scale))
    if variant == "noscale":
        s = torch.ones_like(s)
    elif variant == "nobase":
        b = torch.zeros_like(b)
    return s * p + b


def residual_op(ujets, c, variant=""):
    """(6, B) u jets and the (7,) operator -> (B,) residual."""
    u = ujets[0]
    sx = 1.0 if variant == "sign_dxx" else -1.0
    return c[0] * u + c[6] * u ** 3 + c[1] * ujets[1] + c[2] * ujets[2] + c[3] * ujets[3] + sx * c[4] * ujets[4] - c[5] * ujets[5]


def reference_loss_inverse(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, p=P0,
                           base=BASE, scale=SCALE, encoding="angle", variant=""):
    """flat (NP,) weights, three (B, 3) point sets, their (B,) targets and the operator -> (grad (NP + 7,), parts (3,))
    float64: the gradient of 2 L_r + 4 L_bc + 2 L_ic with respect to (weights, p) and (L_r, L_bc, L_ic)."""
    pt = torch.tensor(_F32(p).astype(np.float64), requires_grad=True)
    s = Step(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, encoding=encoding, extra=[pt])

    def l_r(u):
        res = residual_op(u, operator(pt, base, scale, variant), variant)
        return ((res - as64(r_res)) ** 2).mean()
    return s.weighted(s.losses(l_r, mse_to(u_bc, u_ic)))


def case_job(case, variant=""):
    return T.case_record("inv", case, case_inputs(case)[4:], (BASE, SCALE, P0),
                         lambda *a, **k: reference_loss_inverse(*a, variant=variant, **k), variant)


def case_reference(case, variant=""):
    """reference_loss_inverse of one case through conftest.cached_oracle -> {"grad": (NP + 7,), "parts": (3,)}."""
    return case_job(case, variant).get()


UNIFORM_C3 = 0.4        # the cubic coefficient of the agreement test with the coefficient step


def uniform_c3_job(case="reg_cascade4"):
    import coef_reference as CR
    table = CR.uniform_table(CASES[case][4], T.COEFFS, T.C_U, UNIFORM_C3)
    return CR.case_job(case, table=table, key=f"inv_uniform_c3_{case}")


def uniform_c3_reference(case="reg_cascade4"):
    """The coefficient step's own float64 reference (coef_reference.reference_loss_coef) on the uniform table of
    tabulated_reference's operator with c_3 = UNIFORM_C3, through conftest.cached_oracle."""
    return uniform_c3_job(case).get()


def oracle_jobs():
    return T.controlled_jobs(case_job, CASES, CONTROLS) + [uniform_c3_job()]
