"""Float64 references of the coefficient step (qc_fused_pinn_coef_step, qc_post_coef, qc_sample_dataset_coef,
include/qcpinn_hip.h): the tabulated step with one operator row per residual point,

    res_p = c_u[p] u + c_3[p] u^3 + c_t[p] u_t + c_x[p] u_x + c_y[p] u_y - (d_xx[p] u_xx + d_yy[p] u_yy),

rows (c_u, c_t, c_x, c_y, d_xx, d_yy, c_3).  ``reference_loss_coef`` is tabulated_reference.reference_loss_data with
(B, 7) rows and the cubic term; the value points are those of the tabulated step.

The seeded cases are the cases of tests/tabulated_reference.py (same weights, points and targets) with the coefficient
table ``coef_star`` of their residual points: float32 roundings of smooth O(1) functions of (t, x, y), no column constant
and none at a default, c_u and c_3 of both signs, the velocity a rotation about (1/2, 1/2) that drifts in time, and every
fifth row replaced by the pure-derivative row (0, 0, 1, 0, 0, 0, 0) of a flux condition.  Negative controls: the table
rolled by one point, the c_3 column zeroed, the d_xx / d_yy columns swapped.
"""
import numpy as np
import torch

import mlp_reference as R
import tabulated_reference as T
from step_reference import Step, as64, mse_to

COLS = ("c_u", "c_t", "c_x", "c_y", "d_xx", "d_yy", "c_3")
FLUX_ROW = np.array([0, 0, 1, 0, 0, 0, 0], dtype=np.float32)       # res = u_x: a Neumann / zero-flux point
CASES, case_H, case_inputs = T.CASES, T.case_H, T.case_inputs
CONTROLS = {"reg_cascade4": ("roll", "c3zero", "swap_d"), "wave_layered7": ("roll", "c3zero", "swap_d")}
# Klein-Gordon of the reference (nn/pde.py:28-41: alpha = -1, beta = 0, gamma = 1) with (t, x) on the x / y slots:
# u_tt - u_xx + u^3 = -(d_xx u_"xx" + d_yy u_"yy") + c_3 u^3 with d_xx = -1, d_yy = 1
KLEIN_GORDON_ROW = np.array([0, 0, 0, 0, -1, 1, 1], dtype=np.float32)


def coef_star(X):
    """(B, 7) float32 coefficient rows of the points X (B, 3), formed in float64."""
    X = np.asarray(X, dtype=np.float64)
    t, x, y = X[:, 0], X[:, 1], X[:, 2]
    tab = np.stack([0.7 * np.cos(3.0 * x + t),                      # c_u: both signs
                    1.0 + 0.3 * np.sin(2.0 * y + t),                # c_t
                    -2.0 * (y - 0.5) + 0.2 * t,                     # c_x, c_y: a rotation that drifts
                    2.0 * (x - 0.5) - 0.3 * t,
                    0.3 + 0.2 * np.sin(3.0 * t + y),                # d_xx
                    0.25 + 0.15 * np.cos(2.0 * x - t),              # d_yy
                    1.2 * np.sin(2.0 * np.pi * (x - y) + 0.5)],     # c_3: both signs
                   axis=1).astype(np.float32)
    tab[4::5] = FLUX_ROW
    return tab


def uniform_table(B, coeffs, c_u, c_3=0.0):
    """The (B, 7) table of one operator for every point: what the data step applies with ``coeffs`` and ``c_u``."""
    c_t, c_x, c_y, d_xx, d_yy = coeffs
    return np.tile(np.array([c_u, c_t, c_x, c_y, d_xx, d_yy, c_3], dtype=np.float32), (B, 1))


def residual_coef(ujets, coef):
    """(6, B) u jets and (B, 7) rows -> (B,) residual."""
    c = torch.as_tensor(np.asarray(coef), dtype=R.F64)
    u = ujets[0]
    return c[:, 0] * u + c[:, 6] * u ** 3 + c[:, 1] * ujets[1] + c[:, 2] * ujets[2] + c[:, 3] * ujets[3] - \
        (c[:, 4] * ujets[4] + c[:, 5] * ujets[5])


def residual_points(flat, H, n, n_theta, theta_shape, ansatz, haar, X_res, coef, encoding="angle"):
    """(u (B,), res (B,)) float64 tensors of the residual points, and the parameter dict they hang on."""
    s = Step(flat, H, n, n_theta, theta_shape, ansatz, haar, X_res[:0], X_res[:0], X_res, encoding=encoding)
    return s.u_res[0], residual_coef(s.u_res, coef), s.P


def reference_loss_coef(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef,
                        encoding="angle"):
    """flat (NP,) weights, three (B, 3) point sets, their (B,) targets and the (B_res, 7) rows -> (grad (NP,), parts (3,))
    float64: the gradient of 2 L_r + 4 L_bc + 2 L_ic and (L_r, L_bc, L_ic)."""
    s = Step(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, encoding=encoding)
    return s.weighted(s.losses(lambda u: ((residual_coef(u, coef) - as64(r_res)) ** 2).mean(), mse_to(u_bc, u_ic)))


def variant_table(variant, coef):
    """The table a negative control's reference applies."""
    coef = np.array(coef, dtype=np.float32)
    if variant == "roll":
        coef = np.roll(coef, 1, axis=0)
    elif variant == "c3zero":
        coef[:, 6] = 0.0
    elif variant == "swap_d":
        coef[:, [4, 5]] = coef[:, [5, 4]]
    elif variant:
        raise ValueError(variant)
    return coef


def case_table(case):
    return coef_star(case_inputs(case)[3])


def case_job(case, variant="", table=None, key=None):
    """The record of reference_loss_coef on one case, under ``variant_table`` of its coef_star table or on ``table``."""
    inp = case_inputs(case)
    coef = variant_table(variant, coef_star(inp[3])) if table is None else table
    return T.case_record("coef", case, inp[4:], (coef,), lambda *a, **k: reference_loss_coef(*a, coef, **k), variant, key)


def case_reference(case, variant=""):
    """reference_loss_coef of one case through conftest.cached_oracle -> {"grad": (NP,), "parts": (3,)}."""
    return case_job(case, variant).get()


def uniform_reference(case="reg_cascade4"):
    """The case on the uniform table of tabulated_reference's operator (c_3 = 0): its reference IS the data step's
    committed record (tab_*.npz), reached through tabulated_reference.case_reference."""
    return T.case_reference(case)


def oracle_jobs():
    return T.controlled_jobs(case_job, CASES, CONTROLS)
