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

import mlp_reference as R
import tabulated_reference as T
from conftest import cached_oracle, pkg
from step_reference import haar_for

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
    from oracle import jets as oj
    from oracle import statevector as sv
    P = R.unpack(flat, H, n, n_theta)
    theta = P["theta"].reshape(theta_shape)
    pt = torch.tensor(_F32(p).astype(np.float64), requires_grad=True)
    zero = torch.zeros((), dtype=R.F64)
    as64 = lambda a: torch.as_tensor(np.asarray(a), dtype=R.F64)
    l_r = zero
    if len(X_res):
        a = R.pre_jets(P, X_res, 6)
        q = oj.qjets_from_ajets(a, theta, ansatz, n, haar, encoding)
        res = residual_op(R.post_jets(P, q), operator(pt, base, scale, variant), variant)
        l_r = ((res - as64(r_res)) ** 2).mean()
    out = []
    for Xv, tv in ((X_bc, u_bc), (X_ic, u_ic)):
        if not len(Xv):
            out.append(zero)
            continue
        av = R.pre_jets(P, Xv, 1)
        qv = sv.circuit_expvals(av[0].T, theta, ansatz, n, haar, encoding)[None]
        uv = R.post_jets(P, qv)
        out.append(((uv[0] - as64(tv)) ** 2).mean())
    l_bc, l_ic = out
    loss = 2.0 * l_r + 4.0 * l_bc + 2.0 * l_ic
    grads = torch.autograd.grad(loss, [P[k] for k in R.NAMES] + [pt], allow_unused=True)
    gp = np.zeros(N_OP) if grads[-1] is None else grads[-1].numpy()
    g = np.concatenate([R.flatten(dict(zip(R.NAMES, grads[:-1])), H, n, n_theta), gp])
    return g, np.array([l_r.item(), l_bc.item(), l_ic.item()])


def case_reference(case, variant=""):
    """reference_loss_inverse of one case through conftest.cached_oracle -> {"grad": (NP + 7,), "parts": (3,)}."""
    ans, n, L, enc, B_res, n_ic, n_bc = CASES[case]
    P = int(pkg("circuits").params_per_layer(ans, n))
    flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res = case_inputs(case)

    def compute():
        g, parts = reference_loss_inverse(flat, case_H(case), n, L * P, (L, P), ans, haar_for(n, 1),
                                          *(torch.as_tensor(x).double() for x in (X_ic, X_bc, X_res)), u_ic, u_bc, r_res,
                                          encoding=enc, variant=variant)
        return {"grad": g, "parts": parts}
    inputs = (np.asarray(flat, dtype=np.float32),) + tuple(np.asarray(x, dtype=np.float32) for x in (X_ic, X_bc, X_res)) + \
        (u_ic, u_bc, r_res, _F32(BASE), _F32(SCALE), _F32(P0))
    key = f"inv_{ans}_n{n}_L{L}_{enc}_r{B_res}_i{n_ic}_b{n_bc}" + (f"_H{case_H(case)}" if case in T.CASE_H else "") + \
        (f"_{variant}" if variant else "")
    return cached_oracle(key, inputs, compute)


UNIFORM_C3 = 0.4        # the cubic coefficient of the agreement test with the coefficient step


def uniform_c3_reference(case="reg_cascade4"):
    """The coefficient step's own float64 reference (coef_reference.reference_loss_coef) on the uniform table of
    tabulated_reference's operator with c_3 = UNIFORM_C3, through conftest.cached_oracle."""
    import coef_reference as CR
    ans, n, L, enc, B_res, n_ic, n_bc = CASES[case]
    P = int(pkg("circuits").params_per_layer(ans, n))
    flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res = case_inputs(case)
    table = CR.uniform_table(B_res, T.COEFFS, T.C_U, UNIFORM_C3)

    def compute():
        g, parts = CR.reference_loss_coef(flat, case_H(case), n, L * P, (L, P), ans, haar_for(n, 1),
                                          *(torch.as_tensor(x).double() for x in (X_ic, X_bc, X_res)), u_ic, u_bc, r_res,
                                          table, encoding=enc)
        return {"grad": g, "parts": parts}
    inputs = (np.asarray(flat, dtype=np.float32),) + tuple(np.asarray(x, dtype=np.float32) for x in (X_ic, X_bc, X_res)) + \
        (u_ic, u_bc, r_res, table)
    return cached_oracle(f"inv_uniform_c3_{case}", inputs, compute)


def oracle_jobs():
    """(case, variant) of every committed record (tests/golden/make_inverse_oracle_cache.py)."""
    return [(c, "") for c in CASES] + [(c, v) for c, vs in CONTROLS.items() for v in vs]
