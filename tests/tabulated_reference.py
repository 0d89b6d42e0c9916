"""Float64 references of the tabulated step (qc_fused_pinn_data_step, qc_sample_dataset, include/qcpinn_hip.h).

``dataset_indices``: the rows the device gather picks, restated on tests/philox_reference.philox4x32_10.  Global point
``g`` of segment ``seg`` (0 residual, 1 IC, 2 BC) draws the block of the coordinate draw, counter
(g lo, g hi, step lo, step hi ^ seg << 30) and key = seed, and takes row ``(word 0 * N) >> 32`` of a segment of N rows.

``reference_loss_data``: tests/step_reference.reference_loss with the targets taken from arrays and the residual
c_u u + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy); composed from tests/mlp_reference.py and the circuit
oracles in the same way, differentiated by torch.autograd.

The seeded cases of the GPU tests (tests/test_gpu_tabulated.py) live here too, so that the CPU tests and
tests/golden/make_oracle_cache.py see the same inputs: weights and points from step_reference.step_inputs,
targets the float32 roundings of two smooth functions that are no solution of the operator.
"""
import numpy as np
import torch

import mlp_reference as R
import philox_reference as PR
from conftest import pkg
from step_reference import Step, as64, case_key, haar_for, mse_to, record, step_inputs

H = 50
# c_t, c_x, c_y, d_xx, d_yy and the zeroth-order coefficient: none at its default
COEFFS = (0.9, 1.3, -0.6, 0.02, 0.015)
C_U = 0.7
DEFAULT_COEFFS = (1.0, 1.0, 1.0, 0.01, 0.01)

# id -> (ansatz, n, L, encoding, B_res, n_ic, n_bc); the comment names the form the case reaches
CASES = {
    "reg_cascade4": ("cascade", 4, 1, "angle", 70, 30, 20),          # merged; one value tile holds IC and BC
    "reg_sim_circ_15_5": ("sim_circ_15", 5, 1, "angle", 20, 0, 0),   # two-stream form, B_val = 0
    "reg_cascade3_L2": ("cascade", 3, 2, "angle", 0, 70, 75),        # two-stream form, B_res = 0, three value tiles
    "wave_layered7": ("layered", 7, 1, "angle", 65, 1, 40),          # lanes family
    "hbm_cascade9": ("cascade", 9, 1, "angle", 65, 3, 2),            # HBM family
    "amp_cascade4": ("cascade", 4, 1, "amplitude", 40, 10, 10),      # amplitude encoding
    "reg_cascade4_H129": ("cascade", 4, 1, "angle", 70, 30, 20),     # merged, H > 128: point + weight-gradient kernel pair
    # the ends of the merged form's range of wire counts.  Two tiles in both pipelines, the second holding one point; the
    # first value tile mixes IC and BC: the smallest merged shape with every tail
    "reg_cascade2": ("cascade", 2, 1, "angle", 65, 1, 64),
    "reg_cascade5": ("cascade", 5, 1, "angle", 65, 1, 64),
}
CASE_H = {"reg_cascade4_H129": 129}     # hidden width of a case (default H)


def case_H(case):
    return CASE_H.get(case, H)


# negative controls: residual targets rolled by one point, value targets rolled by one, c_u = 0 in place of C_U
CONTROLS = {"reg_cascade4": ("roll_res", "roll_val", "cu0"), "wave_layered7": ("roll_res", "roll_val", "cu0")}


def dataset_indices(seg, offset, count, N, seed, step):
    """(count,) int64 rows of global points offset .. offset + count - 1 of segment ``seg`` in a dataset of N rows."""
    assert 1 <= N < 2 ** 31
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    g = np.uint64(offset) + np.arange(count, dtype=np.uint64)
    ctr = (g & PR.MASK, g >> PR.S32, step & 0xFFFFFFFF, (step >> 32) ^ ((seg << 30) & 0xFFFFFFFF))
    w0 = PR.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[0]
    return ((w0 * np.uint64(N)) >> PR.S32).astype(np.int64)        # word < 2^32, N < 2^31: no overflow in uint64


def u_star(X):
    """sin(2 pi x) cos(pi y) exp(-t / 2) + 0.3 in float64, rounded to float32."""
    X = np.asarray(X, dtype=np.float64)
    t, x, y = X[:, 0], X[:, 1], X[:, 2]
    return (np.sin(2 * np.pi * x) * np.cos(np.pi * y) * np.exp(-0.5 * t) + 0.3).astype(np.float32)


def r_star(X):
    """1.5 cos(3 t + x - 2 y) in float64, rounded to float32."""
    X = np.asarray(X, dtype=np.float64)
    return (1.5 * np.cos(3.0 * X[:, 0] + X[:, 1] - 2.0 * X[:, 2])).astype(np.float32)


def data_residual(r_res, coeffs=DEFAULT_COEFFS, c_u=0.0):
    """The residual loss of the data step for Step.losses: mean (c_u u + c_t u_t + ... - r)^2 of the u jets."""
    def l_r(u):
        res = c_u * u[0] + R.residual(u, coeffs)
        return ((res - as64(r_res)) ** 2).mean()
    return l_r


def reference_loss_data(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res,
                        coeffs=DEFAULT_COEFFS, c_u=0.0, encoding="angle"):
    """flat (NP,) weights, three (B, 3) point sets and their (B,) targets -> (grad (NP,), parts (3,)) float64: the
    gradient of 2 L_r + 4 L_bc + 2 L_ic and (L_r, L_bc, L_ic), L_r on c_u u + c_t u_t + ... - r."""
    s = Step(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, encoding=encoding)
    return s.weighted(s.losses(data_residual(r_res, coeffs, c_u), mse_to(u_bc, u_ic)))


def case_inputs(case):
    """(flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res) of one seeded case: float32 numpy targets, torch points."""
    ans, n, L, enc, B_res, n_ic, n_bc = CASES[case]
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    flat, X_ic, X_bc, X_res = step_inputs(case_H(case), n, n_theta, B_res, n_ic, n_bc, salt=3)
    return flat, X_ic, X_bc, X_res, u_star(X_ic), u_star(X_bc), r_star(X_res)


def variant_targets(variant, u_ic, u_bc, r_res, c_u=C_U):
    """Targets and c_u of a negative control.  "roll_val" rolls the value targets in the step's order, IC then BC."""
    if variant == "roll_res":
        r_res = np.roll(r_res, 1)
    elif variant == "roll_val":
        uv = np.roll(np.concatenate([u_ic, u_bc]), 1)
        u_ic, u_bc = uv[:len(u_ic)], uv[len(u_ic):]
    elif variant == "cu0":
        c_u = 0.0
    elif variant:
        raise ValueError(variant)
    return u_ic, u_bc, r_res, c_u


def case_record(prefix, case, targets, tail, loss, variant="", key=None):
    """The record ``<prefix>_<case>[_H<H>][_<variant>]`` of one reference of this family of cases (data, coefficient,
    inverse, balanced step).  Its inputs: the case's weights and points, ``targets`` = (u_ic, u_bc, r_res) and ``tail``.
    ``loss(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, *targets, encoding=)`` gives (grad, parts)
    or the record's dict."""
    ans, n, L, enc, *_ = CASES[case]
    P = int(pkg("circuits").params_per_layer(ans, n))
    flat, X_ic, X_bc, X_res = case_inputs(case)[:4]

    def compute():
        out = loss(flat, case_H(case), n, L * P, (L, P), ans, haar_for(n, 1),
                   *(torch.as_tensor(x).double() for x in (X_ic, X_bc, X_res)), *targets, encoding=enc)
        return out if isinstance(out, dict) else {"grad": out[0], "parts": out[1]}
    return record(key or case_key(prefix, CASES[case]), (flat, X_ic, X_bc, X_res) + tuple(targets) + tuple(tail), compute,
                  H=CASE_H.get(case), variant=variant, case=case)


def case_job(case, variant=""):
    ui, ub, rr, c_u = variant_targets(variant, *case_inputs(case)[4:])
    return case_record("tab", case, (ui, ub, rr), (COEFFS + (c_u,),),
                       lambda *a, **k: reference_loss_data(*a, coeffs=COEFFS, c_u=c_u, **k), variant)


def case_reference(case, variant=""):
    """reference_loss_data of one case through conftest.cached_oracle -> {"grad": (NP,), "parts": (3,)}."""
    return case_job(case, variant).get()


def controlled_jobs(job, cases, controls):
    """``job(case)`` of every case and ``job(case, variant)`` of every negative control: a module's committed records."""
    return [job(c) for c in cases] + [job(c, v) for c, vs in controls.items() for v in vs]


def oracle_jobs():
    return controlled_jobs(case_job, CASES, CONTROLS)
