"""Float64 reference of qc_dataset_scores (include/qcpinn_hip.h): the six channels of u on the residual rows of a seeded
dataset, from tests/mlp_reference.py and the circuit oracle like tests/tabulated_reference.py, cached through
conftest.cached_oracle (arrays only; tests/golden/make_oracle_cache.py writes the records).  Every residual
the tests compare against is formed from those channels in float64:

  data step        C_U u + residual(u, COEFFS)                 (tests/tabulated_reference.py)
  coefficient step residual_coef(u, coef_star(X))              (tests/coef_reference.py, c_3 != 0)
  qc_post mode 0   residual(u, COEFFS)                         (the parent's residual: the yardstick of the tolerance)

and the score is |res - r_star(X)|.  One dataset of N_MAX = 2 B_RES + 3 rows per case; the smaller datasets are its
leading rows, so one oracle run serves every size."""
import numpy as np
import torch

import coef_reference as CR
import mlp_reference as R
import tabulated_reference as T
from conftest import pkg
from step_reference import Step, haar_for, record, step_inputs

B_RES = 64
N_MAX = 2 * B_RES + 3
SIZES = (1, 65, B_RES + 1, 2 * B_RES + 3)
# id -> (ansatz, n, L, encoding): merged ends, the coefficient case, lanes, HBM and amplitude encoding
CASES = {"reg_cascade2": ("cascade", 2, 1, "angle"), "reg_cascade4": ("cascade", 4, 1, "angle"),
         "wave_layered7": ("layered", 7, 1, "angle"), "hbm_cascade9": ("cascade", 9, 1, "angle"),
         "amp_cascade4": ("cascade", 4, 1, "amplitude")}


def case_inputs(case):
    """(flat (NP,) float32, X (N_MAX, 3) float32 numpy, r (N_MAX,) float32, coef (N_MAX, 7) float32)."""
    ans, n, L, enc = CASES[case]
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    flat, _, _, X = step_inputs(T.H, n, n_theta, N_MAX, 0, 0, salt=5)
    X = X.numpy()
    return flat, X, T.r_star(X), CR.coef_star(X)


def ujets_job(case):
    ans, n, L, enc = CASES[case]
    P = int(pkg("circuits").params_per_layer(ans, n))
    flat, X, _, _ = case_inputs(case)

    def compute():
        Xr = torch.as_tensor(X).double()
        return {"ujets": Step(flat, T.H, n, L * P, (L, P), ans, haar_for(n, 1), Xr[:0], Xr[:0], Xr, encoding=enc).u_res.detach().numpy()}
    return record(f"adapt_ujets_{ans}_n{n}_L{L}_{enc}_N{N_MAX}", (flat, X), compute)


def case_ujets(case):
    """(6, N_MAX) float64 channels of u on the case's rows."""
    return ujets_job(case).get()["ujets"]


def oracle_jobs():
    return [ujets_job(c) for c in CASES]


def residuals(case):
    """{"mode0", "data", "coef"} -> (N_MAX,) float64 residuals of the case's rows."""
    _, X, _, coef = case_inputs(case)
    u = torch.as_tensor(case_ujets(case))
    lin = R.residual(u, T.COEFFS)
    return {"mode0": lin.numpy(), "data": (T.C_U * u[0] + lin).numpy(), "coef": CR.residual_coef(u, coef).numpy()}
