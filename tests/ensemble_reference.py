"""Cases and committed float64 records of the ensemble step (qc_fused_pinn_ensemble_step, QC_PHASE_GRADS): member m of a
case takes ``step_inputs(..., salt=1 + m)``, so weights and points differ per member, and its record is the single-model
reference ``step_reference.reference_loss`` on those inputs, keyed by case and member
(tests/golden/make_ensemble_oracle.py writes the records)."""
import numpy as np
import torch

from conftest import pkg
from step_reference import haar_for, record, reference_loss, step_inputs, step_key

SEED = 1       # args["seed"]: the fixed two-wire unitaries of n >= 4

# id -> (ansatz, n, L, H, M, B_res, n_ic, n_bc)
CASES = {
    "cascade4": ("cascade", 4, 1, 50, 3, 70, 30, 20),       # static program, ragged tiles, IC and BC in one value tile
    "alternate5": ("alternate", 5, 1, 50, 2, 40, 25, 10),   # static, n = 5
    "cascade3_L2": ("cascade", 3, 2, 33, 3, 65, 1, 40),     # interpreter, odd H, two residual tiles
    "farhi2": ("farhi", 2, 1, 50, 2, 10, 5, 6),             # smallest n
}


def n_theta_of(case):
    ans, n, L = CASES[case][:3]
    return L * int(pkg("circuits").params_per_layer(ans, n))


def member_inputs(case, m):
    """(flat, X_ic, X_bc, X_res) of member ``m``."""
    ans, n, L, H, M, B_res, n_ic, n_bc = CASES[case]
    return step_inputs(H, n, n_theta_of(case), B_res, n_ic, n_bc, salt=1 + m)


def member_job(case, m):
    ans, n, L, H, M, B_res, n_ic, n_bc = CASES[case]
    flat, X_ic, X_bc, X_res = member_inputs(case, m)
    n_theta = n_theta_of(case)

    def compute():
        g, parts = reference_loss(flat, H, n, n_theta, (L, n_theta // L), ans, haar_for(n, SEED),
                                  *(torch.as_tensor(x).double() for x in (X_ic, X_bc, X_res)))
        return {"grad": g, "parts": parts}
    # (the prefix keeps these records apart from the single-model step's, which tests/test_oracle_records_cpu.py counts)
    return record("ens" + step_key(ans, n, L, SEED, "angle", B_res, n_ic, n_bc), (np.asarray(flat, dtype=np.float32), X_ic, X_bc, X_res),
                  compute, H=H, variant=f"m{m}", case=case)


def oracle_jobs():
    return [member_job(c, m) for c in CASES for m in range(CASES[c][4])]


def member_reference(case, m):
    return member_job(case, m).get()
