"""Float64 replays of balanced training runs (BalancedTrainer with the device gather): the dataset, sizes, seed, batches
and six steps of tests/tabulated_training.py, the balancer of tests/balanced_reference.py (SCALE, p starting at P0), and
the histories of F and of the effective weights of the float64 OracleSolver copy trained on them with the three p_k as
one more Adam param group (same lr), the gradient clip over the model's parameters ONLY, and ReduceLROnPlateau stepping
on F.  ``hold=True``: the same replay with the balancer frozen at its start, the negative control of the weight check.
"""
import numpy as np
import torch

import balanced_reference as BR
import tabulated_reference as T
import tabulated_training as TT
from step_reference import batch_inputs, flat_of, record

TRAIN_CASES, BATCH, STEPS, N_IC, N_BC = TT.TRAIN_CASES, TT.BATCH, TT.STEPS, TT.N_IC, TT.N_BC
dataset_arrays, expected_batches = TT.dataset_arrays, TT.expected_batches


def balanced_run(model, batches, p0=BR.P0, scale=BR.SCALE, w=BR.W, hold=False, coeffs=T.COEFFS, c_u=T.C_U):
    """(history of F (steps,), effective weights w_k e_k USED in each step (steps, 3)) of the float64 copy of ``model``
    and the balancer trained on ``batches``: tabulated_training.replay with the objective F and ``p`` as a param group of
    its own, outside the clip."""
    p = torch.tensor(np.asarray(p0, dtype=np.float32).astype(np.float64), requires_grad=not hold)
    sc = torch.tensor(np.asarray(scale, dtype=np.float32).astype(np.float64))
    wt = torch.tensor(np.asarray(w, dtype=np.float64))
    whist = []

    def objective(*parts):
        s = sc * p
        we = wt * torch.exp(-s)
        whist.append(we.detach().numpy().copy())
        return (we * torch.stack(parts) + s).sum()
    hist = TT.replay(model, batches, TT.data_residual(coeffs, c_u), objective, extra=[] if hold else [p], extra_group=True)
    return hist, np.array(whist)


def training_job(case, batches=None, hold=False):
    batches = expected_batches() if batches is None else batches
    model = TT.initial_model(case)

    def compute():
        loss, weights = balanced_run(model, batches, hold=hold)
        return {"loss": loss, "weights": weights}
    return record(f"baltrain_{case}", [flat_of(model), T.COEFFS + (T.C_U,), BR.SCALE, BR.P0, BR.W] + batch_inputs(*batches),
                  compute, variant="hold" if hold else "")


def training_reference(case, batches=None, hold=False):
    """{"loss": (STEPS,), "weights": (STEPS, 3)} of one case through conftest.cached_oracle, keyed on the initial weights,
    the balancer and the batches."""
    return training_job(case, batches, hold).get()


def oracle_jobs():
    return [training_job(c, hold=h) for c in TRAIN_CASES for h in (False, True)]
