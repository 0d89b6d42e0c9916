"""Float64 replay of a training run on a coefficient dataset (FusedTrainer(..., dataset=) with ``coef_res``): the
dataset, sizes, seed and batches of tests/tabulated_training.py with the coefficient table coef_reference.coef_star of
its residual rows, gathered by the same indices, and the loss history of the float64 OracleSolver copy trained on them
with the per-point residual c_u u + c_3 u^3 + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy).
"""
import torch

import coef_reference as CR
import tabulated_reference as T
import tabulated_training as TT
from step_reference import as64, batch_inputs, flat_of, record

TRAIN_CASES, BATCH, STEPS, N_IC, N_BC = TT.TRAIN_CASES, TT.BATCH, TT.STEPS, TT.N_IC, TT.N_BC


def dataset_arrays():
    """(X_res, r, X_ic, u_ic, X_bc, u_bc, coef_res): tabulated_training's dataset and the table of its residual rows."""
    arr = TT.dataset_arrays()
    return arr + (CR.coef_star(arr[0]),)


def expected_batches(seed=None):
    """Per step: (X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef_res (BATCH, 7))."""
    seed = TT.trainer_seed() if seed is None else seed
    coef = dataset_arrays()[6]
    out = []
    for step, b in enumerate(TT.expected_batches(seed), start=1):
        kr = T.dataset_indices(0, 0, BATCH, TT.DS_SIZES[0], seed, step)
        out.append(b + (coef[kr],))
    return out


def row_residual(b, jets):
    """The ``residual`` of tabulated_training.replay on per-point rows: batch entry 6 holds the (B, 7) table."""
    rows = (as64(b[6])[:, k:k + 1] for k in range(7))
    return torch.nn.functional.mse_loss(TT.operator_residual(jets[0], *rows), as64(b[5])[:, None])


def training_job(case, batches=None):
    batches = expected_batches() if batches is None else batches
    model = TT.initial_model(case)
    return record(f"coeftrain_{case}", [flat_of(model)] + batch_inputs(*batches),
                  lambda: {"loss": TT.replay(model, batches, row_residual)})


def training_reference(case, batches=None):
    """{"loss": (STEPS,)} of one case through conftest.cached_oracle, keyed on the initial weights and the batches."""
    return training_job(case, batches).get()


def oracle_jobs():
    return [training_job(c) for c in TRAIN_CASES]
