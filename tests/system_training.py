"""Float64 replay of a training run of trainer.system_train.SystemTrainer with the device gather: the seeded dataset of a
three-output model (tests/system_reference.py's scaled Navier-Stokes, its weights and targets), the minibatches the
gather picks (tabulated_reference.dataset_indices) and the loss history of a float64 copy of oracle.solver.OracleSolver
([3, 50, 3]) trained on them: the term list evaluated on autograd derivatives, loss = 2 L_r + 4 L_bc + 2 L_ic,
clip_grad_norm_(1), Adam, ReduceLROnPlateau, as in tests/coef_training.py.
"""
import torch

import system_reference as S
import tabulated_reference as T
import tabulated_training as TT
from step_reference import as64, batch_inputs, flat_of, record

DS_SIZES, BATCH, STEPS, N_IC, N_BC = TT.DS_SIZES, TT.BATCH, TT.STEPS, TT.N_IC, TT.N_BC
K, N_EQ = 3, 3
ANSATZ, N_QUBITS = "cascade", 4


def base_args():
    return dict(TT.base_args(ANSATZ, N_QUBITS), classic_network=[3, 50, K])


def dataset_arrays():
    """(X_res, R (N, 3), X_ic, U_ic (N, 3), X_bc, U_bc (N, 3)): tabulated_training's points with the system's targets."""
    Xr, _, Xi, _, Xb, _ = TT.dataset_arrays()
    return Xr, S.residual_targets(Xr, N_EQ), Xi, S.value_targets(Xi, K), Xb, S.value_targets(Xb, K)


def expected_batches(seed=None):
    """Per step (1-based counter): (X_ic, X_bc, X_res, U_ic, U_bc, R_res)."""
    seed = TT.trainer_seed() if seed is None else seed
    Xr, Rr, Xi, Ui, Xb, Ub = dataset_arrays()
    out = []
    for step in range(1, STEPS + 1):
        kr = T.dataset_indices(0, 0, BATCH, DS_SIZES[0], seed, step)
        ki = T.dataset_indices(1, 0, N_IC, DS_SIZES[1], seed, step)
        kb = T.dataset_indices(2, 0, N_BC, DS_SIZES[2], seed, step)
        out.append((Xi[ki], Xb[kb], Xr[kr], Ui[ki], Ub[kb], Rr[kr]))
    return out


def initial_model():
    """The float32 OracleSolver a DVPDESolver built after torch.manual_seed(1) starts equal to (same RNG consumption)."""
    from oracle import solver as osol
    torch.manual_seed(1)
    return osol.OracleSolver(base_args(), device=torch.device("cpu"))


def system_run(model, batches):
    """Loss history of the float64 copy of ``model`` trained on ``batches``: tabulated_training.replay with the term list
    as the residual and the parts weighted per equation and per output."""
    terms, w_eq, w_out = S.system_of(K)
    we, wo = as64(w_eq), as64(w_out)

    def residual(b, jets):
        res = S.eval_terms(torch.stack([torch.stack(j)[:, :, 0] for j in jets]), terms, N_EQ) - as64(b[5]).T
        return (we * (res ** 2).mean(1)).sum()
    return TT.replay(model, batches, residual, value=lambda net, X, U: (wo * ((net(as64(X)) - as64(U)) ** 2).mean(0)).sum())


def training_job(batches=None):
    batches = expected_batches() if batches is None else batches
    model = initial_model()
    return record(f"systrain_{ANSATZ}{N_QUBITS}_K{K}", [flat_of(model)] + batch_inputs(*batches),
                  lambda: {"loss": system_run(model, batches)})


def training_reference(batches=None):
    """{"loss": (STEPS,)} through conftest.cached_oracle, keyed on the initial weights and the batches."""
    return training_job(batches).get()


def oracle_jobs():
    return [training_job()]
