"""Float64 replay of a training run of trainer.system_train.SystemTrainer with the device gather: the seeded dataset of a
three-output model (tests/system_reference.py's scaled Navier-Stokes, its weights and targets), the minibatches the
gather picks (tabulated_reference.dataset_indices) and the loss history of a float64 copy of oracle.solver.OracleSolver
([3, 50, 3]) trained on them: the term list evaluated on autograd derivatives, loss = 2 L_r + 4 L_bc + 2 L_ic,
clip_grad_norm_(1), Adam, ReduceLROnPlateau, as in tests/coef_training.py.
"""
import numpy as np
import torch

import system_reference as S
import tabulated_reference as T
import tabulated_training as TT
from conftest import cached_oracle

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


def replay(model, batches):
    """Loss history of the float64 copy of ``model`` trained on ``batches``."""
    from oracle import statevector as sv
    model = model.double()
    ql = model.quantum_layer
    terms, w_eq, w_out = S.system_of(K)

    def net(x):
        q = sv.circuit_expvals(model.preprocessor(x), ql.params, ql.q_ansatz, ql.num_qubits, ql._haar, "angle")
        return model.postprocessor(q.T.reshape(-1, ql.num_qubits))

    opt = torch.optim.Adam(model.parameters(), lr=model.args["lr"])
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=1000)
    g = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    as64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    we, wo = as64(w_eq), as64(w_out)
    hist = []
    for X_ic, X_bc, X_res, U_ic, U_bc, R_res in batches:
        opt.zero_grad()
        t, x, y = [as64(X_res)[:, k:k + 1].requires_grad_(True) for k in range(3)]
        f = net(torch.cat((t, x, y), 1))
        jets = []
        for k in range(K):
            u = f[:, k:k + 1]
            u_x, u_y = g(u, x), g(u, y)
            jets.append(torch.stack([u, g(u, t), u_x, u_y, g(u_x, x), g(u_y, y)])[:, :, 0])
        res = S.eval_terms(torch.stack(jets), terms, N_EQ) - as64(R_res).T
        l_r = (we * (res ** 2).mean(1)).sum()
        l_bc = (wo * ((net(as64(X_bc)) - as64(U_bc)) ** 2).mean(0)).sum()
        l_ic = (wo * ((net(as64(X_ic)) - as64(U_ic)) ** 2).mean(0)).sum()
        loss = 2.0 * l_r + 4.0 * l_bc + 2.0 * l_ic
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1)
        opt.step()
        sch.step(loss)
        hist.append(loss.item())
    return np.array(hist)


def training_reference(batches=None):
    """{"loss": (STEPS,)} through conftest.cached_oracle, keyed on the initial weights and the batches."""
    batches = expected_batches() if batches is None else batches
    model = initial_model()
    flat0 = np.concatenate([p.detach().numpy().reshape(-1) for p in model.parameters()]).astype(np.float32)
    inputs = [flat0]
    for b in batches:
        inputs += [np.asarray(a, dtype=np.float32) for a in b]
    return cached_oracle(f"systrain_{ANSATZ}{N_QUBITS}_K{K}", inputs, lambda: {"loss": replay(model, batches)})
