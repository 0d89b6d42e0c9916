"""Float64 replay of a training run on a coefficient dataset (FusedTrainer(..., dataset=) with ``coef_res``): the
dataset, sizes, seed and batches of tests/tabulated_training.py with the coefficient table coef_reference.coef_star of
its residual rows, gathered by the same indices, and the loss history of the float64 OracleSolver copy trained on them
with the per-point residual c_u u + c_3 u^3 + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy).
"""
import numpy as np
import torch

import coef_reference as CR
import tabulated_reference as T
import tabulated_training as TT
from conftest import cached_oracle

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


def replay(model, batches):
    """Loss history of the float64 copy of ``model`` trained on ``batches`` (tabulated_training.replay, per-point rows)."""
    from oracle import statevector as sv
    model = model.double()
    ql = model.quantum_layer

    def net(x):
        q = sv.circuit_expvals(model.preprocessor(x), ql.params, ql.q_ansatz, ql.num_qubits, ql._haar, "angle")
        return model.postprocessor(q.T.reshape(-1, ql.num_qubits))

    opt = torch.optim.Adam(model.parameters(), lr=model.args["lr"])
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=1000)
    g = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    mse = torch.nn.MSELoss()
    hist = []
    for X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef in batches:
        as64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
        c_u, c_t, c_x, c_y, d_xx, d_yy, c_3 = (as64(coef)[:, k:k + 1] for k in range(7))
        opt.zero_grad()
        t, x, y = [as64(X_res)[:, k:k + 1].requires_grad_(True) for k in range(3)]
        u = net(torch.cat((t, x, y), 1))
        u_x, u_y = g(u, x), g(u, y)
        res = c_u * u + c_3 * u ** 3 + c_t * g(u, t) + c_x * u_x + c_y * u_y - (d_xx * g(u_x, x) + d_yy * g(u_y, y))
        loss = 2.0 * mse(res, as64(r_res)[:, None]) + 4.0 * mse(net(as64(X_bc)), as64(u_bc)[:, None]) + \
            2.0 * mse(net(as64(X_ic)), as64(u_ic)[:, None])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1)
        opt.step()
        sch.step(loss)
        hist.append(loss.item())
    return np.array(hist)


def training_reference(case, batches=None):
    """{"loss": (STEPS,)} of one case through conftest.cached_oracle, keyed on the initial weights and the batches."""
    batches = expected_batches() if batches is None else batches
    model = TT.initial_model(case)
    flat0 = np.concatenate([p.detach().numpy().reshape(-1) for p in model.parameters()]).astype(np.float32)
    inputs = [flat0]
    for b in batches:
        inputs += [np.asarray(a, dtype=np.float32) for a in b]
    return cached_oracle(f"coeftrain_{case}", inputs, lambda: {"loss": replay(model, batches)})
