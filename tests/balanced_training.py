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
from conftest import cached_oracle

TRAIN_CASES, BATCH, STEPS, N_IC, N_BC = TT.TRAIN_CASES, TT.BATCH, TT.STEPS, TT.N_IC, TT.N_BC
dataset_arrays, expected_batches = TT.dataset_arrays, TT.expected_batches


def replay(model, batches, p0=BR.P0, scale=BR.SCALE, w=BR.W, hold=False, coeffs=T.COEFFS, c_u=T.C_U):
    """(history of F (steps,), effective weights w_k e_k USED in each step (steps, 3)) of the float64 copy of ``model``
    and the balancer trained on ``batches``."""
    from oracle import statevector as sv
    model = model.double()
    ql = model.quantum_layer

    def net(x):     # OracleSolver.forward without its float32 cast of the expectation values
        q = sv.circuit_expvals(model.preprocessor(x), ql.params, ql.q_ansatz, ql.num_qubits, ql._haar, "angle")
        return model.postprocessor(q.T.reshape(-1, ql.num_qubits))

    p = torch.tensor(np.asarray(p0, dtype=np.float32).astype(np.float64), requires_grad=not hold)
    sc = torch.tensor(np.asarray(scale, dtype=np.float32).astype(np.float64))
    wt = torch.tensor(np.asarray(w, dtype=np.float64))
    groups = [{"params": list(model.parameters())}] + ([] if hold else [{"params": [p]}])
    opt = torch.optim.Adam(groups, lr=model.args["lr"])
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=1000)
    c_t, c_x, c_y, d_xx, d_yy = coeffs
    g = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    mse = torch.nn.MSELoss()
    hist, whist = [], []
    for X_ic, X_bc, X_res, u_ic, u_bc, r_res in batches:
        as64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
        opt.zero_grad()
        t, x, y = [as64(X_res)[:, k:k + 1].requires_grad_(True) for k in range(3)]
        u = net(torch.cat((t, x, y), 1))
        u_x, u_y = g(u, x), g(u, y)
        res = c_u * u + c_t * g(u, t) + c_x * u_x + c_y * u_y - (d_xx * g(u_x, x) + d_yy * g(u_y, y))
        parts = torch.stack([mse(res, as64(r_res)[:, None]), mse(net(as64(X_bc)), as64(u_bc)[:, None]),
                             mse(net(as64(X_ic)), as64(u_ic)[:, None])])
        s = sc * p
        we = wt * torch.exp(-s)
        whist.append(we.detach().numpy().copy())
        F = (we * parts + s).sum()
        F.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1)      # the balancer is not clipped
        opt.step()
        sch.step(F)
        hist.append(F.item())
    return np.array(hist), np.array(whist)


def training_reference(case, batches=None, hold=False):
    """{"loss": (STEPS,), "weights": (STEPS, 3)} of one case through conftest.cached_oracle, keyed on the initial weights,
    the balancer and the batches."""
    batches = expected_batches() if batches is None else batches
    model = TT.initial_model(case)
    flat0 = np.concatenate([p.detach().numpy().reshape(-1) for p in model.parameters()]).astype(np.float32)
    inputs = [flat0, np.asarray(T.COEFFS + (T.C_U,), dtype=np.float32)] + \
        [np.asarray(a, dtype=np.float32) for a in (BR.SCALE, BR.P0, BR.W)]
    for b in batches:
        inputs += [np.asarray(a, dtype=np.float32) for a in b]

    def compute():
        loss, weights = replay(model, batches, hold=hold)
        return {"loss": loss, "weights": weights}
    return cached_oracle(f"baltrain_{case}" + ("_hold" if hold else ""), inputs, compute)
