"""Float64 replays of inverse-problem training runs (InverseTrainer with the device gather).

``training_reference``: the dataset, sizes, seed and batches of tests/tabulated_training.py, the operator of
tests/inverse_reference.py (BASE, SCALE, p starting at P0) and the loss and coefficient histories of the float64
OracleSolver copy trained on them with ``p`` as one more Adam parameter (same lr, one clip over all of them).
``hold=True``: the same replay with the operator held at its initial value, the negative control of the coefficient check.

``recovery_*``: the identification run of the GPU test.  u* = sin 2 pi x cos pi y exp(-t / 2) + 0.3 (tabulated_reference.u_star)
observed at 2 x 1 024 interior points, r = u*_t + 0.8 u*_x - 0.05 (u*_xx + u*_yy) at 4 096 residual points, all uniform in the
unit cube; c_t, d_xx, d_yy fixed at their true values and c_x learnt from 0.2.  The committed record holds c_x every 100
steps of the float64 replay on the float32 dataset and the Philox batches of the test's seed.  On these batches the
replay overshoots to 1.03 near step 800, is back at 0.84 by step 1 000 and 0.820 by step 2 000, and lies in 0.8137 .. 0.8169
over steps 3 000 .. 4 000 (the finite dataset and the 16-unit network leave a bias of about +0.015): the run is 4 000 steps
long, twice the 2 000 a replay on torch.randint batches of a float64 dataset needed, and the learning rate stays 0.005.
"""
import numpy as np
import torch

import inverse_reference as IR
import tabulated_reference as T
import tabulated_training as TT
from conftest import cached_oracle

TRAIN_CASES, BATCH, STEPS, N_IC, N_BC = TT.TRAIN_CASES, TT.BATCH, TT.STEPS, TT.N_IC, TT.N_BC
dataset_arrays, expected_batches = TT.dataset_arrays, TT.expected_batches


def _net(model):
    from oracle import statevector as sv
    ql = model.quantum_layer

    def net(x):     # OracleSolver.forward without its float32 cast of the expectation values
        q = sv.circuit_expvals(model.preprocessor(x), ql.params, ql.q_ansatz, ql.num_qubits, ql._haar, "angle")
        return model.postprocessor(q.T.reshape(-1, ql.num_qubits))
    return net


def replay(model, batches, p0=IR.P0, base=IR.BASE, scale=IR.SCALE, hold=False, every=1):
    """(loss history, (steps / every, 7) coefficients USED in steps 1, 1 + every, ...) of the float64 copy of ``model``
    and the operator trained on ``batches`` (an iterable)."""
    model = model.double()
    net = _net(model)
    p = torch.tensor(np.asarray(p0, dtype=np.float32).astype(np.float64), requires_grad=not hold)
    params = list(model.parameters()) + ([] if hold else [p])
    opt = torch.optim.Adam(params, lr=model.args["lr"])
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=1000)
    g = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    mse = torch.nn.MSELoss()
    hist, chist = [], []
    for i, (X_ic, X_bc, X_res, u_ic, u_bc, r_res) in enumerate(batches):
        as64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
        c = IR.operator(p, base, scale)
        if i % every == 0:
            chist.append(c.detach().numpy().copy())
        opt.zero_grad()
        t, x, y = [as64(X_res)[:, k:k + 1].requires_grad_(True) for k in range(3)]
        u = net(torch.cat((t, x, y), 1))
        u_x, u_y = g(u, x), g(u, y)
        res = c[0] * u + c[6] * u ** 3 + c[1] * g(u, t) + c[2] * u_x + c[3] * u_y - (c[4] * g(u_x, x) + c[5] * g(u_y, y))
        loss = 2.0 * mse(res, as64(r_res)[:, None]) + 4.0 * mse(net(as64(X_bc)), as64(u_bc)[:, None]) + \
            2.0 * mse(net(as64(X_ic)), as64(u_ic)[:, None])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, max_norm=1)
        opt.step()
        sch.step(loss)
        hist.append(loss.item())
    return np.array(hist), np.array(chist)


def training_reference(case, batches=None, hold=False):
    """{"loss": (STEPS,), "coef": (STEPS, 7)} of one case through conftest.cached_oracle, keyed on the initial weights,
    the operator and the batches."""
    batches = expected_batches() if batches is None else batches
    model = TT.initial_model(case)
    flat0 = np.concatenate([p.detach().numpy().reshape(-1) for p in model.parameters()]).astype(np.float32)
    inputs = [flat0] + [np.asarray(a, dtype=np.float32) for a in (IR.BASE, IR.SCALE, IR.P0)]
    for b in batches:
        inputs += [np.asarray(a, dtype=np.float32) for a in b]

    def compute():
        loss, coef = replay(model, batches, hold=hold)
        return {"loss": loss, "coef": coef}
    return cached_oracle(f"invtrain_{case}" + ("_hold" if hold else ""), inputs, compute)


# ---- recovery of a transport coefficient
REC_DS = (4096, 1024, 1024)
REC_BATCH, REC_N_IC, REC_N_BC, REC_STEPS, REC_EVERY = 64, 21, 21, 4000, 100
REC_SETTLED = 3000          # the float64 replay has settled from here on (tests/test_inverse_cpu.py)
REC_SEED = 0x5EED1234
REC_TRUE, REC_START = 0.8, 0.2
REC_FIXED = {"c_t": 1.0, "d_xx": 0.05, "d_yy": 0.05}
REC_ARGS = {"batch_size": REC_BATCH, "epochs": 1, "lr": 0.005, "seed": 1, "print_every": 10 ** 9, "num_qubits": 2,
            "num_quantum_layers": 1, "classic_network": [3, 16, 1], "q_ansatz": "cascade", "shots": 1024,
            "problem": "diffusion", "solver": "DV", "encoding": "None", "use_ibm_hardware": False}


def recovery_forcing(X):
    """r = u*_t + 0.8 u*_x - 0.05 (u*_xx + u*_yy) of u* = sin 2 pi x cos pi y exp(-t / 2) + 0.3, float64 -> float32."""
    X = np.asarray(X, dtype=np.float64)
    t, x, y = X[:, 0], X[:, 1], X[:, 2]
    e, pi = np.exp(-0.5 * t), np.pi
    s, c, cy = np.sin(2 * pi * x), np.cos(2 * pi * x), np.cos(pi * y)
    w = s * cy * e
    u_t, u_x = -0.5 * w, 2 * pi * c * cy * e
    u_xx, u_yy = -4 * pi * pi * w, -pi * pi * w
    return (u_t + REC_TRUE * u_x - 0.05 * (u_xx + u_yy)).astype(np.float32)


def recovery_dataset():
    """(X_res, r, X_ic, u_ic, X_bc, u_bc) float32: every segment uniform in the unit cube (interior observations)."""
    g = torch.Generator().manual_seed(4242)
    Xr, Xi, Xb = (torch.rand(m, 3, generator=g).to(torch.float32).numpy() for m in REC_DS)
    return Xr, recovery_forcing(Xr), Xi, T.u_star(Xi), Xb, T.u_star(Xb)


def recovery_batches(steps=REC_STEPS, seed=REC_SEED):
    """Generator of the Philox batches of the device gather, step counter 1-based."""
    Xr, rr, Xi, ui, Xb, ub = recovery_dataset()
    for step in range(1, steps + 1):
        kr = T.dataset_indices(0, 0, REC_BATCH, REC_DS[0], seed, step)
        ki = T.dataset_indices(1, 0, REC_N_IC, REC_DS[1], seed, step)
        kb = T.dataset_indices(2, 0, REC_N_BC, REC_DS[2], seed, step)
        yield Xi[ki], Xb[kb], Xr[kr], ui[ki], ub[kb], rr[kr]


def recovery_operator():
    base = [REC_FIXED.get(k, 0.0) for k in IR.COLS]
    scale = [0.0] * IR.N_OP
    base[IR.COLS.index("c_x")], scale[IR.COLS.index("c_x")] = REC_START, 1.0
    return base, scale


def recovery_reference():
    """{"c_x": (REC_STEPS / REC_EVERY,)}: c_x used in steps 1, 101, 201, ... of the float64 replay, through
    conftest.cached_oracle, keyed on the dataset and the seed (the batches follow from both)."""
    from oracle import solver as osol
    inputs = list(recovery_dataset()) + [np.array([REC_SEED, REC_STEPS, REC_EVERY], dtype=np.int64)]

    def compute():
        torch.manual_seed(1)
        model = osol.OracleSolver(REC_ARGS, device=torch.device("cpu"))
        base, scale = recovery_operator()
        _, coef = replay(model, recovery_batches(), p0=[0.0] * IR.N_OP, base=base, scale=scale, every=REC_EVERY)
        return {"c_x": coef[:, IR.COLS.index("c_x")]}
    return cached_oracle("inv_recover_cascade2_H16", inputs, compute)
