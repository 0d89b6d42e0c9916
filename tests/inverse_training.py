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
import itertools

import numpy as np
import torch

import inverse_reference as IR
import tabulated_reference as T
import tabulated_training as TT
from step_reference import as64, batch_inputs, flat_of, record

TRAIN_CASES, BATCH, STEPS, N_IC, N_BC = TT.TRAIN_CASES, TT.BATCH, TT.STEPS, TT.N_IC, TT.N_BC
dataset_arrays, expected_batches = TT.dataset_arrays, TT.expected_batches


def operator_run(model, batches, p0=IR.P0, base=IR.BASE, scale=IR.SCALE, hold=False, every=1):
    """(loss history, (steps / every, 7) coefficients USED in steps 1, 1 + every, ...) of the float64 copy of ``model``
    and the operator trained on ``batches`` (an iterable): tabulated_training.replay with ``p`` in the model's param group
    and under its clip."""
    p = torch.tensor(np.asarray(p0, dtype=np.float32).astype(np.float64), requires_grad=not hold)
    chist, count = [], itertools.count()

    def residual(b, jets):
        c = IR.operator(p, base, scale)
        if next(count) % every == 0:
            chist.append(c.detach().numpy().copy())
        return torch.nn.functional.mse_loss(TT.operator_residual(jets[0], *c), as64(b[5])[:, None])
    hist = TT.replay(model, batches, residual, extra=[] if hold else [p], clip_extra=True)
    return hist, np.array(chist)


def training_job(case, batches=None, hold=False):
    batches = expected_batches() if batches is None else batches
    model = TT.initial_model(case)

    def compute():
        loss, coef = operator_run(model, batches, hold=hold)
        return {"loss": loss, "coef": coef}
    return record(f"invtrain_{case}", [flat_of(model), IR.BASE, IR.SCALE, IR.P0] + batch_inputs(*batches), compute,
                  variant="hold" if hold else "")


def training_reference(case, batches=None, hold=False):
    """{"loss": (STEPS,), "coef": (STEPS, 7)} of one case through conftest.cached_oracle, keyed on the initial weights,
    the operator and the batches."""
    return training_job(case, batches, hold).get()


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


def recovery_job():
    from oracle import solver as osol

    def compute():
        torch.manual_seed(1)
        model = osol.OracleSolver(REC_ARGS, device=torch.device("cpu"))
        base, scale = recovery_operator()
        _, coef = operator_run(model, recovery_batches(), p0=[0.0] * IR.N_OP, base=base, scale=scale, every=REC_EVERY)
        return {"c_x": coef[:, IR.COLS.index("c_x")]}
    return record("inv_recover_cascade2_H16",
                  list(recovery_dataset()) + [np.array([REC_SEED, REC_STEPS, REC_EVERY], dtype=np.int64)], compute, dtype=None)


def recovery_reference():
    """{"c_x": (REC_STEPS / REC_EVERY,)}: c_x used in steps 1, 101, 201, ... of the float64 replay, through
    conftest.cached_oracle, keyed on the dataset and the seed (the batches follow from both)."""
    return recovery_job().get()


def oracle_jobs():
    return [training_job(c, hold=h) for c in TRAIN_CASES for h in (False, True)] + [recovery_job()]
