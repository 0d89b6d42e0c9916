"""Float64 replay of a tabulated training run (FusedTrainer(..., dataset=) with the device gather): the seeded dataset,
the minibatches the gather picks (tabulated_reference.dataset_indices) and the loss history of a float64 copy of
oracle.solver.OracleSolver trained on them as oracle/solver.train_step trains: loss = 2 L_r + 4 L_bc + 2 L_ic,
clip_grad_norm_(1), Adam, ReduceLROnPlateau, with the dataset's targets and its residual
c_u u + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy).

The GPU test reads the batches back from the step's buffers and hands them to ``training_reference``; the records
committed under tests/golden/oracle/ (make_tabulated_oracle_cache.py) are computed from ``expected_batches``, which the
device must reproduce bit for bit for a record's digest to match.
"""
import numpy as np
import torch

import tabulated_reference as T
from conftest import cached_oracle

TRAIN_CASES = {"cascade4": ("cascade", 4), "layered8": ("layered", 8)}
DS_SIZES = (256, 64, 64)            # residual, IC, BC rows
BATCH, STEPS = 64, 6                # FusedTrainer(model, 64, capacity=6): 64 residual, 21 IC, 21 BC points per step
N_IC = N_BC = BATCH // 3
TRAINER_SEED_AT = 77                # torch.manual_seed before the trainer draws its Philox seed


def base_args(ansatz, n):
    return {"batch_size": BATCH, "epochs": STEPS - 1, "lr": 0.005, "seed": 1, "print_every": 10 ** 9, "num_qubits": n,
            "num_quantum_layers": 1, "classic_network": [3, 50, 1], "q_ansatz": ansatz, "shots": 1024,
            "problem": "diffusion", "solver": "DV", "encoding": "None", "use_ibm_hardware": False}


def dataset_arrays():
    """Seeded float32 dataset in the trainer's boxes: (X_res, r, X_ic, u_ic, X_bc, u_bc) numpy arrays."""
    from oracle import solver as osol
    g = torch.Generator().manual_seed(2024)
    Xr, Xi, Xb = [(torch.tensor(b[0]) + (torch.tensor(b[1]) - torch.tensor(b[0])) * torch.rand(m, 3, generator=g))
                  .to(torch.float32).numpy() for b, m in zip((osol.BOX_DOM, osol.BOX_IC, osol.BOX_BC1), DS_SIZES)]
    return Xr, T.r_star(Xr), Xi, T.u_star(Xi), Xb, T.u_star(Xb)


def trainer_seed():
    """The Philox seed a FusedTrainer constructed right after torch.manual_seed(TRAINER_SEED_AT) draws."""
    torch.manual_seed(TRAINER_SEED_AT)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def expected_batches(seed=None):
    """Per step (1-based counter, as FusedStep.run advances it): (X_ic, X_bc, X_res, u_ic, u_bc, r_res)."""
    seed = trainer_seed() if seed is None else seed
    Xr, rr, Xi, ui, Xb, ub = dataset_arrays()
    out = []
    for step in range(1, STEPS + 1):
        kr = T.dataset_indices(0, 0, BATCH, DS_SIZES[0], seed, step)
        ki = T.dataset_indices(1, 0, N_IC, DS_SIZES[1], seed, step)
        kb = T.dataset_indices(2, 0, N_BC, DS_SIZES[2], seed, step)
        out.append((Xi[ki], Xb[kb], Xr[kr], ui[ki], ub[kb], rr[kr]))
    return out


def initial_model(case):
    """The float32 OracleSolver a DVPDESolver built after torch.manual_seed(1) starts equal to (same RNG consumption)."""
    from oracle import solver as osol
    ans, n = TRAIN_CASES[case]
    torch.manual_seed(1)
    return osol.OracleSolver(base_args(ans, n), device=torch.device("cpu"))


def replay(model, batches, coeffs=T.COEFFS, c_u=T.C_U):
    """Loss history of the float64 copy of ``model`` trained on ``batches``."""
    from oracle import statevector as sv
    model = model.double()
    ql = model.quantum_layer

    def net(x):     # OracleSolver.forward without its float32 cast of the expectation values
        q = sv.circuit_expvals(model.preprocessor(x), ql.params, ql.q_ansatz, ql.num_qubits, ql._haar, "angle")
        return model.postprocessor(q.T.reshape(-1, ql.num_qubits))

    opt = torch.optim.Adam(model.parameters(), lr=model.args["lr"])
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=1000)
    c_t, c_x, c_y, d_xx, d_yy = coeffs
    g = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    mse = torch.nn.MSELoss()
    hist = []
    for X_ic, X_bc, X_res, u_ic, u_bc, r_res in batches:
        as64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
        opt.zero_grad()
        t, x, y = [as64(X_res)[:, k:k + 1].requires_grad_(True) for k in range(3)]
        u = net(torch.cat((t, x, y), 1))
        u_x, u_y = g(u, x), g(u, y)
        res = c_u * u + c_t * g(u, t) + c_x * u_x + c_y * u_y - (d_xx * g(u_x, x) + d_yy * g(u_y, y))
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
    model = initial_model(case)
    flat0 = np.concatenate([p.detach().numpy().reshape(-1) for p in model.parameters()]).astype(np.float32)
    inputs = [flat0, np.asarray(T.COEFFS + (T.C_U,), dtype=np.float32)]
    for b in batches:
        inputs += [np.asarray(a, dtype=np.float32) for a in b]
    return cached_oracle(f"tabtrain_{case}", inputs, lambda: {"loss": replay(model, batches)})
