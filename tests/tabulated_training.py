"""Float64 replay of a tabulated training run (FusedTrainer(..., dataset=) with the device gather): the seeded dataset,
the minibatches the gather picks (tabulated_reference.dataset_indices) and the loss history of a float64 copy of
oracle.solver.OracleSolver trained on them as oracle/solver.train_step trains: loss = 2 L_r + 4 L_bc + 2 L_ic,
clip_grad_norm_(1), Adam, ReduceLROnPlateau, with the dataset's targets and its residual
c_u u + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy).

The GPU test reads the batches back from the step's buffers and hands them to ``training_reference``; the records
committed under tests/golden/oracle/ (make_oracle_cache.py) are computed from ``expected_batches``, which the
device must reproduce bit for bit for a record's digest to match.
"""
import numpy as np
import torch

import tabulated_reference as T
from step_reference import as64, batch_inputs, flat_of, record

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


def replay(model, batches, residual, objective=None, value=None, extra=(), extra_group=False, clip_extra=False,
           set_grads=None):
    """Loss history (steps,) of the float64 copy of ``model`` trained on ``batches``, one step per batch: Adam at the
    model's lr, ReduceLROnPlateau(0.9, 1000), the derivatives of the residual by autograd, clip_grad_norm_(1) and the step.
    A batch is (X_ic, X_bc, X_res, ic targets, bc targets, residual targets, ...).  Every replay of the suite but L-BFGS's
    is a call of this one with what is its own:

    ``residual(batch, jets)``: the residual part of the loss; ``jets[k]`` = (u, u_t, u_x, u_y, u_xx, u_yy), (B, 1) each, of
    output k at the batch's residual points.  ``value(net, X, target)``: the BC / IC part (default: the MSE).
    ``objective(l_r, l_bc, l_ic)``: the scalar that is descended, handed to the scheduler and recorded (default
    2 l_r + 4 l_bc + 2 l_ic).  ``extra``: tensors trained next to the model's, in its param group or (``extra_group``) in
    one of their own; the clip covers the model's parameters only unless ``clip_extra``.  ``set_grads(parts, params,
    batch)`` writes the parameters' ``.grad`` itself, in place of ``loss.backward()``.  Each callable runs exactly once per
    step, in the order residual, value (BC), value (IC), objective, set_grads; the variants rely on that to record what
    else they keep per step (coefficients, weights, the annealing of eps)."""
    from oracle import statevector as sv
    model = model.double()
    ql = model.quantum_layer

    def net(x):     # OracleSolver.forward without its float32 cast of the expectation values
        q = sv.circuit_expvals(model.preprocessor(x), ql.params, ql.q_ansatz, ql.num_qubits, ql._haar, "angle")
        return model.postprocessor(q.T.reshape(-1, ql.num_qubits))

    mse = torch.nn.MSELoss()
    value = value or (lambda net, X, target: mse(net(as64(X)), as64(target)[:, None]))
    objective = objective or (lambda l_r, l_bc, l_ic: 2.0 * l_r + 4.0 * l_bc + 2.0 * l_ic)
    prm, extra = list(model.parameters()), list(extra)
    groups = [prm, extra] if extra_group else [prm + extra]
    opt = torch.optim.Adam([{"params": g} for g in groups if g], lr=model.args["lr"])
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=1000)
    g = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    hist = []
    for b in batches:
        opt.zero_grad()
        t, x, y = [as64(b[2])[:, k:k + 1].requires_grad_(True) for k in range(3)]
        f = net(torch.cat((t, x, y), 1))
        jets = []
        for k in range(f.shape[1]):
            u = f[:, k:k + 1]
            u_x, u_y = g(u, x), g(u, y)
            jets.append((u, g(u, t), u_x, u_y, g(u_x, x), g(u_y, y)))
        parts = (residual(b, jets), value(net, b[1], b[4]), value(net, b[0], b[3]))
        loss = objective(*parts)
        if set_grads is None:
            loss.backward()
        else:
            set_grads(parts, prm, b)
        torch.nn.utils.clip_grad_norm_(prm + extra if clip_extra else prm, max_norm=1)
        opt.step()
        sch.step(loss)
        hist.append(loss.item())
    return np.array(hist)


def operator_residual(jets, c_u, c_t, c_x, c_y, d_xx, d_yy, c_3=None):
    """c_u u [+ c_3 u^3] + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy) of one output's jets."""
    u, u_t, u_x, u_y, u_xx, u_yy = jets
    head = c_u * u if c_3 is None else c_u * u + c_3 * u ** 3
    return head + c_t * u_t + c_x * u_x + c_y * u_y - (d_xx * u_xx + d_yy * u_yy)


def data_residual(coeffs=T.COEFFS, c_u=T.C_U):
    """The ``residual`` of ``replay`` on a dataset's scalar operator: the MSE against the batch's residual targets."""
    return lambda b, jets: torch.nn.functional.mse_loss(operator_residual(jets[0], c_u, *coeffs), as64(b[5])[:, None])


def training_job(case, batches=None):
    batches = expected_batches() if batches is None else batches
    model = initial_model(case)
    return record(f"tabtrain_{case}", [flat_of(model), T.COEFFS + (T.C_U,)] + batch_inputs(*batches),
                  lambda: {"loss": replay(model, batches, data_residual())})


def training_reference(case, batches=None):
    """{"loss": (STEPS,)} of one case through conftest.cached_oracle, keyed on the initial weights and the batches."""
    return training_job(case, batches).get()


def oracle_jobs():
    return [training_job(c) for c in TRAIN_CASES]
