"""Float64 references of the causal step (qc_fused_pinn_causal_step, qc_sample_dataset_slabs, qc_causal_fold,
include/qcpinn_hip.h): the tabulated step with the residual of time slab i weighted by

    W_i = exp(-eps sum_{k<i} L_k),   W_0 = 1,   L_r^c = (1/M) sum_i W_i L_i,

L_i the mean squared residual of the batch's points of slab i, the weights constants when differentiating.  Tile
tau = g / 64 of the residual batch (g the global point index) holds points of slab tau mod M.

``slab_table`` / ``slab_rows``: the host's sort and the rows the device gather picks, restated on numpy and
tests/philox_reference.  ``slab_gradients``: grad L_i of every slab and grad L_bc, grad L_ic one by one, the way the device
forms the causal gradient (partial rows summed with one scalar each); ``combine`` forms weights and gradient from them for
any eps, ``autograd_gradient`` differentiates 2 L_r^c + 4 L_bc + 2 L_ic with detached weights in one piece (the CPU test
compares the two).  ``weights`` and ``anneal`` restate the record's arithmetic: cumulative sums and exp in float64, W
rounded to float32, W_{M-1} > delta compared in float32, eps = float32(min(eps * growth, eps_max)).

``causal_run``: the training loop of tests/tabulated_training.py under those weights, with the annealing; ``unit=True`` is
the control with every weight 1.
"""
import numpy as np
import torch

import mlp_reference as R
import philox_reference as PR
import tabulated_reference as T
import tabulated_training as TT
from conftest import pkg
from step_reference import Step, as64, batch_inputs, flat_of, haar_for, mse_to, record, step_inputs

F32 = lambda a: np.asarray(a, dtype=np.float32)
W3 = (2.0, 4.0, 2.0)
STEPS, N_IC, N_BC = 6, 21, 21
TRAIN_CASES = {"cascade4": ("cascade", 4), "cascade2": ("cascade", 2), "layered6": ("layered", 6)}
# id -> (B_res, M, eps0, growth, eps_max, delta): chosen with the replay alone so that W_{M-1} of step 1 lies in [0.05, 0.9]
# and eps is raised in some of the six steps and held in others (test_causal_cpu.py checks both on the committed records)
CONFIGS = {"b128m2": (128, 2, 1.0, 1.5, 100.0, 0.25), "b512m4": (512, 4, 0.3, 1.5, 100.0, 0.26)}
HBM_CASE = ("cascade", 9, 1, 128, 2, 3, 2)      # ansatz, n, L, B_res, M, n_ic, n_bc
HBM_EPS = 1.0


# ---------------------------------------------------------------- host sort and device gather
def slab_table(t, M, t_range=None):
    """(order, slab_lo): the stable ascending order of ``t`` and the (M + 1,) int64 offsets of M equal-width slabs in it:
    slab i holds edge_i <= t < edge_{i+1}, rows on an inner edge join the upper slab."""
    t = np.asarray(t, dtype=np.float64)
    order = np.argsort(t, kind="stable")
    ts = t[order]
    lo, hi = (float(ts[0]), float(ts[-1])) if t_range is None else t_range
    edges = torch.linspace(lo, hi, M + 1, dtype=torch.float64).numpy()
    inner = np.searchsorted(ts, edges[1:-1], side="left")
    return order, np.concatenate([[0], inner, [len(ts)]]).astype(np.int64)


def slab_rows(offset, count, M, slab_lo, seed, step):
    """(count,) int64 rows of residual points offset .. offset + count - 1 under the slab rule."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    g = np.uint64(offset) + np.arange(count, dtype=np.uint64)
    ctr = (g & PR.MASK, g >> PR.S32, step & 0xFFFFFFFF, step >> 32)
    w0 = PR.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[0]
    s = ((g >> np.uint64(6)) % np.uint64(M)).astype(np.int64)
    lo = np.asarray(slab_lo, dtype=np.int64)
    width = (lo[s + 1] - lo[s]).astype(np.uint64)
    return lo[s] + ((w0 * width) >> PR.S32).astype(np.int64)


def slab_of_points(count, M, offset=0):
    """(count,) slab index of every point of a residual batch."""
    return ((offset + np.arange(count)) // 64) % M


# ---------------------------------------------------------------- the record's arithmetic
def weights(L, eps):
    """(W float32 (M,), W float64) from the slab losses and the float32 eps the record holds."""
    L = np.asarray(L, dtype=np.float64)
    cum = np.concatenate([[0.0], np.cumsum(L)[:-1]])
    W = np.exp(-float(np.float32(eps)) * cum)
    return W.astype(np.float32), W


def anneal(eps, n_raised, W_last, growth, eps_max, delta):
    """(eps, n_raised) of the next step."""
    eps = np.float32(eps)
    if np.float32(W_last) > np.float32(delta) and eps < np.float32(eps_max):
        eps = np.float32(min(float(eps) * float(np.float32(growth)), float(np.float32(eps_max))))
        n_raised += 1
    return eps, n_raised


# ---------------------------------------------------------------- one step: per-slab gradients
def _slab_losses(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, M, coeffs, c_u):
    """(the Step, [L_0 .. L_{M-1}], L_bc, L_ic): the data step's parts with the residual's mean taken slab by slab."""
    s = Step(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res)
    slab = torch.as_tensor(slab_of_points(len(r_res), M))

    def slab_means(u):
        sq = (c_u * u[0] + R.residual(u, coeffs) - as64(r_res)) ** 2
        return [sq[slab == i].mean() for i in range(M)]
    return (s,) + s.losses(slab_means, mse_to(u_bc, u_ic))


def slab_gradients(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, M, coeffs=T.COEFFS,
                   c_u=T.C_U):
    """{"g_slab": (M, NP) grad L_i, "L": (M,), "g_bc", "g_ic": (NP,), "vals": (L_bc, L_ic)} float64."""
    s, Ls, l_bc, l_ic = _slab_losses(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, M,
                                     coeffs, c_u)
    return {"g_slab": np.array([s.grad(Li, retain_graph=True) for Li in Ls]), "L": np.array([Li.item() for Li in Ls]),
            "g_bc": s.grad(l_bc), "g_ic": s.grad(l_ic), "vals": np.array([l_bc.item(), l_ic.item()])}


def combine(rec, eps, unit=False, w=W3):
    """(grad (NP,), parts (L_r^c, L_bc, L_ic), W (M,)) of 2 L_r^c + 4 L_bc + 2 L_ic from a ``slab_gradients`` record, the
    way the device forms it: per-slab gradients summed with one scalar each.  ``unit``: every weight 1."""
    M = len(rec["L"])
    W = np.ones(M) if unit else weights(rec["L"], eps)[1]
    g = w[0] * (W[:, None] * rec["g_slab"]).sum(0) / M + w[1] * rec["g_bc"] + w[2] * rec["g_ic"]
    return g, np.array([float((W * rec["L"]).sum() / M), rec["vals"][0], rec["vals"][1]]), W


def autograd_gradient(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, M, eps,
                      coeffs=T.COEFFS, c_u=T.C_U, w=W3):
    """The same gradient in one piece: torch autograd of w_res L_r^c + w_bc L_bc + w_ic L_ic with the weights detached."""
    s, Ls, l_bc, l_ic = _slab_losses(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, M,
                                     coeffs, c_u)
    L = torch.stack(Ls)
    cum = torch.cumsum(L, 0) - L
    W = torch.exp(-float(np.float32(eps)) * cum).detach()
    return s.weighted(((W * L).mean(), l_bc, l_ic), w)[0]


def step_case_inputs(ansatz, n, L, B_res, n_ic, n_bc, H=T.H, salt=11):
    """Seeded weights, points and targets of a one-step case (the rule of tabulated_reference.case_inputs)."""
    n_theta = L * pkg("circuits").params_per_layer(ansatz, n)
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=salt)
    return flat, X_ic, X_bc, X_res, T.u_star(X_ic), T.u_star(X_bc), T.r_star(X_res)


def hbm_job():
    ans, n, L, B_res, M, n_ic, n_bc = HBM_CASE
    P = int(pkg("circuits").params_per_layer(ans, n))
    flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res = step_case_inputs(ans, n, L, B_res, n_ic, n_bc)

    def compute():
        return slab_gradients(flat, T.H, n, L * P, (L, P), ans, haar_for(n, 1),
                              *(torch.as_tensor(x).double() for x in (X_ic, X_bc, X_res)), u_ic, u_bc, r_res, M)
    return record(f"causal_{ans}_n{n}_L{L}_r{B_res}_m{M}_i{n_ic}_b{n_bc}",
                  (flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res, T.COEFFS + (T.C_U,), [M]), compute)


def hbm_reference():
    """slab_gradients of HBM_CASE through conftest.cached_oracle."""
    return hbm_job().get()


# ---------------------------------------------------------------- training replay
def base_args(ansatz, n, batch):
    return dict(TT.base_args(ansatz, n), batch_size=batch, epochs=STEPS - 1)


def sorted_dataset(M):
    """TT.dataset_arrays with the residual segment sorted by t, and its slab offsets."""
    Xr, rr, Xi, ui, Xb, ub = TT.dataset_arrays()
    order, lo = slab_table(Xr[:, 0], M)
    return (Xr[order], rr[order], Xi, ui, Xb, ub), lo


def expected_batches(config, seed=None):
    """Per step (1-based counter): (X_ic, X_bc, X_res, u_ic, u_bc, r_res) as the causal trainer's gather fills them."""
    B_res, M = CONFIGS[config][:2]
    seed = TT.trainer_seed() if seed is None else seed
    (Xr, rr, Xi, ui, Xb, ub), lo = sorted_dataset(M)
    out = []
    for step in range(1, STEPS + 1):
        kr = slab_rows(0, B_res, M, lo, seed, step)
        ki = T.dataset_indices(1, 0, N_IC, len(Xi), seed, step)
        kb = T.dataset_indices(2, 0, N_BC, len(Xb), seed, step)
        out.append((Xi[ki], Xb[kb], Xr[kr], ui[ki], ub[kb], rr[kr]))
    return out


def initial_model(case, batch):
    from oracle import solver as osol
    ans, n = TRAIN_CASES[case]
    torch.manual_seed(1)
    return osol.OracleSolver(base_args(ans, n, batch), device=torch.device("cpu"))


def causal_run(model, batches, M, eps0, growth, eps_max, delta, unit=False, coeffs=T.COEFFS, c_u=T.C_U):
    """{"loss": (steps,), "W": (steps, M) float64 weights USED in each step, "L": (steps, M), "eps": (steps,) float32 eps
    used in each step, "eps_end": (1,), "n_raised": (1,), "raised": (steps,) bool} of the float64 copy of ``model``:
    tabulated_training.replay with the residual part taken slab by slab under the weights, and the annealing."""
    state = {"eps": np.float32(eps0), "n_raised": 0}
    Wh, Lh, eh, rh = [], [], [], []

    def residual(b, jets):      # once per step (the contract of TT.replay): it also advances the annealing
        res = TT.operator_residual(jets[0], c_u, *coeffs)
        sq = ((res - as64(b[5])[:, None]) ** 2).reshape(-1)
        slab = torch.as_tensor(slab_of_points(len(b[5]), M))
        L = torch.stack([sq[slab == i].mean() for i in range(M)])
        W32, W = weights(L.detach().numpy(), state["eps"])
        Wh.append(W)
        Lh.append(L.detach().numpy().copy())
        eh.append(state["eps"])
        state["eps"], now = anneal(state["eps"], state["n_raised"], W32[-1], growth, eps_max, delta)
        rh.append(now != state["n_raised"])
        state["n_raised"] = now
        return ((torch.ones(M, dtype=torch.float64) if unit else torch.as_tensor(W)) * L).mean()
    hist = TT.replay(model, batches, residual)
    return {"loss": hist, "W": np.array(Wh), "L": np.array(Lh), "eps": np.array(eh, dtype=np.float32),
            "eps_end": np.array([state["eps"]], dtype=np.float32), "n_raised": np.array([state["n_raised"]]),
            "raised": np.array(rh)}


def training_job(case, config, batches=None, unit=False):
    B_res, M, eps0, growth, eps_max, delta = CONFIGS[config]
    batches = expected_batches(config) if batches is None else batches
    model = initial_model(case, B_res)
    return record(f"causaltrain_{case}_{config}",
                  [flat_of(model), T.COEFFS + (T.C_U,), [M, eps0, growth, eps_max, delta]] + batch_inputs(*batches),
                  lambda: causal_run(model, batches, M, eps0, growth, eps_max, delta, unit=unit), variant="unit" if unit else "")


def training_reference(case, config, batches=None, unit=False):
    """``causal_run`` of one case and configuration through conftest.cached_oracle, keyed on the initial weights, the
    configuration and the batches."""
    return training_job(case, config, batches, unit).get()


def oracle_jobs():
    return [hbm_job()] + [training_job(c, k, unit=u) for c in TRAIN_CASES for k in CONFIGS for u in (False, True)]
