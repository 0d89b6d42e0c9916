"""Float64 references of the gradient-norm step (qc_gradnorm_fold, qc_fused_pinn_gradnorm_step, include/qcpinn_hip.h):
Wang, Teng, Perdikaris 2021, Algorithm 1 on the three loss classes of the fused step,

    hat_k = max_j |G_res[j]| / mean_j |G_k[j]|,   lam_k <- (1 - alpha) lam_k + alpha hat_k,   k in {BC, IC},
    flat  = G_res + lam_bc G_bc + lam_ic G_ic     (the weights after this step's update),

G_c the gradient of class c as the rows of the step carry it (w_c grad L_c).

``class_sums`` / ``Record``: the restatement of the two launches on a row matrix: float64 column sums per class, then the
statistics, the update every ``every`` calls, the combination and the history row.  ``dtype=np.float32`` mirrors the
device's storage (weights rounded to float32, the combination as two fused multiply-adds in float32); ``np.float64`` keeps
everything in double (the CPU test compares that with Algorithm 1 written directly on torch).

``class_gradients``: the three per-class gradients of one step from three autograd passes over the float64 oracle (the
tabulated, the analytic and the coefficient-table problem), through conftest.cached_oracle.  ``gradnorm_run``: the training loop
of tests/tabulated_training.py with three backward passes per step, the weights, clip, Adam and plateau; ``unit=True`` is
the control with both weights held at 1.
"""
import numpy as np
import torch

import coef_reference as CF
import tabulated_reference as T
import tabulated_training as TT
from conftest import pkg
from step_reference import batch_inputs, flat_of, haar_for, record, reference_loss, step_inputs

F32 = lambda a: np.asarray(a, dtype=np.float32)
W3 = (2.0, 4.0, 2.0)
STATE_WORDS, HIST_COLS = 16, 7


# ---------------------------------------------------------------- the two launches, restated
def class_sums(part, n_res, n_ic, n_bc, ncols):
    """(3, ncols) float64 column sums of the residual, IC and BC rows of a row matrix (rows in that order)."""
    p = np.asarray(part, dtype=np.float64)[:, :ncols]
    cut = (0, n_res, n_res + n_ic, n_res + n_ic + n_bc)
    return np.stack([p[cut[c]:cut[c + 1]].sum(0) for c in range(3)])


def fmaf32(a, b, c):
    """float32 fused multiply-add: the product of two floats is exact in double; one rounding of the sum to double ahead
    of the rounding to float (the rare double rounding lies inside the 2^-23 the tests allow)."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


class Record:
    """The device record and its arithmetic.  ``dtype``: np.float32 (the device's storage) or np.float64."""

    def __init__(self, alpha=0.1, every=10, lam_max=1e4, init=(1.0, 1.0), dtype=np.float32, w=(1.0, 1.0, 1.0)):
        f = dtype
        self.f, self.alpha, self.lam_max, self.every = f, float(np.float32(alpha) if f is np.float32 else alpha), \
            float(np.float32(lam_max) if f is np.float32 else lam_max), int(every)
        self.lam_bc, self.lam_ic = f(init[0]), f(init[1])
        self.n_steps = self.n_updates = 0
        self.m_r = self.a_bc = self.a_ic = self.hat_bc = self.hat_ic = f(0.0)
        self.w = tuple(float(v) for v in w)
        self.rows = []

    def step(self, G, n_ic=1, n_bc=1):
        """``G`` (3, NP + 3): the class sums G_res, G_ic, G_bc with their loss columns.  Returns flat (NP + 3,) and appends
        the history row (lam_bc, lam_ic, m_r, a_bc, a_ic, lambda-weighted loss, updated)."""
        f = self.f
        G = np.asarray(G, dtype=f)
        NP = G.shape[1] - 3
        g_res, g_ic, g_bc = G[0, :NP], G[1, :NP], G[2, :NP]
        update = self.n_steps % self.every == 0
        if update:
            m = np.abs(g_res).max()                                   # numpy's max keeps a NaN
            mr = float(m)
            ab, ai = float(np.abs(g_bc).astype(np.float64).sum() / NP), float(np.abs(g_ic).astype(np.float64).sum() / NP)
            ok_bc = n_bc > 0 and np.isfinite(mr) and np.isfinite(ab) and ab > 0.0
            ok_ic = n_ic > 0 and np.isfinite(mr) and np.isfinite(ai) and ai > 0.0
            hb, hi = (mr / ab if ok_bc else 0.0), (mr / ai if ok_ic else 0.0)
            if ok_bc:
                self.lam_bc = f(min(self.lam_max, (1.0 - self.alpha) * float(self.lam_bc) + self.alpha * hb))
            if ok_ic:
                self.lam_ic = f(min(self.lam_max, (1.0 - self.alpha) * float(self.lam_ic) + self.alpha * hi))
            self.m_r, self.a_bc, self.a_ic, self.hat_bc, self.hat_ic = f(m), f(ab), f(ai), f(hb), f(hi)
            self.n_updates += 1
        if f is np.float32:
            grad = fmaf32(self.lam_ic, g_ic, fmaf32(self.lam_bc, g_bc, g_res))
        else:
            grad = g_res + self.lam_bc * g_bc + self.lam_ic * g_ic
        loss = (G[0, NP:] + G[1, NP:]) + G[2, NP:]
        wl = float(self.w[0] * loss[0] + float(self.lam_bc) * self.w[1] * loss[1] + float(self.lam_ic) * self.w[2] * loss[2])
        self.rows.append([self.lam_bc, self.lam_ic, self.m_r, self.a_bc, self.a_ic, wl, 1.0 if update else 0.0])
        self.n_steps += 1
        return np.concatenate([grad, loss]).astype(f)

    def state(self):
        """The record as the engine's ``read_state`` gives it."""
        return {"lam_bc": float(self.lam_bc), "lam_ic": float(self.lam_ic), "n_steps": self.n_steps, "hist_base": 0,
                "n_updates": self.n_updates, "m_r": float(self.m_r), "a_bc": float(self.a_bc), "a_ic": float(self.a_ic),
                "hat_bc": float(self.hat_bc), "hat_ic": float(self.hat_ic)}

    def history(self):
        return np.array(self.rows, dtype=np.float64).reshape(-1, HIST_COLS)


# ---------------------------------------------------------------- one step: the three class gradients
# id -> (kind, ansatz, n, L, B_res, n_ic, n_bc): the base batch is two residual tiles, one IC tile, a full and a partial BC tile
STEP_CASES = {
    "reg_cascade4": ("tab", "cascade", 4, 1, 128, 64, 70),
    "reg_cascade2": ("tab", "cascade", 2, 1, 128, 64, 70),
    "lanes_layered6": ("tab", "layered", 6, 1, 128, 64, 70),
    "hbm_cascade9": ("tab", "cascade", 9, 1, 128, 64, 70),
    "no_ic": ("tab", "cascade", 4, 1, 128, 0, 70),
    "no_bc": ("tab", "cascade", 4, 1, 128, 70, 0),
    "analytic": ("analytic", "cascade", 4, 1, 128, 64, 70),
    "coef": ("coef", "cascade", 4, 1, 128, 64, 70),
    "sampled": ("sampled", "cascade", 4, 1, 128, 64, 70),      # the batches of QC_PHASE_SAMPLE from TT.dataset_arrays
}
SAMPLE_SEED = 0x5EED12345678
STEP_CFG = dict(alpha=0.5, every=1, lam_max=1e4, init=(1.0, 1.0))


def step_case_inputs(case):
    """(flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef | None) of one seeded case."""
    kind, ans, n, L, B_res, n_ic, n_bc = STEP_CASES[case]
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    flat, X_ic, X_bc, X_res = step_inputs(T.H, n, n_theta, B_res, n_ic, n_bc, salt=13)
    coef = CF.coef_star(X_res) if kind == "coef" else None
    if kind == "sampled":
        return (flat, *sampled_inputs(SAMPLE_SEED, 1, B_res, n_ic, n_bc), None)
    return flat, X_ic, X_bc, X_res, T.u_star(X_ic), T.u_star(X_bc), T.r_star(X_res), coef


def class_gradients(kind, flat, n, n_theta, theta_shape, ans, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef=None, H=T.H):
    """{"g_res", "g_ic", "g_bc": (NP,) float64 = w_c grad L_c, "parts": (L_r, L_bc, L_ic)}: one autograd pass per class
    (a pass over one class alone: the other two batches empty)."""
    haar = haar_for(n, 1)
    X = [torch.as_tensor(np.asarray(x)).double().reshape(-1, 3) for x in (X_ic, X_bc, X_res)]
    none, e = torch.zeros(0, 3, dtype=torch.float64), np.zeros(0, np.float32)

    def one(Xi, Xb, Xr, ui, ub, rr, cf):
        if kind == "analytic":
            return reference_loss(flat, H, n, n_theta, theta_shape, ans, haar, Xi, Xb, Xr)
        if kind == "coef":
            return CF.reference_loss_coef(flat, H, n, n_theta, theta_shape, ans, haar, Xi, Xb, Xr, ui, ub, rr, cf)
        return T.reference_loss_data(flat, H, n, n_theta, theta_shape, ans, haar, Xi, Xb, Xr, ui, ub, rr, coeffs=T.COEFFS, c_u=T.C_U)
    NP = len(flat)
    out = {"g_res": np.zeros(NP), "g_ic": np.zeros(NP), "g_bc": np.zeros(NP), "parts": np.zeros(3)}
    if len(X[2]):
        out["g_res"], p = one(none, none, X[2], e, e, r_res, coef)
        out["parts"][0] = p[0]
    if len(X[1]):
        out["g_bc"], p = one(none, X[1], none, e, u_bc, e, np.zeros((0, 7), np.float32))
        out["parts"][1] = p[1]
    if len(X[0]):
        out["g_ic"], p = one(X[0], none, none, u_ic, e, e, np.zeros((0, 7), np.float32))
        out["parts"][2] = p[2]
    return out


def step_job(case, inputs=None):
    kind, ans, n, L, B_res, n_ic, n_bc = STEP_CASES[case]
    P = int(pkg("circuits").params_per_layer(ans, n))
    flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef = step_case_inputs(case) if inputs is None else inputs
    return record(f"gradnorm_{case}",
                  [flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res, T.COEFFS + (T.C_U,)] + ([] if coef is None else [coef]),
                  lambda: class_gradients(kind, flat, n, L * P, (L, P), ans, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef))


def step_reference(case, inputs=None):
    """``class_gradients`` of one case (or of the given inputs under the case's shapes) through conftest.cached_oracle."""
    return step_job(case, inputs).get()


def expected_step(rec, n_ic, n_bc, cfg=STEP_CFG, unit=False, w=W3):
    """(flat (NP + 3,) float64, state dict, history (1, 7)) of the first call on a ``class_gradients`` record, in double.
    ``unit``: the control with both weights held at 1 (alpha = 0)."""
    r = Record(**dict(cfg, alpha=0.0 if unit else cfg["alpha"]), dtype=np.float64, w=w)
    parts = rec["parts"]
    G = np.zeros((3, len(rec["g_res"]) + 3))
    G[0, :-3], G[1, :-3], G[2, :-3] = rec["g_res"], rec["g_ic"], rec["g_bc"]
    G[0, -3], G[2, -2], G[1, -1] = parts[0], parts[1], parts[2]
    flat = r.step(G, n_ic, n_bc)
    return flat, r.state(), r.history()


def sampled_inputs(seed, step, B_res, n_ic, n_bc):
    """The batches the uniform device gather picks from TT.dataset_arrays for one step counter."""
    Xr, rr, Xi, ui, Xb, ub = TT.dataset_arrays()
    kr = T.dataset_indices(0, 0, B_res, len(Xr), seed, step)
    ki = T.dataset_indices(1, 0, n_ic, len(Xi), seed, step)
    kb = T.dataset_indices(2, 0, n_bc, len(Xb), seed, step)
    return Xi[ki], Xb[kb], Xr[kr], ui[ki], ub[kb], rr[kr]


# ---------------------------------------------------------------- training replay
TRAIN = dict(ansatz="cascade", n=4, H=16, B_res=128, n_ic=64, n_bc=64, steps=6)
TRAIN_CFG = dict(alpha=0.5, every=2, lam_max=1e4, init=(1.0, 1.0))


def base_args():
    return dict(TT.base_args(TRAIN["ansatz"], TRAIN["n"]), batch_size=TRAIN["B_res"], epochs=TRAIN["steps"] - 1,
                classic_network=[3, TRAIN["H"], 1])


def expected_batches(seed=None):
    seed = TT.trainer_seed() if seed is None else seed
    return [sampled_inputs(seed, step, TRAIN["B_res"], TRAIN["n_ic"], TRAIN["n_bc"]) for step in range(1, TRAIN["steps"] + 1)]


def initial_model():
    from oracle import solver as osol
    torch.manual_seed(1)
    return osol.OracleSolver(base_args(), device=torch.device("cpu"))


def gradnorm_run(model, batches, cfg=TRAIN_CFG, unit=False, coeffs=T.COEFFS, c_u=T.C_U, w=W3):
    """{"loss": (steps,) 2 L_r + 4 L_bc + 2 L_ic, "hist": (steps, 7) history rows, "g_abs": (steps, 3) mean |G_c|} of the
    float64 copy of ``model``: tabulated_training.replay with three backward passes per step and the combined gradient
    written in place of ``loss.backward()``; clip, Adam and plateau on it as every replay has them."""
    rec = Record(**dict(cfg, alpha=0.0 if unit else cfg["alpha"]), dtype=np.float32, w=w)
    hist, gabs = [], []

    def set_grads(parts, prm, b):
        l_r, l_bc, l_ic = parts
        sizes = [p.numel() for p in prm]
        flat = lambda L: np.concatenate([(torch.zeros_like(p) if q is None else q).reshape(-1).numpy()
                                         for p, q in zip(prm, torch.autograd.grad(L, prm, allow_unused=True))])
        G = np.zeros((3, sum(sizes) + 3))
        G[0, :-3], G[1, :-3], G[2, :-3] = flat(w[0] * l_r), flat(w[2] * l_ic), flat(w[1] * l_bc)
        G[0, -3], G[2, -2], G[1, -1] = l_r.item(), l_bc.item(), l_ic.item()
        gabs.append(np.abs(G[:, :-3]).mean(1))
        # the statistics and the combination in double; only the stored weights are rounded as the record rounds them
        r64 = Record(alpha=rec.alpha, every=rec.every, lam_max=rec.lam_max, dtype=np.float64, w=w)
        r64.lam_bc, r64.lam_ic, r64.n_steps = float(rec.lam_bc), float(rec.lam_ic), rec.n_steps
        r64.m_r, r64.a_bc, r64.a_ic = float(rec.m_r), float(rec.a_bc), float(rec.a_ic)
        comb = r64.step(G, len(b[3]), len(b[4]))
        rec.lam_bc, rec.lam_ic, rec.n_steps = np.float32(r64.lam_bc), np.float32(r64.lam_ic), r64.n_steps
        rec.m_r, rec.a_bc, rec.a_ic = np.float32(r64.m_r), np.float32(r64.a_bc), np.float32(r64.a_ic)
        row = r64.rows[-1]
        hist.append([float(rec.lam_bc), float(rec.lam_ic)] + [float(v) for v in row[2:]])
        off = 0
        for p, k in zip(prm, sizes):
            p.grad = torch.as_tensor(comb[off:off + k].reshape(p.shape).copy())
            off += k
    loss = TT.replay(model, batches, TT.data_residual(coeffs, c_u), lambda l_r, l_bc, l_ic: w[0] * l_r + w[1] * l_bc + w[2] * l_ic,
                     set_grads=set_grads)
    return {"loss": loss, "hist": np.array(hist)[:, :HIST_COLS].copy(), "g_abs": np.array(gabs)}


def training_job(batches=None, unit=False):
    batches = expected_batches() if batches is None else batches
    model = initial_model()
    c = TRAIN_CFG
    return record("gradnormtrain_cascade4_h16",
                  [flat_of(model), T.COEFFS + (T.C_U,), [c["alpha"], c["every"], c["lam_max"], *c["init"]]] + batch_inputs(*batches),
                  lambda: gradnorm_run(model, batches, unit=unit), variant="unit" if unit else "")


def training_reference(batches=None, unit=False):
    """``gradnorm_run`` of the training case through conftest.cached_oracle, keyed on the initial weights, the
    configuration and the batches."""
    return training_job(batches, unit).get()


def oracle_jobs():
    return [step_job(c) for c in STEP_CASES] + [training_job(unit=u) for u in (False, True)]
