"""Float64 replay of an Adam -> L-BFGS run of the fused step on ONE explicit batch: ADAM clip + Adam steps in float64 on the
flat vector, then EVALS evaluations of tests/lbfgs_reference.py (backtracking mode) driven by step_reference.reference_loss.
The GPU test (tests/test_gpu_lbfgs_train.py) runs FusedTrainer + LbfgsTrainer on the same weights and batch; the records
are committed under tests/golden/oracle/ (tests/golden/make_oracle_cache.py) and keyed on the inputs.

The generator asserts, on the replay: the Armijo slack |f - (f0 + c1 t gtd0)| >= 1e-3 max(1, |f0|) at every trial (fp32
cannot flip a decision), and at least one rejected trial (the salt is chosen so that both hold).

``usefulness_reference``: the same model trained for 200 Adam steps on a fixed batch, then 100 more Adam steps against 100
L-BFGS evaluations, in float64; the record stores both final losses and the generator asserts a factor >= 2."""
import numpy as np
import torch

import lbfgs_reference as LR
from conftest import cached_oracle, pkg
from step_reference import haar_for, reference_loss, step_inputs

H = 16
B_RES, N_IC, N_BC = 64, 21, 21
LR_ADAM, ADAM = 0.005, 5
#                     ansatz, n, L, L-BFGS evaluations, history, salt of step_inputs
CASES = {"cascade4": ("cascade", 4, 1, 14, 4, 29), "layered6": ("layered", 6, 1, 6, 4, 19)}
W = (2.0, 4.0, 2.0)


def case_shape(case):
    ans, n, L, evals, m, salt = CASES[case]
    P = int(pkg("circuits").params_per_layer(ans, n))
    return ans, n, L, L * P, (L, P), evals, m, salt


def case_inputs(case):
    ans, n, L, n_theta, _, _, _, salt = case_shape(case)
    return step_inputs(H, n, n_theta, B_RES, N_IC, N_BC, salt)


def loss_fn(case, X_ic, X_bc, X_res):
    """x (float64 flat vector) -> (f, grad, parts) of 2 L_r + 4 L_bc + 2 L_ic on the batch, float64."""
    ans, n, L, n_theta, shape, *_ = case_shape(case)
    haar = haar_for(n, 1)
    Xi, Xb, Xr = (torch.as_tensor(np.asarray(x)).double() for x in (X_ic, X_bc, X_res))

    def fg(x):
        g, parts = reference_loss(np.asarray(x, dtype=np.float64), H, n, n_theta, shape, ans, haar, Xi, Xb, Xr)
        return float(W[0] * parts[0] + W[1] * parts[1] + W[2] * parts[2]), np.asarray(g, dtype=np.float64), parts
    return fg


def adam_steps(fg, x, steps, lr=LR_ADAM, state=None):
    """clip_grad_norm_(1) + Adam (torch defaults) in float64; returns (x, losses, state)."""
    m, v, t = state if state is not None else (np.zeros_like(x), np.zeros_like(x), 0)
    losses = []
    for _ in range(steps):
        f, g, _ = fg(x)
        losses.append(f)
        g = g * min(1.0, 1.0 / (np.linalg.norm(g) + 1e-6))
        t += 1
        m = m + 0.1 * (g - m)
        v = 0.999 * v + 0.001 * g * g
        x = x - lr / (1.0 - 0.9 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - 0.999 ** t) + 1e-8)
    return x, losses, (m, v, t)


def lbfgs_evals(fg, x, evals, m, check=True):
    """-> (reference, per-evaluation losses, the point to evaluate next); ``check``: the conditions on the replay."""
    ref = LR.LbfgsReference(x.size, m, LR.ARMIJO)
    fs = []
    for _ in range(evals):
        f, g, _ = fg(x)
        fs.append(f)
        x = ref.step(x, f, g)
        if check:
            assert ref.slack is None or ref.slack >= 1e-3 * max(1.0, abs(ref.slack_f0)), (len(fs), ref.slack, ref.slack_f0)
    return ref, np.array(fs), x


def replay(case):
    ans, n, L, n_theta, shape, evals, m, salt = case_shape(case)
    flat, X_ic, X_bc, X_res = case_inputs(case)
    fg = loss_fn(case, X_ic, X_bc, X_res)
    x, adam_losses, _ = adam_steps(fg, flat.astype(np.float64), ADAM)
    ref, fs, _ = lbfgs_evals(fg, x, evals, m)
    assert ref.n_rejected >= 1, "the replay must reject at least one trial"
    return {"adam_loss": np.array(adam_losses), "x_adam": x, "loss": fs, "accepted": np.array([r[2] for r in ref.rows]),
            "t_led": np.array([r[1] for r in ref.rows]), "x_k": ref.x_k, "n_pairs": np.array([ref.n_pairs])}


def training_reference(case):
    flat, X_ic, X_bc, X_res = case_inputs(case)
    inputs = [flat] + [np.asarray(x, dtype=np.float32) for x in (X_ic, X_bc, X_res)] + \
        [np.array(CASES[case][3:], dtype=np.float32)]
    return cached_oracle(f"lbfgs_train_{case}", inputs, lambda: replay(case))


# ---- usefulness: Adam -> L-BFGS against Adam alone, the same 200 Adam steps in front of both
USE_CASE, USE_ADAM, USE_MORE, USE_M = "cascade4", 200, 100, 10


def usefulness_replay():
    flat, X_ic, X_bc, X_res = case_inputs(USE_CASE)
    fg = loss_fn(USE_CASE, X_ic, X_bc, X_res)
    x, _, st = adam_steps(fg, flat.astype(np.float64), USE_ADAM)
    xa, _, _ = adam_steps(fg, x, USE_MORE, state=st)
    ref, _, _ = lbfgs_evals(fg, x, USE_MORE, USE_M, check=False)
    f_adam, f_lbfgs = fg(xa)[0], float(ref.f0)
    assert f_adam >= 2.0 * f_lbfgs, (f_adam, f_lbfgs)
    return {"f_adam": np.array([f_adam]), "f_lbfgs": np.array([f_lbfgs]), "f_start": np.array([fg(x)[0]])}


def usefulness_reference():
    flat, X_ic, X_bc, X_res = case_inputs(USE_CASE)
    inputs = [flat] + [np.asarray(x, dtype=np.float32) for x in (X_ic, X_bc, X_res)] + \
        [np.array([USE_ADAM, USE_MORE, USE_M], dtype=np.float32)]
    return cached_oracle("lbfgs_usefulness", inputs, usefulness_replay)
