"""Float64 references of the seven-channel stages and step (the *_tt entry points of include/qcpinn_hip.h): the six
derivative channels {value, d/dt, d/dx, d/dy, d2/dx2, d2/dy2} and channel 6 = d2/dt2, operator rows of eight columns

    res_p = c_u u + c_3 u^3 + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy + d_tt u_tt),

rows (c_u, c_t, c_x, c_y, d_xx, d_yy, c_3, d_tt).

No seven-channel arithmetic is written here.  Every stage is the existing six-channel reference evaluated twice on shared
leaf tensors: as it stands, and with the roles of t and x exchanged, whose channel 4 ("xx") is then d2/dt2:

  * pre network: ``R.pre_jets`` with the t and x columns swapped in both W1 and X;
  * circuit and post network: the six-channel functions on the channels [0, 2, 1, 3, 6, 5] of their seven-channel input.

tests/test_tt_cpu.py checks the construction against an independent double ``autograd.grad`` of u(X).  Gradients come from
torch.autograd with respect to the shared leaves.  Negative-control tables: the d_tt column zeroed, the d_tt and d_xx
columns swapped, the table rolled by one row.
"""
import numpy as np
import torch

import coef_reference as CR
import mlp_reference as R
from step_reference import Step, as64, haar_for, mse_to, step_inputs

COLS = CR.COLS + ("d_tt",)
SWAP = [1, 0, 2]                  # columns of W1 and X with t and x exchanged
PERM = [0, 2, 1, 3, 6, 5]         # the six channels of that model among the seven: value, x, t, y, tt, yy
UT_ROW = np.array([0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float32)       # res = u_t: the second initial condition of a wave
CONTROLS = ("dtt_zero", "swap_tt_xx", "roll")


def pre_jets7(P, X):
    """X (B, 3) float64 -> angle jets (7, n, B)."""
    X = torch.as_tensor(X, dtype=R.F64)
    a = R.pre_jets(P, X, 6)
    a_s = R.pre_jets(dict(P, W1=P["W1"][:, SWAP]), X[:, SWAP], 6)
    return torch.cat([a, a_s[4:5]])


def qjets7(ajets, theta, ansatz, n, haar):
    """Angle jets (7, n, B) -> <Z> jets (7, n, B) of the circuit oracle."""
    from oracle import jets as oj
    q = oj.qjets_from_ajets(ajets[:6], theta, ansatz, n, haar, "angle")
    q_s = oj.qjets_from_ajets(ajets[PERM], theta, ansatz, n, haar, "angle")
    return torch.cat([q, q_s[4:5]])


def post_jets7(P, qjets):
    """<Z> jets (7, n, B) -> u jets (7, B)."""
    return torch.cat([R.post_jets(P, qjets[:6]), R.post_jets(P, qjets[PERM])[4:5]])


def u_jets7(P, X, theta_shape, ansatz, n, haar):
    return post_jets7(P, qjets7(pre_jets7(P, X), P["theta"].reshape(theta_shape), ansatz, n, haar))


def residual_coef_tt(ujets, coef):
    """(7, B) u jets and (B, 8) rows -> (B,) residual."""
    c = torch.as_tensor(np.asarray(coef), dtype=R.F64)
    return CR.residual_coef(ujets[:6], c[:, :7]) - c[:, 7] * ujets[6]


class StepTT(Step):
    """``Step`` whose residual points carry seven channels (``u_res`` (7, B)); the value points are ``Step``'s."""

    def __init__(self, flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res):
        X_res = torch.as_tensor(np.asarray(X_res), dtype=R.F64)
        super().__init__(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res[:0])
        if len(X_res):
            self.u_res = u_jets7(self.P, X_res, theta_shape, ansatz, n, haar)


def references_tt(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, tables):
    """``reference_loss_tt`` for several (B_res, 8) tables (a case and its negative controls) on ONE evaluation of the
    network and the circuit: a list of (grad (NP,), parts (3,))."""
    from step_reference import W3
    X_ic, X_bc = (torch.as_tensor(np.asarray(x), dtype=R.F64) for x in (X_ic, X_bc))
    s = StepTT(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res)
    out = []
    for coef in tables:
        l_r, l_bc, l_ic = s.losses(lambda u: ((residual_coef_tt(u, coef) - as64(r_res)) ** 2).mean(), mse_to(u_bc, u_ic))
        g = s.grad(W3[0] * l_r + W3[1] * l_bc + W3[2] * l_ic, retain_graph=True)
        out.append((g, np.array([l_r.item(), l_bc.item(), l_ic.item()])))
    return out


def reference_loss_tt(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef):
    """flat (NP,) weights, three (B, 3) point sets, their (B,) targets and the (B_res, 8) rows -> (grad (NP,), parts (3,))
    float64: the gradient of 2 L_r + 4 L_bc + 2 L_ic and (L_r, L_bc, L_ic)."""
    return references_tt(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, u_ic, u_bc, r_res, [coef])[0]


def coef_tt_star(X):
    """(B, 8) float32 rows of the points X: ``coef_reference.coef_star`` (no column constant, c_u and c_3 of both signs) with
    a d_tt column of both signs, every fifth row the pure u_t row."""
    X64 = np.asarray(X, dtype=np.float64)
    d_tt = (-1.0 + 1.6 * np.sin(2.0 * X64[:, 0] + 3.0 * X64[:, 2] + 0.3)).astype(np.float32)
    tab = np.concatenate([CR.coef_star(X), d_tt[:, None]], axis=1)
    tab[4::5] = UT_ROW
    return tab


def variant_table(variant, coef):
    """The table a negative control's reference applies."""
    coef = np.array(coef, dtype=np.float32)
    if variant == "dtt_zero":
        coef[:, 7] = 0.0
    elif variant == "swap_tt_xx":
        coef[:, [4, 7]] = coef[:, [7, 4]]
    elif variant == "roll":
        coef = np.roll(coef, 1, axis=0)
    elif variant:
        raise ValueError(variant)
    return coef


def case_inputs(ansatz, n, L, H, B_res, n_ic, n_bc, salt=31):
    """Seeded inputs of one step case: (n_theta, theta_shape, haar, flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef8)."""
    from conftest import pkg
    Pl = int(pkg("circuits").params_per_layer(ansatz, n))
    n_theta, theta_shape = L * Pl, (L, Pl)
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt)
    g = np.random.default_rng(salt + n + B_res)
    u_ic, u_bc, r_res = (g.standard_normal(m).astype(np.float32) * 0.5 for m in (n_ic, n_bc, B_res))
    haar = haar_for(n, 1)
    return n_theta, theta_shape, haar, flat, X_ic.numpy(), X_bc.numpy(), X_res.numpy(), u_ic, u_bc, r_res, coef_tt_star(X_res.numpy())


def autograd_jets7(P, X, theta_shape, ansatz, n, haar):
    """The seven channels (7, B) by differentiating the composed float64 model u(X) twice with respect to X: independent of
    every jet formula (value path only: ``R.pre_jets`` / ``R.post_jets`` with one channel, the statevector oracle)."""
    from oracle import statevector as sv
    X = torch.as_tensor(np.asarray(X), dtype=R.F64).clone().requires_grad_(True)
    a = R.pre_jets(P, X, 1)
    q = sv.circuit_expvals(a[0].T, P["theta"].reshape(theta_shape), ansatz, n, haar, "angle")[None]
    u = R.post_jets(P, q)[0]
    (g1,) = torch.autograd.grad(u.sum(), X, create_graph=True)
    second = [torch.autograd.grad(g1[:, k].sum(), X, retain_graph=True)[0][:, k] for k in range(3)]
    return torch.stack([u, g1[:, 0], g1[:, 1], g1[:, 2], second[1], second[2], second[0]]).detach()


# ---------------------------------------------------------------- the standing wave and its float64 replay
WAVE_C = 0.5


def wave_u(X, c=WAVE_C):
    """u = cos(sqrt(2) pi c t) sin(pi x) sin(pi y): u_tt = c^2 (u_xx + u_yy), zero on the faces of the unit square, u_t = 0
    at t = 0."""
    X = np.asarray(X, dtype=np.float64)
    return (np.cos(np.sqrt(2.0) * np.pi * c * X[:, 0]) * np.sin(np.pi * X[:, 1]) * np.sin(np.pi * X[:, 2])).astype(np.float32)


def wave_dataset(n_int=192, n_vel=64, n_ic=96, n_bc=96, c=WAVE_C, seed=4):
    """Seeded float32 arrays (X_res, r, X_ic, u_ic, X_bc, u_bc, coef8) of the standing-wave problem: interior rows
    (0, 0, 0, 0, c^2, c^2, 0, -1) with target 0 followed by rows (0, 1, 0, 0, 0, 0, 0, 0) at t = 0 with target 0 (the
    condition u_t(0, .) = 0), u(0, .) on the IC points and 0 on the four faces."""
    g = np.random.default_rng(seed)
    Xi = g.uniform(0, 1, (n_int, 3)).astype(np.float32)
    Xv = g.uniform(0, 1, (n_vel, 3)).astype(np.float32)
    Xv[:, 0] = 0.0
    X0 = g.uniform(0, 1, (n_ic, 3)).astype(np.float32)
    X0[:, 0] = 0.0
    Xb = g.uniform(0, 1, (n_bc, 3)).astype(np.float32)
    face = np.arange(n_bc) % 4
    Xb[face == 0, 1], Xb[face == 1, 1], Xb[face == 2, 2], Xb[face == 3, 2] = 0.0, 1.0, 0.0, 1.0
    rows = np.concatenate([np.tile(np.array([0, 0, 0, 0, c * c, c * c, 0, -1], np.float32), (n_int, 1)), np.tile(UT_ROW, (n_vel, 1))])
    X_res = np.concatenate([Xi, Xv])
    return X_res, np.zeros(len(X_res), np.float32), X0, wave_u(X0, c), Xb, np.zeros(n_bc, np.float32), rows


def replay_tt(model, batches):
    """(loss history (steps,), final flat weights) of the float64 copy of the OracleSolver ``model`` trained on ``batches``
    = (X_ic, X_bc, X_res, u_ic, u_bc, r_res, coef8) per step as tests/tabulated_training.py::replay trains: the reference's
    Adam / clip_grad_norm_(1) / ReduceLROnPlateau(0.9, 1000) on 2 L_r + 4 L_bc + 2 L_ic, every derivative of the residual,
    u_tt included, by autograd."""
    from oracle import statevector as sv
    from step_reference import flat_of
    model = model.double()
    ql = model.quantum_layer

    def net(x):
        q = sv.circuit_expvals(model.preprocessor(x), ql.params, ql.q_ansatz, ql.num_qubits, ql._haar, "angle")
        return model.postprocessor(q.T.reshape(-1, ql.num_qubits))

    mse = torch.nn.MSELoss()
    prm = list(model.parameters())
    opt = torch.optim.Adam(prm, lr=model.args["lr"])
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=1000)
    g = lambda out, wrt: torch.autograd.grad(out, wrt, torch.ones_like(out), create_graph=True)[0]
    hist = []
    for b in batches:
        opt.zero_grad()
        t, x, y = [as64(b[2])[:, k:k + 1].requires_grad_(True) for k in range(3)]
        u = net(torch.cat((t, x, y), 1))
        u_t, u_x, u_y = g(u, t), g(u, x), g(u, y)
        c = [as64(b[6])[:, k:k + 1] for k in range(8)]
        res = c[0] * u + c[6] * u ** 3 + c[1] * u_t + c[2] * u_x + c[3] * u_y - (c[4] * g(u_x, x) + c[5] * g(u_y, y) + c[7] * g(u_t, t))
        loss = 2.0 * mse(res, as64(b[5])[:, None]) + 4.0 * mse(net(as64(b[1])), as64(b[4])[:, None]) + \
            2.0 * mse(net(as64(b[0])), as64(b[3])[:, None])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(prm, max_norm=1)
        opt.step()
        sch.step(loss)
        hist.append(loss.item())
    return np.array(hist), flat_of(model)
