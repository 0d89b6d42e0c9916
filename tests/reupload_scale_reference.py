"""Float64 restatement of the data re-uploading circuit WITH trainable input scalings (args["reupload_scale"]: RX(s a_w)
in front of every ansatz layer after the first, the w.x of Perez-Salinas et al. 2020), built like
tests/reupload_reference.py from the oracle's ``Simulator`` and ``ANSATZ`` and on top of that module.

The whole circuit behind the first embedding is ONE builder ``(sim, theta, x)`` of the kind reupload_reference.expvals
takes (``takes_angles``): theta is the kernels' flat vector, the ansatz slots (L, P) first and the scalings behind them
("wire": slot L P + (l - 1) n + w, "layer": slot L P + (l - 1)).  So ``expvals`` / ``qjets`` are reupload_reference's own,
called with a one-row parameter matrix and reupload=False, and differentiate with respect to the scalings as well.

The step reference composes tests/mlp_reference.py with these functions as reupload_reference.step_reference does, with a
``dtype`` argument on top: complex64 runs the same gates on a single-precision state (the fp32 - fp64 gap of a case).
"""
import numpy as np
import torch

import mlp_reference as R
import reupload_reference as RR
from conftest import cached_oracle, pkg
from oracle.statevector import ANSATZ
from step_reference import PDE, W3, haar_for, step_inputs, unpack

RDT = torch.float64


def n_scales(n, L, mode):
    return (L - 1) * (n if mode == "wire" else 1)


def scale_slot(n, L, P, mode, layer, w):
    return L * P + (layer - 1) * (n if mode == "wire" else 1) + (w if mode == "wire" else 0)


def whole_circuit(ansatz, n, L, mode):
    """The builder of a ``build_program(ansatz, n, L, ., reupload=True, reupload_scale=mode)`` circuit."""
    P = int(pkg("circuits").params_per_layer(ansatz, n))

    def build(sim, theta, x):
        for layer in range(L):
            if layer > 0:
                for w in range(n):
                    sim.RX(theta[scale_slot(n, L, P, mode, layer, w)] * x[:, w], w)
            ANSATZ[ansatz](sim, theta[layer * P:(layer + 1) * P])
    build.takes_angles = True
    return build


def expvals(x, theta, builder, n, haar=None, dtype=torch.complex128):
    """x (B, n), theta flat -> (n, B) <Z_w>; ``builder``: ``whole_circuit(...)`` or a hand-written ``(sim, theta, x)``."""
    return RR.expvals(x, theta.reshape(1, -1), builder, n, haar, False, dtype)


def qjets(ajets, theta, builder, n, haar=None, dtype=torch.complex128):
    return RR.qjets(ajets, theta.reshape(1, -1), builder, n, haar, False, dtype)


# ---------------------------------------------------------------- circuit cases
def scalings(ns, seed):
    """1 + 0.4 randn from their own seed."""
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 0.4 * torch.randn(ns, generator=g, dtype=torch.float64)


def vjp_inputs(ans, n, L, B, mode="wire"):
    """theta flat float32 (ansatz slots as reupload_reference draws them, then the scalings), x, cot."""
    params, x, cot = RR.vjp_inputs(ans, n, L, B)
    s = scalings(n_scales(n, L, mode), 11 + n + B)
    return torch.cat([params.reshape(-1), s.float()]), x, cot


def jets_inputs(ans, n, L, B, mode="wire"):
    params, ajets, w = RR.jets_inputs(ans, n, L, B)
    s = scalings(n_scales(n, L, mode), 23 + n + B)
    return torch.cat([params.reshape(-1), s.float()]), ajets, w


def ones_control(theta, ns):
    t = theta.clone()
    t[theta.numel() - ns:] = 1.0
    return t


def vjp_compute(builder, n, haar, theta, x, cot, dtype=torch.complex128):
    xo, to = x.double().requires_grad_(True), theta.double().requires_grad_(True)
    q = expvals(xo, to, builder, n, haar, dtype)
    (q * cot.double()).sum().backward()
    return {"q": q.detach().numpy(), "dx": xo.grad.numpy(), "dp": to.grad.numpy()}


def jets_compute(builder, n, haar, theta, ajets, w, dtype=torch.complex128):
    ao, to = ajets.double().requires_grad_(True), theta.double().requires_grad_(True)
    qo = qjets(ao, to, builder, n, haar, dtype)
    (qo * w.double()).sum().backward()
    return {"q": qo.detach().numpy(), "da": ao.grad.numpy(), "dp": to.grad.numpy()}


def vjp_reference(ans, n, L, seed, B, mode, theta, x, cot, control=False):
    """``control``: the same theta with every scaling set to 1 (the reupload=True circuit)."""
    ns = n_scales(n, L, mode)
    th = ones_control(theta, ns) if control else theta
    return cached_oracle(f"reupsvjp_{ans}_n{n}_L{L}_s{seed}_B{B}_{mode}" + ("_ones" if control else ""),
                         (th.numpy(), x.numpy(), cot.numpy()),
                         lambda: vjp_compute(whole_circuit(ans, n, L, mode), n, haar_for(n, seed), th, x, cot))


def jets_reference(ans, n, L, seed, B, mode, theta, ajets, w, control=False):
    ns = n_scales(n, L, mode)
    th = ones_control(theta, ns) if control else theta
    return cached_oracle(f"reupsjets_{ans}_n{n}_L{L}_s{seed}_B{B}_{mode}" + ("_ones" if control else ""),
                         (th.numpy(), ajets.numpy(), w.numpy()),
                         lambda: jets_compute(whole_circuit(ans, n, L, mode), n, haar_for(n, seed), th, ajets, w))


# ---------------------------------------------------------------- the step
def step_reference(flat, H, n, n_theta, builder, haar, X_ic, X_bc, X_res, Bf=None, dtype=torch.complex128):
    """(grad (NP,), parts (3,)) float64 as reupload_reference.step_reference, theta flat (scalings in its tail)."""
    X_ic, X_bc, X_res = (torch.as_tensor(np.asarray(x), dtype=R.F64) for x in (X_ic, X_bc, X_res))
    if Bf is None:
        P = unpack(flat, H, n, n_theta)
        pre = lambda X, nch: R.pre_jets(P, X, nch)
    else:
        import fourier_reference as FR
        Bf = torch.as_tensor(np.asarray(Bf), dtype=R.F64)
        P = FR.unpack(flat, H, n, n_theta, Bf.shape[1])
        pre = lambda X, nch: FR.pre_jets_ff(P, Bf, X, nch)
    leaves = [P[k] for k in R.NAMES]
    theta = P["theta"].reshape(-1)
    zero = torch.zeros((), dtype=R.F64)
    l_r = zero
    if len(X_res):
        u = R.post_jets(P, qjets(pre(X_res, 6), theta, builder, n, haar, dtype))
        l_r = (R.point_errors(u, X_res, PDE, 6) ** 2).mean()
    vals = []
    for Xv in (X_bc, X_ic):
        if not len(Xv):
            vals.append(zero)
            continue
        uv = R.post_jets(P, expvals(pre(Xv, 1)[0].T, theta, builder, n, haar, dtype)[None])
        vals.append(((uv[0] - R.analytic_u(Xv)) ** 2).mean())
    l_bc, l_ic = vals
    loss = W3[0] * l_r + W3[1] * l_bc + W3[2] * l_ic
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    g = np.concatenate([(torch.zeros_like(p) if gr is None else gr).detach().numpy().reshape(-1) for p, gr in zip(leaves, grads)])
    return g, np.array([l_r.item(), l_bc.item(), l_ic.item()])


def step_case_inputs(ans, n, L, H, B_res, n_ic, n_bc, m=None, scale=2.0):
    """(Bf | None, flat, X_ic, X_bc, X_res) of a "wire" case: the inputs of the reupload=True case with n_theta grown by the
    scalings, which are then drawn as 1 + 0.4 randn from their own seed."""
    ns = n_scales(n, L, "wire")
    n_theta = L * int(pkg("circuits").params_per_layer(ans, n)) + ns
    if m is None:
        Bf = None
        flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=1)
    else:
        import fourier_reference as FR
        Bf, flat, X_ic, X_bc, X_res = FR.step_inputs(H, n, n_theta, m, scale, B_res, n_ic, n_bc, salt=3)
    flat = np.array(flat, dtype=np.float32)
    flat[-ns:] = scalings(ns, 2000 + n + L).numpy()
    return Bf, flat, X_ic, X_bc, X_res


def step_record(ans, n, L, seed, flat, X_ic, X_bc, X_res, H, variant="", Bf=None):
    """{"grad", "parts"} of a "wire" case; ``variant``: "" | "ones" (every scaling 1) | "c64" (complex64 state: the
    fp32 - fp64 gap of the restatement)."""
    ns = n_scales(n, L, "wire")
    n_theta = L * int(pkg("circuits").params_per_layer(ans, n)) + ns
    f = np.array(flat, dtype=np.float32)
    if variant == "ones":
        f[-ns:] = 1.0

    def compute():
        g, parts = step_reference(f, H, n, n_theta, whole_circuit(ans, n, L, "wire"), haar_for(n, seed), X_ic, X_bc, X_res, Bf=Bf,
                                  dtype=torch.complex64 if variant == "c64" else torch.complex128)
        return {"grad": g, "parts": parts}
    key = (f"reupsstep_{ans}_n{n}_L{L}_s{seed}_H{H}_r{len(X_res)}_i{len(X_ic)}_b{len(X_bc)}" + (f"_m{np.shape(Bf)[1]}" if Bf is not None else "")
           + (f"_{variant}" if variant else ""))
    arrays = [f, X_ic, X_bc, X_res] + ([Bf] if Bf is not None else [])
    return cached_oracle(key, [np.asarray(a, dtype=np.float32) for a in arrays], compute)


def write_records():
    """Every record the GPU tests of this feature read (tests/golden/oracle/reups*.npz), through the tests' own case lists:
    ``QC_WRITE_ORACLE_CACHE=1 python tests/reupload_scale_reference.py``."""
    import test_gpu_reupload_scale_circuit as TC
    import test_gpu_reupload_scale_step as TS
    for ans, n, L, seed, B, mode in TC.VJP_CASES:
        for c in (False, True):
            vjp_reference(ans, n, L, seed, B, mode, *vjp_inputs(ans, n, L, B, mode), control=c)
    for ans, n, L, seed, B, mode in TC.JETS_CASES:
        for c in (False, True):
            jets_reference(ans, n, L, seed, B, mode, *jets_inputs(ans, n, L, B, mode), control=c)
    for case, (ans, n, L, B_res, n_ic, n_bc) in TS.CASES.items():
        _, flat, X_ic, X_bc, X_res = step_case_inputs(ans, n, L, TS.H, B_res, n_ic, n_bc)
        for v in ("", "ones", "c64"):
            step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, TS.H, variant=v)
    ans, n, L, m, B_res, n_ic, n_bc = TS.FOURIER_CASE
    Bf, flat, X_ic, X_bc, X_res = step_case_inputs(ans, n, L, TS.H, B_res, n_ic, n_bc, m=m)
    for v in ("", "ones"):
        step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, TS.H, variant=v, Bf=Bf)


if __name__ == "__main__":
    write_records()
