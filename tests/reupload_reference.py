"""Float64 restatement of the data re-uploading circuit (Perez-Salinas et al. 2020; the reference's own experiments embed
in front of every entangling layer: hybrid_testing/hqpinn_pennylane.py:46-59), built FROM the oracle: its ``Simulator``
and its ``ANSATZ`` builders are imported and used as they are.

``expvals`` applies the RX embedding before layer 0 and, with ``reupload``, before every later layer; ``qjets`` forms the
six channels along input curves exactly as oracle/jets.py does.  ``dtype=torch.complex64`` runs the same gates on a
single-precision state (the gate matrices rounded to it), to measure the fp32 - fp64 gap of a case.

The step reference composes tests/mlp_reference.py with these circuit functions as tests/step_reference.py composes it
with the plain oracle: the gradient of 2 L_r + 4 L_bc + 2 L_ic and (L_r, L_bc, L_ic) on the analytic problem.
"""
import numpy as np
import torch

import mlp_reference as R
from conftest import cached_oracle, pkg
from oracle.statevector import ANSATZ, Simulator
from step_reference import PDE, W3, haar_for, unpack

RDT = torch.float64


class _Sim(Simulator):
    """The oracle's simulator on a state of another complex dtype: every gate matrix is cast to the state's dtype."""

    def __init__(self, n, batch, dtype):
        super().__init__(n, batch)
        self.state = self.state.to(dtype)

    def apply1(self, mat, w):
        super().apply1(mat.to(self.state.dtype), w)

    def apply2(self, mat4, a, b):
        super().apply2(mat4.to(self.state.dtype), a, b)


def expvals(x, params, ansatz, n, haar=None, reupload=True, dtype=torch.complex128):
    """x (B, n) angles, params (L, P) -> (n, B) <Z_w>, differentiable.  ``ansatz``: a name of the oracle's table, or a
    builder ``(sim, p)`` of the same kind (the closed-form checks use one without an entangler); a builder with the
    attribute ``takes_angles`` is called as ``(sim, p, x)`` and applies RX(x[:, w]) wherever it likes."""
    x, params = x.to(RDT), params.to(RDT)
    builder = ANSATZ[ansatz] if isinstance(ansatz, str) else ansatz
    if getattr(builder, "takes_angles", False):      # a builder that places its own re-uploads: (sim, p, x)
        own = builder
        builder = lambda s, p: own(s, p, x)
    sim = _Sim(n, x.shape[0], dtype)
    for layer in range(params.shape[0]):
        if layer == 0 or reupload:
            for w in range(n):
                sim.RX(x[:, w], w)
        builder(sim, params[layer])
    if haar is not None:
        sim.apply2(haar[0], 0, 1)
        sim.apply2(haar[1], 2, 3)
    sim.H(n - 1)
    return torch.stack([sim.expval_z(w) for w in range(n)]).to(RDT)


def qjets(ajets, params, ansatz, n, haar=None, reupload=True, dtype=torch.complex128):
    """ajets (6, n, B) -> (6, n, B): channels 0 value, 1 d/dt, 2 d/dx, 3 d/dy, 4 d2/dx2, 5 d2/dy2 (oracle/jets.py)."""
    B = ajets.shape[2]
    a0 = ajets[0].T
    chans = {0: expvals(a0, params, ansatz, n, haar, reupload, dtype)}
    for k in (1, 2, 3):
        eps = torch.zeros(B, dtype=RDT, requires_grad=True)
        curve = a0 + eps[:, None] * ajets[k].T
        if k >= 2:
            curve = curve + 0.5 * eps[:, None] ** 2 * ajets[k + 2].T
        q = expvals(curve, params, ansatz, n, haar, reupload, dtype)
        q1 = torch.stack([torch.autograd.grad(q[i].sum(), eps, create_graph=True)[0] for i in range(n)])
        chans[k] = q1
        if k >= 2:
            chans[k + 2] = torch.stack([torch.autograd.grad(q1[i].sum(), eps, create_graph=True)[0] for i in range(n)])
    return torch.stack([chans[c] for c in range(6)])


# ---------------------------------------------------------------- circuit cases (inputs as tests/test_gpu_circuit.py draws them)
def vjp_inputs(ans, n, L, B, salt=5):
    g = torch.Generator().manual_seed(salt + n + B)
    P = pkg("circuits").params_per_layer(ans, n)
    params = torch.randn(L, P, generator=g) * 0.8
    x = torch.randn(B, n, generator=g) * 1.1
    cot = torch.randn(n, B, generator=g)
    return params, x, cot


def jets_inputs(ans, n, L, B, salt=77):
    g = torch.Generator().manual_seed(salt + n + B)
    P = pkg("circuits").params_per_layer(ans, n)
    params = torch.randn(L, P, generator=g) * 0.8
    ajets = torch.randn(6, n, B, generator=g) * 0.9
    w = torch.randn(6, n, B, generator=g)
    return params, ajets, w


def vjp_reference(ans, n, L, seed, B, params, x, cot, reupload=True, dtype=torch.complex128):
    haar = haar_for(n, seed)

    def compute():
        xo, po = x.double().requires_grad_(True), params.double().requires_grad_(True)
        q = expvals(xo, po, ans, n, haar, reupload, dtype)
        (q * cot.double()).sum().backward()
        return {"q": q.detach().numpy(), "dx": xo.grad.numpy(), "dp": po.grad.numpy()}
    if dtype != torch.complex128:
        return compute()
    return cached_oracle(f"reupvjp_{ans}_n{n}_L{L}_s{seed}_B{B}_{'re' if reupload else 'plain'}",
                         (params.numpy(), x.numpy(), cot.numpy()), compute)


def jets_reference(ans, n, L, seed, B, params, ajets, w, reupload=True, dtype=torch.complex128):
    haar = haar_for(n, seed)

    def compute():
        ao, po = ajets.double().requires_grad_(True), params.double().requires_grad_(True)
        qo = qjets(ao, po, ans, n, haar, reupload, dtype)
        (qo * w.double()).sum().backward()
        return {"q": qo.detach().numpy(), "da": ao.grad.numpy(), "dp": po.grad.numpy()}
    if dtype != torch.complex128:
        return compute()
    return cached_oracle(f"reupjets_{ans}_n{n}_L{L}_s{seed}_B{B}_{'re' if reupload else 'plain'}",
                         (params.numpy(), ajets.numpy(), w.numpy()), compute)


# ---------------------------------------------------------------- the step
def step_reference(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, reupload=True, Bf=None):
    """(grad (NP,), parts (3,)) float64, as step_reference.reference_loss, on the re-uploaded circuit.  ``Bf`` (3, m): the
    Fourier-feature map of tests/fourier_reference.py in front of the pre network (W1 is then (H, 2m))."""
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
    theta = P["theta"].reshape(theta_shape)
    zero = torch.zeros((), dtype=R.F64)
    l_r = zero
    if len(X_res):
        a = pre(X_res, 6)
        u = R.post_jets(P, qjets(a, theta, ansatz, n, haar, reupload))
        l_r = (R.point_errors(u, X_res, PDE, 6) ** 2).mean()
    vals = []
    for Xv in (X_bc, X_ic):
        if not len(Xv):
            vals.append(zero)
            continue
        av = pre(Xv, 1)
        uv = R.post_jets(P, expvals(av[0].T, theta, ansatz, n, haar, reupload)[None])
        vals.append(((uv[0] - R.analytic_u(Xv)) ** 2).mean())
    l_bc, l_ic = vals
    loss = W3[0] * l_r + W3[1] * l_bc + W3[2] * l_ic
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    g = np.concatenate([(torch.zeros_like(p) if gr is None else gr).detach().numpy().reshape(-1) for p, gr in zip(leaves, grads)])
    return g, np.array([l_r.item(), l_bc.item(), l_ic.item()])


def step_record(ansatz, n, L, seed, flat, X_ic, X_bc, X_res, H, variant="", Bf=None):
    """{"grad", "parts"} of one case; ``variant``: "" | "plain" (the circuit without re-uploading) | "drop_res"."""
    Pn = int(pkg("circuits").params_per_layer(ansatz, n))
    Xr = X_res[:-1] if variant == "drop_res" else X_res

    def compute():
        g, parts = step_reference(flat, H, n, L * Pn, (L, Pn), ansatz, haar_for(n, seed),
                                  X_ic, X_bc, Xr, reupload=variant != "plain", Bf=Bf)
        return {"grad": g, "parts": parts}
    key = (f"reupstep_{ansatz}_n{n}_L{L}_s{seed}_H{H}_r{len(X_res)}_i{len(X_ic)}_b{len(X_bc)}" + (f"_m{np.shape(Bf)[1]}" if Bf is not None else "")
           + (f"_{variant}" if variant else ""))
    arrays = [flat, X_ic, X_bc, X_res] + ([Bf] if Bf is not None else [])
    return cached_oracle(key, [np.asarray(a, dtype=np.float32) for a in arrays], compute)


def write_records():
    """Every record the GPU tests of this feature read (tests/golden/oracle/reup*.npz), through the tests' own case
    lists: ``QC_WRITE_ORACLE_CACHE=1 python tests/reupload_reference.py``."""
    import fourier_reference as FR
    import test_gpu_reupload_circuit as TC
    import test_gpu_reupload_step as TS
    from step_reference import step_inputs
    for ans, n, L, seed, B in TC.VJP_CASES:
        for re in (True, False):
            vjp_reference(ans, n, L, seed, B, *vjp_inputs(ans, n, L, B), reupload=re)
    for ans, n, L, seed, B in TC.JETS_CASES:
        for re in (True, False):
            jets_reference(ans, n, L, seed, B, *jets_inputs(ans, n, L, B), reupload=re)
    for case, (ans, n, L, B_res, n_ic, n_bc) in TS.CASES.items():
        n_theta = L * int(pkg("circuits").params_per_layer(ans, n))
        flat, X_ic, X_bc, X_res = step_inputs(TS.H, n, n_theta, B_res, n_ic, n_bc, salt=1)
        for v in ("",) + tuple(TS.CONTROLS.get(case, ())):
            step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, TS.H, variant=v)
    ans, n, L, m, scale, B_res, n_ic, n_bc = "cascade", 4, 2, 8, 2.0, 33, 10, 11
    n_theta = L * int(pkg("circuits").params_per_layer(ans, n))
    Bf, flat, X_ic, X_bc, X_res = FR.step_inputs(TS.H, n, n_theta, m, scale, B_res, n_ic, n_bc, salt=3)
    for v in ("", "plain"):
        step_record(ans, n, L, 1, flat, X_ic, X_bc, X_res, TS.H, variant=v, Bf=Bf)


if __name__ == "__main__":
    write_records()
