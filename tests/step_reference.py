"""Float64 reference of the fused training step's [grad | L_r, L_bc, L_ic] vector (qc_fused_pinn_residual_step,
QC_PHASE_GRADS): the classical stages of tests/mlp_reference.py composed with the circuit oracle (oracle/jets.py for the
residual points' six channels, oracle/statevector.py for the value points), differentiated by torch.autograd.

The loss is the trainer's 2 L_r + 4 L_bc + 2 L_ic (trainer/diffusion_train.py:47) on the convection-diffusion operator
with D = 0.01, v = (1, 1) and unit sigmas, the problem the library's step solves by default.  An empty point set
contributes 0 to the loss and to its part, as the step reports it.

``Step`` is that composition, written once.  Every variant of the step (tabulated, coefficient table, inverse, balanced,
causal, gradient-norm, system: tests/*_reference.py) builds a ``Step`` and supplies only its residual, its targets and
how it reduces the three parts.

``Record`` is a committed record under tests/golden/oracle/ as the triple (key, inputs, compute) of
conftest.cached_oracle; ``record`` builds one, and every reference module lists its records in ``oracle_jobs()``
(tests/golden/make_oracle_cache.py writes them, tests/test_oracle_records_cpu.py checks them), so no GPU run pays for the
oracle.  ``step_inputs`` draws the weights and points of the seeded cases from a seeded CPU generator, so the inputs,
and with them the records' digests, do not depend on a device.
"""
from typing import Callable, NamedTuple

import numpy as np
import torch

import mlp_reference as R
from conftest import cached_oracle, pkg

PDE = dict(c_t=1.0, c_x=1.0, c_y=1.0, d_xx=0.01, d_yy=0.01, D=0.01, vx=1.0, vy=1.0, problem=0)
W3 = (2.0, 4.0, 2.0)                   # residual, BC, IC
as64 = lambda a: torch.as_tensor(np.asarray(a), dtype=R.F64)


def layout(H, n, n_theta, K=None):
    """name -> (offset, shape) of the flat vector and its length: mlp_reference.layout, or with K last-layer rows
    W1 b1 W2 b2 | W3 b3 W4[K][H] b4[K] | theta (the same vector at K = 1)."""
    if K is None:
        return R.layout(H, n, n_theta)
    out, off = {}, 0
    for name, shape in zip(R.NAMES, ((H, 3), (H,), (n, H), (n,), (H, n), (H,), (K, H), (K,), (n_theta,))):
        out[name] = (off, shape)
        off += int(np.prod(shape))
    return out, off


def unpack(flat, H, n, n_theta, K=None):
    """flat (NP,) -> dict of float64 leaf tensors that require grad."""
    lay, NP = layout(H, n, n_theta, K)
    flat = np.asarray(flat, dtype=np.float64)
    assert flat.shape == (NP,)
    return {k: torch.tensor(flat[o:o + int(np.prod(s))].reshape(s), dtype=R.F64, requires_grad=True) for k, (o, s) in lay.items()}


class Step:
    """The composition every variant of the step starts from, written once: unpack -> pre_jets -> circuit oracle ->
    post_jets on the residual points (six channels, oracle/jets.py) and on the BC and IC points (values,
    oracle/statevector.py).

    ``u_res``: the u jets (6, B), or (K, 6, B) with ``K`` last-layer rows; ``u_bc`` / ``u_ic``: the values (B,) or (K, B).
    Each is None for an empty point set, which then contributes an exact zero and no graph (``loss``).  ``leaves``: the
    parameters in R.NAMES order followed by ``extra`` (the inverse step's ``p``); ``grad`` differentiates a scalar with
    respect to them into one flat float64 vector, an unused leaf giving zeros."""

    def __init__(self, flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, drop_unit=False, encoding="angle",
                 K=None, extra=()):
        from oracle import jets as oj
        from oracle import statevector as sv
        self.P = P = unpack(flat, H, n, n_theta, K)
        self.leaves = [P[k] for k in R.NAMES] + list(extra)
        theta = P["theta"].reshape(theta_shape)
        rows = {} if K is None else dict(w4=P["W4"], b4=P["b4"])
        self.u_res = None
        if len(X_res):
            a = R.pre_jets(P, X_res, 6, drop_unit)
            q = oj.qjets_from_ajets(a, theta, ansatz, n, haar, encoding)
            self.u_res = R.post_jets(P, q, drop_unit, **rows)
        vals = []
        for Xv in (X_bc, X_ic):
            if not len(Xv):
                vals.append(None)
                continue
            av = R.pre_jets(P, Xv, 1, drop_unit)
            qv = sv.circuit_expvals(av[0].T, theta, ansatz, n, haar, encoding)[None]
            uv = R.post_jets(P, qv, drop_unit, **rows)
            vals.append(uv[0] if K is None else uv[:, 0])
        self.u_bc, self.u_ic = vals

    def losses(self, residual, value):
        """(L_r, L_bc, L_ic) tensors: ``residual(u_res)`` and ``value(u, which)``, which = "bc" / "ic", each a scalar;
        an exact zero for an empty point set."""
        zero = torch.zeros((), dtype=R.F64)
        return (zero if self.u_res is None else residual(self.u_res),
                zero if self.u_bc is None else value(self.u_bc, "bc"),
                zero if self.u_ic is None else value(self.u_ic, "ic"))

    def grad(self, loss, retain_graph=False):
        # the leaves are in R.NAMES order, which is the order of the blocks in the flat layout (layout, any K), so their
        # concatenation IS the flat gradient; extra leaves follow it
        grads = torch.autograd.grad(loss, self.leaves, allow_unused=True, retain_graph=retain_graph)
        return np.concatenate([(torch.zeros_like(p) if g is None else g).detach().numpy().reshape(-1)
                               for p, g in zip(self.leaves, grads)])

    def weighted(self, parts, w=W3):
        """(gradient of w_res L_r + w_bc L_bc + w_ic L_ic, (L_r, L_bc, L_ic)) float64: the reduction of most variants."""
        l_r, l_bc, l_ic = parts
        loss = w[0] * l_r + w[1] * l_bc + w[2] * l_ic
        return self.grad(loss), np.array([l_r.item(), l_bc.item(), l_ic.item()])


def mse_to(u_bc, u_ic):
    """The ``value`` of Step.losses for tabulated targets: mean (u - target)^2."""
    targets = {"bc": u_bc, "ic": u_ic}
    return lambda u, which: ((u - as64(targets[which])) ** 2).mean()


def reference_loss(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, drop_unit=False,
                   encoding="angle"):
    """flat (NP,) weights in model.parameters() order and three (B, 3) point sets -> (grad (NP,), parts (3,)) float64:
    the gradient of 2 L_r + 4 L_bc + 2 L_ic and (L_r, L_bc, L_ic) on the analytic problem."""
    s = Step(flat, H, n, n_theta, theta_shape, ansatz, haar, X_ic, X_bc, X_res, drop_unit, encoding)
    X_val = {"bc": X_bc, "ic": X_ic}
    return s.weighted(s.losses(lambda u: (R.point_errors(u, X_res, PDE, 6) ** 2).mean(),
                               lambda u, which: ((u - R.analytic_u(X_val[which])) ** 2).mean()))


def layout_from_fixture(z, prefix, H, n, n_theta):
    """The flat weight vector of a reference fixture's ``<prefix>`` state (model.parameters() order)."""
    names = ("preprocessor__0__weight", "preprocessor__0__bias", "preprocessor__2__weight", "preprocessor__2__bias",
             "postprocessor__0__weight", "postprocessor__0__bias", "postprocessor__2__weight", "postprocessor__2__bias",
             "quantum_layer__params")
    flat = np.concatenate([np.asarray(z[prefix + k], dtype=np.float32).reshape(-1) for k in names])
    assert flat.size == R.layout(H, n, n_theta)[1]
    return flat


def step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt):
    """Seeded CPU draw of one case: flat float32 weights (initialiser-like scales; theta wide enough that the circuit
    gradient is not small) and float32 IC / BC / domain points in the trainer's boxes."""
    from oracle import solver as osol
    g = torch.Generator().manual_seed(1000 * salt + 7 * n + B_res + 3 * n_ic + 5 * n_bc)
    lay, NP = R.layout(H, n, n_theta)
    scale = {"W1": np.sqrt(2.0 / (H + 3)), "b1": 0.1, "W2": np.sqrt(2.0 / (H + n)), "b2": 0.1,
             "W3": 1.0 / np.sqrt(n), "b3": 0.3, "W4": 1.0 / np.sqrt(H), "b4": 0.1, "theta": 0.8}
    flat = np.zeros(NP, dtype=np.float32)
    for k, (o, s) in lay.items():
        m = int(np.prod(s))
        flat[o:o + m] = (torch.randn(m, generator=g, dtype=torch.float64) * scale[k]).numpy()
    X_ic, X_bc, X_res = [(torch.tensor(b[0]) + (torch.tensor(b[1]) - torch.tensor(b[0])) * torch.rand(m, 3, generator=g))
                         .to(torch.float32)
                         for b, m in ((osol.BOX_IC, n_ic), (osol.BOX_BC1, n_bc), (osol.BOX_DOM, B_res))]
    return flat, X_ic, X_bc, X_res


def haar_for(n, seed):
    """The oracle's fixed two-wire unitaries of a seeded layer (present for n >= 4), or None."""
    from oracle import statevector as sv
    return sv.haar_pair(seed, seed + 1) if (seed is not None and n >= 4) else None


# ---------------------------------------------------------------- committed records
class Record(NamedTuple):
    """One record of tests/golden/oracle/: the arguments of conftest.cached_oracle."""
    key: str
    inputs: list
    compute: Callable
    case: str = ""              # the id of the case in its module's CASES, for the writer's -k

    def get(self):
        return cached_oracle(self.key, self.inputs, self.compute)


def record(key, inputs, compute, H=None, variant="", dtype=np.float32, case=""):
    """Record ``key`` [+ "_H<H>"] [+ "_<variant>"] on the input arrays in the given order, as ``dtype``."""
    key += (f"_H{H}" if H else "") + (f"_{variant}" if variant else "")
    return Record(key, [np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype) for a in inputs], compute, case)


def case_key(prefix, case):
    """``<prefix>_<ansatz>_n<n>_L<L>_<encoding>_r<B_res>_i<n_ic>_b<n_bc>`` of a case tuple that starts with those seven."""
    ans, n, L, enc, B_res, n_ic, n_bc = case[:7]
    return f"{prefix}_{ans}_n{n}_L{L}_{enc}_r{B_res}_i{n_ic}_b{n_bc}"


def batch_inputs(*batches):
    """The arrays of a replay's batches, step by step, for a training record's inputs."""
    return [a for b in batches for a in b]


def flat_of(model):
    """The model's parameters as one vector, in model.parameters() order."""
    return np.concatenate([p.detach().numpy().reshape(-1) for p in model.parameters()])


def step_key(ansatz, n, L, seed, encoding, B_res, n_ic, n_bc, variant=""):
    return f"step_{ansatz}_n{n}_L{L}_s{seed}_{encoding}_r{B_res}_i{n_ic}_b{n_bc}" + (f"_{variant}" if variant else "")


def step_record(ansatz, n, L, seed, encoding, flat, X_ic, X_bc, X_res, H=50, variant=""):
    """The record of reference_loss on one case -> {"grad": (NP,), "parts": (3,)}.

    ``variant``: a negative control of the GPU tests.  "drop_res" / "drop_val" drop the last residual / value point
    (the value point is the last BC point, or the last IC point when there are no BC points); "swap_haar" swaps the
    two fixed unitaries; "drop_unit" removes hidden unit H - 1 from both networks (its records are keyed without the
    theta block)."""
    P = int(pkg("circuits").params_per_layer(ansatz, n))
    n_theta, theta_shape = L * P, (L, P)
    haar = haar_for(n, seed)
    Xi, Xb, Xr = X_ic, X_bc, X_res
    if variant == "drop_res":
        Xr = X_res[:-1]
    elif variant == "drop_val":
        if len(X_bc):
            Xb = X_bc[:-1]
        else:
            Xi = X_ic[:-1]
    elif variant == "swap_haar":
        haar = (haar[1], haar[0])
    elif variant and variant != "drop_unit":
        raise ValueError(variant)

    def compute():
        g, parts = reference_loss(flat, H, n, n_theta, theta_shape, ansatz, haar,
                                  *(torch.as_tensor(x).double() for x in (Xi, Xb, Xr)), drop_unit=variant == "drop_unit",
                                  encoding=encoding)
        return {"grad": g, "parts": parts}
    flat = np.asarray(flat, dtype=np.float32)
    theta = () if variant == "drop_unit" else (flat[R.layout(H, n, n_theta)[0]["theta"][0]:],)
    return record(step_key(ansatz, n, L, seed, encoding, len(X_res), len(X_ic), len(X_bc), variant),
                  (flat,) + theta + (X_ic, X_bc, X_res), compute)


def cached_step_reference(*args, **kw):
    return step_record(*args, **kw).get()
