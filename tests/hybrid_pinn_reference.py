"""Float64 restatement of the third workload (the reference's trainer/train.py) for the tests: the model with a circuit
built from oracle/statevector.py (RX, RY, RZ, CNOT; parity unpinned like every circuit of the oracle), its
loss and gradient, the reference's training loop, and the output map a = pi tanh(v) of the pre network in closed form.

Everything here is plain torch float64 on the CPU; nothing calls the library."""
import math

import numpy as np
import torch
import torch.nn as nn

F64 = torch.float64
D, VX, VY = 0.01, 1.0, 1.0
# state_dict keys / shapes of the reference's HybridPINN at Config's defaults (n = 4, L = 2, H = 50)
REFERENCE_KEYS = {"encoder.0.weight": (50, 3), "encoder.0.bias": (50,), "encoder.2.weight": (4, 50), "encoder.2.bias": (4,),
                  "q_layer.weights": (2, 4, 3), "decoder.0.weight": (50, 4), "decoder.0.bias": (50,),
                  "decoder.2.weight": (1, 50), "decoder.2.bias": (1,)}
# kernel (flat-parameter) order of the same tensors
KERNEL_ORDER = ("encoder.0.weight", "encoder.0.bias", "encoder.2.weight", "encoder.2.bias", "decoder.0.weight",
                "decoder.0.bias", "decoder.2.weight", "decoder.2.bias", "q_layer.weights")


def angle_map_fwd(v):
    """v: (6, ...) jets {value, t, x, y, xx, yy} of the network output -> jets of a = pi tanh(v) (or (1, ...) -> (1, ...))."""
    tau = torch.tanh(v[0])
    ps = math.pi * (1.0 - tau * tau)
    if v.shape[0] == 1:
        return (math.pi * tau)[None]
    return torch.stack([math.pi * tau, ps * v[1], ps * v[2], ps * v[3], ps * (v[4] - 2.0 * tau * v[2] ** 2),
                        ps * (v[5] - 2.0 * tau * v[3] ** 2)])


def angle_map_bwd(ab, a):
    """Closed-form reverse of angle_map_fwd from the angle jets alone (the kernel's prologue, csrc/qc_mlp.hip)."""
    tau = a[0] / math.pi
    ps = math.pi * (1.0 - tau * tau)
    if ab.shape[0] == 1:
        return (ps * ab[0])[None]
    v0 = (ps * ab[0] - 2.0 * tau * (a[1] * ab[1] + a[2] * ab[2] + a[3] * ab[3])
          - (2.0 * tau * a[4] + 2.0 * a[2] ** 2 / math.pi) * ab[4] - (2.0 * tau * a[5] + 2.0 * a[3] ** 2 / math.pi) * ab[5])
    return torch.stack([v0, ps * ab[1], ps * ab[2] - 4.0 * tau * a[2] * ab[4], ps * ab[3] - 4.0 * tau * a[3] * ab[5],
                        ps * ab[4], ps * ab[5]])


def exact_u(X):
    X = torch.as_tensor(X, dtype=F64)
    return torch.exp(-100.0 * ((X[:, 1:2] - 0.5) ** 2 + (X[:, 2:3] - 0.5) ** 2)) * torch.exp(-X[:, 0:1])


class StandIn(nn.Module):
    """The reference model in float64 with an oracle circuit: encoder Linear(3, H) - Tanh - Linear(H, n) - Tanh,
    RX(pi v_i), L x [Rot(w[l, i]) on every wire, CNOT ring], <Z_i>, decoder Linear(n, H) - Tanh - Linear(H, 1).
    Created in the reference's order (encoder, q_layer, decoder) with TorchLayer's uniform [0, 2 pi) weights."""

    def __init__(self, n=4, L=2, H=50):
        super().__init__()
        self.n, self.L = n, L
        self.encoder = nn.Sequential(nn.Linear(3, H), nn.Tanh(), nn.Linear(H, n), nn.Tanh())
        self.q_layer = nn.Module()
        self.q_layer.weights = nn.Parameter(nn.init.uniform_(torch.empty(L, n, 3), 0.0, 2 * math.pi))
        self.decoder = nn.Sequential(nn.Linear(n, H), nn.Tanh(), nn.Linear(H, 1))

    def circuit(self, v):
        from oracle import statevector as sv
        sim = sv.Simulator(self.n, v.shape[0])
        for i in range(self.n):
            sim.RX(v[:, i] * math.pi, i)
        w = self.q_layer.weights
        for layer in range(self.L):
            for i in range(self.n):
                sim.RZ(w[layer, i, 0], i)
                sim.RY(w[layer, i, 1], i)
                sim.RZ(w[layer, i, 2], i)
            for i in range(self.n):
                sim.CNOT(i, (i + 1) % self.n)
        return torch.stack([sim.expval_z(i) for i in range(self.n)], 1)

    def forward(self, x):
        return self.decoder(self.circuit(self.encoder(x)))

    def kernel_params(self):
        sd = dict(self.named_parameters())
        return [sd[k] for k in KERNEL_ORDER]


def standin(n, L, H, seed, state=None):
    """A float64 stand-in: drawn under torch.manual_seed(seed), or loaded from a float32 state_dict."""
    torch.manual_seed(seed)
    m = StandIn(n, L, H)
    if state is not None:
        m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.double()


def residual(model, X):
    """(f, u) by autograd in the inputs, as the reference's get_pde_residual."""
    t, x, y = [X[:, k:k + 1].clone().requires_grad_(True) for k in range(3)]
    inp = torch.cat([t, x, y], dim=1)
    u = model(inp)
    du = torch.autograd.grad(u, inp, torch.ones_like(u), create_graph=True)[0]
    u_x, u_y = du[:, 1:2], du[:, 2:3]
    u_xx = torch.autograd.grad(u_x, x, torch.ones_like(u_x), create_graph=True)[0]
    u_yy = torch.autograd.grad(u_y, y, torch.ones_like(u_y), create_graph=True)[0]
    return du[:, 0:1] + VX * u_x + VY * u_y - D * (u_xx + u_yy), u


def step_loss(model, X_ic, X_bc, X_res):
    """loss = L_pde + 5 L_ic + 5 L_bc (trainer/train.py:266-283) and its parts (L_r, L_bc, L_ic)."""
    X_ic, X_bc, X_res = (torch.as_tensor(v, dtype=F64) for v in (X_ic, X_bc, X_res))
    f, _ = residual(model, X_res)
    l_r = (f ** 2).mean()
    l_ic = ((model(X_ic) - exact_u(X_ic)) ** 2).mean()
    l_bc = ((model(X_bc) - exact_u(X_bc)) ** 2).mean()
    return l_r + 5.0 * l_ic + 5.0 * l_bc, (l_r, l_bc, l_ic)


def step_gradient(model, X_ic, X_bc, X_res):
    """[grad | L_r, L_bc, L_ic] of one step, the gradient in the kernels' flat order (theta last)."""
    loss, parts = step_loss(model, X_ic, X_bc, X_res)
    g = torch.autograd.grad(loss, model.kernel_params())
    return np.concatenate([x.detach().numpy().reshape(-1) for x in g] + [np.array([p.item() for p in parts])])


def train(model, batches, lr=0.005):
    """The reference loop (:254-289) on given batches: Adam, ReduceLROnPlateau(0.9, 200), no clipping.  Returns the
    loss history."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=200)
    hist = []
    for b in batches:
        opt.zero_grad()
        loss, _ = step_loss(model, *b)
        loss.backward()
        opt.step()
        sch.step(loss.item())
        hist.append(loss.item())
    return hist
