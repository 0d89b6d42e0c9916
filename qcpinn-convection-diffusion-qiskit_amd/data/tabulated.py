"""A user's own problem as data: collocation points with their targets, and the coefficients of the linear operator

    residual = c_u u + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy).

The reference's ``Sampler(dim, coords, func)`` (data/diffusion_dataset.py:12-19) accepts ANY callable as the target and
its ``train()`` compares against whatever ``u`` and ``r`` it is handed; the fused HIP step computes only three analytic
targets in-kernel.  A ``TabulatedProblem`` is the general case for that step: the targets are evaluated (or measured)
once, up front, the three segments live on the device, and every training step gathers its minibatch from them on the
device (``qc_sample_dataset``: sampling with replacement, like a ``torch.randint`` minibatch) and reads the targets from
memory (``qc_fused_pinn_data_step``).  ``from_functions`` is the counterpart of ``Sampler(..., func)``.
"""
from __future__ import annotations

import torch

from .diffusion_dataset import box

MAX_ROWS = 2 ** 31 - 1      # the device gather forms (32-bit word * rows) >> 32


def _segment(name, X, y):
    """(X (N, 3) float32, y (N,) float32) of one segment; an (N, 1) target column is flattened; N = 0 is allowed."""
    X, y = torch.as_tensor(X), torch.as_tensor(y)
    if X.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError(f"{name}: points and targets must be float32 tensors, got {X.dtype} and {y.dtype}")
    if X.dim() != 2 or X.shape[1] != 3:
        raise ValueError(f"{name}: points must have shape (N, 3) = (t, x, y) rows, got {tuple(X.shape)}")
    if y.dim() == 2 and y.shape[1] == 1:
        y = y.reshape(-1)
    if y.dim() != 1:
        raise ValueError(f"{name}: targets must have shape (N,) or (N, 1), got {tuple(y.shape)}")
    if y.shape[0] != X.shape[0]:
        raise ValueError(f"{name}: {X.shape[0]} points but {y.shape[0]} targets")
    if X.shape[0] > MAX_ROWS:
        raise ValueError(f"{name}: at most {MAX_ROWS} rows per segment, got {X.shape[0]}")
    return X.contiguous(), y.contiguous()


class TabulatedProblem:
    """Residual points with forcing values ``r``, initial points with ``u_ic``, boundary points with ``u_bc``."""

    def __init__(self, X_res, r, X_ic, u_ic, X_bc, u_bc, *, c_t=1.0, c_x=1.0, c_y=1.0, d_xx=0.01, d_yy=0.01, c_u=0.0):
        self.X_res, self.r = _segment("residual segment", X_res, r)
        self.X_ic, self.u_ic = _segment("initial segment", X_ic, u_ic)
        self.X_bc, self.u_bc = _segment("boundary segment", X_bc, u_bc)
        self.coeffs = tuple(float(c) for c in (c_t, c_x, c_y, d_xx, d_yy))
        self.c_u = float(c_u)

    @classmethod
    def from_functions(cls, u_ic, u_bc, r, n_res, n_ic, n_bc, generator=None, **coeffs):
        """Evaluate the callables ``u_ic(X)``, ``u_bc(X)``, ``r(X)`` (X: (N, 3) rows (t, x, y) -> (N,) or (N, 1)) on
        uniform points of the trainer's three boxes (trainer/diffusion_train.py:9-20: t = 0 face, x = 0 face, unit cube),
        drawn IC -> BC -> residual from ``generator`` (default: torch's CPU generator)."""
        segs = []
        for name, n, f in (("ics", n_ic, u_ic), ("bc1", n_bc, u_bc), ("dom", n_res, r)):
            b = box(name, "cpu")
            X = b[0:1] + (b[1:2] - b[0:1]) * torch.rand(int(n), 3, generator=generator)
            y = torch.as_tensor(f(X), dtype=torch.float32) if n else torch.zeros(0)
            segs.append((X, y))
        (Xi, ui), (Xb, ub), (Xr, rr) = segs
        return cls(Xr, rr, Xi, ui, Xb, ub, **coeffs)

    # ---- the three segments in the order the samplers use: residual, IC, BC
    def segments(self):
        return ((self.X_res, self.r), (self.X_ic, self.u_ic), (self.X_bc, self.u_bc))

    def sizes(self):
        return tuple(int(X.shape[0]) for X, _ in self.segments())

    def to(self, device):
        """The same problem with its segments on ``device`` (moved once; a problem already there is returned as is)."""
        device = torch.device(device)
        if all(X.device == device and y.device == device for X, y in self.segments()):
            return self
        c = dict(zip(("c_t", "c_x", "c_y", "d_xx", "d_yy"), self.coeffs), c_u=self.c_u)
        (Xr, rr), (Xi, ui), (Xb, ub) = [(X.to(device), y.to(device)) for X, y in self.segments()]
        return TabulatedProblem(Xr, rr, Xi, ui, Xb, ub, **c)
