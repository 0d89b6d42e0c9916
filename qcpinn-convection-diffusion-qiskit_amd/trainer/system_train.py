"""Fused training of a K-output ``DVPDESolver`` on a system of equations (``qc_fused_pinn_system_step``).

The reference trains its Navier-Stokes model, (t, x, y) -> (u, v, p) behind one shared network (nn/pde.py:2-27), with
``navier_stokes_2D_operator`` -> three MSEs -> ``backward`` -> ``clip_grad_norm_`` -> Adam -> scheduler, all in torch.  A
``SystemTrainer`` runs that iteration as one library call: the operator is a term list (``nn.pde.navier_stokes_2D_terms``),
the points and the target rows come from a device-resident ``data.tabulated.TabulatedSystem`` (gathered on the device) or
from ``load_batches``, and the loss is

    w_res sum_e w_eq[e] MSE(res_e - r_e) + w_bc sum_k w_out[k] MSE_bc(u_k - U_k) + w_ic sum_k w_out[k] MSE_ic(u_k - U_k).
"""
from __future__ import annotations

import torch

from ..data.tabulated import TabulatedSystem
from ..hip import engine as _engine
from ..hip import lib as _lib
from .diffusion_train import DatasetTrainer, _dist_info, check_tt, fill_batches


class SystemTrainer(DatasetTrainer):
    """Device-resident training state of one K-output DVPDESolver: the flat parameter buffer (``model.parameters()``
    order, the parameters re-pointed at views of it, so ``model.jets_all`` and the state dict keep working), the optimiser
    record taken from the model's torch Adam / ReduceLROnPlateau, and the step descriptor.  ``step()`` is one training
    iteration without host synchronisation."""

    batch_minor = True      # target rows [N, K] / [N, n_eq] go into [K][B] / [n_eq][B] targets

    def __init__(self, model, batch_size: int, dataset: TabulatedSystem, *, n_ic: int = None, n_bc: int = None,
                 loss_weights=(2.0, 4.0, 2.0), max_norm=1.0, capacity: int = 0, sampler: str = "device"):
        """``dataset``: the system (operator, weights, resident segments; empty segments serve ``load_batches`` only).
        ``batch_size`` residual, ``n_ic`` / ``n_bc`` (default ``batch_size // 3``) initial / boundary points per step;
        ``loss_weights`` = (residual, BC, IC); ``max_norm`` None: no clipping; ``capacity``: length of the loss history;
        ``sampler`` = "device" (the library's gather) or "torch" (``torch.randint`` rows and a copy)."""
        check_tt(None, dataset, SystemTrainer=True)
        if not isinstance(dataset, TabulatedSystem):
            raise ValueError("SystemTrainer needs dataset= a TabulatedSystem (operator terms, weights and segments)")
        if getattr(model, "input_dim", 3) != 3:
            raise ValueError("SystemTrainer needs classic_network = [3, H, K]: a two-input model keeps a zero-padded t column "
                             "in W1 that the step would train")
        if getattr(getattr(model, "quantum_layer", None), "reupload", False):
            raise ValueError("SystemTrainer does not take a re-uploaded circuit (args['reupload'], with or without "
                             "args['reupload_scale']): train it with FusedTrainer")
        self.K = int(getattr(model, "n_out", 1))
        if self.K != dataset.K:
            raise ValueError(f"the model has {self.K} outputs but the dataset prescribes {dataset.K}")
        world, _ = _dist_info()
        if world > 1:
            raise ValueError("SystemTrainer is single-process: world_size > 1 is not supported")
        self.has_r = dataset.R is not None
        super().__init__(model, batch_size, dataset, n_ic, n_bc, loss_weights, max_norm, capacity, sampler)

    def _make_step(self):
        ds = self.dataset
        self.system = _lib.system_record(self.K, ds.n_eq, ds.terms, ds.eq_weights, ds.out_weights)
        return _engine.SystemStep(self.circuit, self.model.hidden_width, self.flat, self.system, self.B_res, self.n_ic,
                                  self.n_bc, self.opt, loss_weights=self.loss_weights, res_targets=self.has_r)

    def load_batches(self, X_ic, X_bc, X_res, targets):
        """Use given batches: ``targets`` = (U_ic (n_ic, K), U_bc (n_bc, K), R_res (B_res, n_eq) | None)."""
        U_ic, U_bc, R = targets
        if (X_ic.shape[0], X_bc.shape[0], X_res.shape[0]) != (self.n_ic, self.n_bc, self.B_res):
            raise ValueError(f"batches must hold ({self.n_ic}, {self.n_bc}, {self.B_res}) points")
        if (R is None) != (not self.has_r):
            raise ValueError("residual targets are given exactly when the dataset has them (R is None: zero targets)")
        for U, n, name in ((U_ic, self.n_ic, "U_ic"), (U_bc, self.n_bc, "U_bc")):
            if n and tuple(torch.as_tensor(U).shape) != (n, self.K):
                raise ValueError(f"{name} must be ({n}, {self.K}): one value per point and output")
        n_eq = self.dataset.n_eq
        if R is not None and self.B_res and tuple(torch.as_tensor(R).shape) != (self.B_res, n_eq):
            raise ValueError(f"R_res must be ({self.B_res}, {n_eq}): one value per point and equation")
        self._explicit = True
        fill_batches(self.fs, (self.B_res, self.n_ic, self.n_bc), (X_ic, X_bc, X_res), targets, batch_minor=True)
