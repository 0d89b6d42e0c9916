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
from .diffusion_train import _dist_info, batch_prologue, gather_rows, opt_state_from_torch, sync_opt_state_to_torch


class SystemTrainer:
    """Device-resident training state of one K-output DVPDESolver: the flat parameter buffer (``model.parameters()``
    order, the parameters re-pointed at views of it, so ``model.jets_all`` and the state dict keep working), the optimiser
    record taken from the model's torch Adam / ReduceLROnPlateau, and the step descriptor.  ``step()`` is one training
    iteration without host synchronisation."""

    def __init__(self, model, batch_size: int, dataset: TabulatedSystem, *, n_ic: int = None, n_bc: int = None,
                 loss_weights=(2.0, 4.0, 2.0), max_norm=1.0, capacity: int = 0, sampler: str = "device"):
        """``dataset``: the system (operator, weights, resident segments; empty segments serve ``load_batches`` only).
        ``batch_size`` residual, ``n_ic`` / ``n_bc`` (default ``batch_size // 3``) initial / boundary points per step;
        ``loss_weights`` = (residual, BC, IC); ``max_norm`` None: no clipping; ``capacity``: length of the loss history;
        ``sampler`` = "device" (the library's gather) or "torch" (``torch.randint`` rows and a copy)."""
        if not isinstance(dataset, TabulatedSystem):
            raise ValueError("SystemTrainer needs dataset= a TabulatedSystem (operator terms, weights and segments)")
        if getattr(model, "input_dim", 3) != 3:
            raise ValueError("SystemTrainer needs classic_network = [3, H, K]: a two-input model keeps a zero-padded t column "
                             "in W1 that the step would train")
        if getattr(getattr(model, "quantum_layer", None), "reupload", False):
            raise ValueError("SystemTrainer does not take a re-uploaded circuit (args['reupload']): train it with FusedTrainer")
        K = int(getattr(model, "n_out", 1))
        if K != dataset.K:
            raise ValueError(f"the model has {K} outputs but the dataset prescribes {dataset.K}")
        world, _ = _dist_info()
        if world > 1:
            raise ValueError("SystemTrainer is single-process: world_size > 1 is not supported")
        self.B_res, self.n_ic, self.n_bc, dev = batch_prologue(model, batch_size, n_ic, n_bc, sampler)
        self.model, self.device, self.K, self.sampler = model, dev, K, sampler
        self.dataset = dataset.to(dev)
        self.max_norm = max_norm
        self.loss_weights = tuple(float(w) for w in loss_weights)
        if not model._packed_ok() or model._flat.device != dev:
            model._pack(dev)             # one flat buffer in model.parameters() order, parameters re-pointed at views
        self.flat = model._flat
        self.circuit = model._circuit(dev)
        self.NP = self.flat.numel()
        self.optimizer, self.scheduler = model.optimizer, model.scheduler
        self.opt = self._make_opt_state(int(capacity))
        ds = self.dataset
        self.system = _lib.system_record(K, ds.n_eq, ds.terms, ds.eq_weights, ds.out_weights)
        self.has_r = ds.R is not None
        self.fs = _engine.SystemStep(self.circuit, model.hidden_width, self.flat, self.system, self.B_res, self.n_ic,
                                     self.n_bc, self.opt, loss_weights=self.loss_weights, res_targets=self.has_r)
        self._sampled = all(n_rows > 0 or n_batch == 0
                            for n_batch, n_rows in zip((self.B_res, self.n_ic, self.n_bc), ds.sizes()))
        if self._sampled:
            self.fs.set_dataset(ds.segments())
        self.fs.refresh_gates()
        self.fs.set_sampler(int(torch.randint(0, 2 ** 62, (1,)).item()))
        self._explicit = False
        model._sync_fused_to_torch = self.sync_to_torch

    # -- optimiser state: continue from the torch optimiser / scheduler objects of the model (FusedTrainer's rule)
    def _make_opt_state(self, capacity):
        return opt_state_from_torch(self.model.parameters(), self.optimizer, self.scheduler, self.device, capacity,
                                    self.max_norm, self.loss_weights)

    def sync_to_torch(self):
        """Mirror the device optimiser record into model.optimizer / model.scheduler (``save_state`` calls this)."""
        sync_opt_state_to_torch(self.opt, self.model.parameters(), self.optimizer, self.scheduler)

    # -- batches
    def sample(self):
        """Rows of the dataset, drawn with replacement.  With the device sampler this only arms the next ``step()``."""
        if not self._sampled:
            raise ValueError("the dataset has an empty segment behind a non-empty batch: use load_batches(...)")
        self._explicit = False
        if self.sampler == "device":
            return
        self._explicit = True
        gather_rows(self.fs, self.dataset.segments(), (self.B_res, self.n_ic, self.n_bc), batch_minor=True)

    def load_batches(self, X_ic, X_bc, X_res, targets):
        """Use given batches: ``targets`` = (U_ic (n_ic, K), U_bc (n_bc, K), R_res (B_res, n_eq) | None)."""
        U_ic, U_bc, R = targets
        fs, dev, ds = self.fs, self.device, self.dataset
        if (X_ic.shape[0], X_bc.shape[0], X_res.shape[0]) != (self.n_ic, self.n_bc, self.B_res):
            raise ValueError(f"batches must hold ({self.n_ic}, {self.n_bc}, {self.B_res}) points")
        if (R is None) != (not self.has_r):
            raise ValueError("residual targets are given exactly when the dataset has them (R is None: zero targets)")
        as32 = lambda a: torch.as_tensor(a, dtype=torch.float32).to(dev)
        for U, n, name in ((U_ic, self.n_ic, "U_ic"), (U_bc, self.n_bc, "U_bc")):
            if n and tuple(torch.as_tensor(U).shape) != (n, self.K):
                raise ValueError(f"{name} must be ({n}, {self.K}): one value per point and output")
        if R is not None and self.B_res and tuple(torch.as_tensor(R).shape) != (self.B_res, ds.n_eq):
            raise ValueError(f"R_res must be ({self.B_res}, {ds.n_eq}): one value per point and equation")
        self._explicit = True
        if self.n_ic:
            fs.X_val[: self.n_ic] = as32(X_ic)
            fs.target_val[:, : self.n_ic] = as32(U_ic).t()
        if self.n_bc:
            fs.X_val[self.n_ic: self.n_ic + self.n_bc] = as32(X_bc)
            fs.target_val[:, self.n_ic: self.n_ic + self.n_bc] = as32(U_bc).t()
        if self.B_res:
            fs.X_res[: self.B_res] = as32(X_res)
            if R is not None:
                fs.target_res[:, : self.B_res] = as32(R).t()

    def step(self):
        draw = 0 if self._explicit else _lib.QC_PHASE_SAMPLE
        self.fs.run(draw | _lib.QC_PHASE_GRADS | _lib.QC_PHASE_UPDATE)

    def loss_history(self, steps=None):
        return self.opt.loss_history(steps)

    def losses(self):
        rec = self.opt.read()
        return (rec["loss"], rec["loss_res"], rec["loss_bc"], rec["loss_ic"]), rec["lr"]
