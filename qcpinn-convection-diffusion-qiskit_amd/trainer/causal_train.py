"""Fused causal training of a ``DVPDESolver`` on a time-dependent dataset (``qc_fused_pinn_causal_step``).

A PINN on a problem that marches in t can settle on a wrong solution at late times: the residual there is cheap to lower
before the solution at earlier times is right.  Causal training (Wang, Sankaran, Perdikaris 2022) cuts the residual points
into M time slabs and weighs slab i by how well the earlier slabs are fitted,

    L_r^c = (1/M) sum_i W_i L_i,      W_i = exp(-eps sum_{k<i} L_k),      W_0 = 1,

with the weights constants when differentiating, and raises eps once even the last slab's weight has passed ``delta``.
The weights depend on this step's slab losses, so the host could only set them with a synchronisation per step; here the
residual batch is drawn one slab per 64-point tile, every stage writes one gradient row per tile as always, and the row
fold sums the rows of slab i with W_i, formed on the device from the loss column of the same rows just before.
"""
from __future__ import annotations

from ..data.tabulated import CausalWeighting, TabulatedProblem
from ..hip import engine as _engine
from .diffusion_train import FusedTrainer, _dist_info, check_fused_single, check_tt, load_with_targets, run_fused_loop


def check_causal(model, dataset, causal, batch_size, adaptive=None, lbfgs=None, balance=None, operator=None):
    """The argument errors of ``causal=``: one ``ValueError`` per fault, none of which needs a GPU."""
    if not isinstance(causal, CausalWeighting):
        raise ValueError("causal= must be a data.tabulated.CausalWeighting")
    if dataset is not None and not isinstance(dataset, TabulatedProblem) and hasattr(dataset, "terms"):
        raise ValueError("causal= does not take a system of equations (a TabulatedSystem)")
    if not isinstance(dataset, TabulatedProblem):
        raise ValueError("causal= needs dataset= a TabulatedProblem: the analytic problems can be tabulated first")
    check_tt(None, dataset, **{"causal=": causal})
    if dataset.coef_res is not None:
        raise ValueError("causal= does not take a per-point coefficient table (dataset.coef_res)")
    if adaptive is not None:
        raise ValueError("causal= cannot be combined with adaptive= sampling: the residual rows are drawn by slab")
    if lbfgs is not None:
        raise ValueError("causal= cannot be combined with an lbfgs= phase: the objective moves with the weights")
    if balance is not None:
        raise ValueError("causal= cannot be combined with balance=")
    if operator is not None:
        raise ValueError("causal= cannot be combined with a learned operator (the inverse step)")
    check_fused_single(model, "causal", _dist_info()[0])
    tile = 64 * causal.n_slabs
    if isinstance(batch_size, bool) or int(batch_size) <= 0 or int(batch_size) % tile:
        raise ValueError(f"causal= needs a batch size that is a positive multiple of 64 * n_slabs = {tile}, got {batch_size}")


class CausalTrainer(FusedTrainer):
    """``FusedTrainer`` on a dataset whose residual segment is sorted by t and drawn one slab per tile, with the causal
    fold in the step.  ``load_batches`` takes residual batches laid out the same way: points [64 r, 64 r + 64) in slab
    r mod M.  Everything else (optimiser record, histories of the loss, value batches) is ``FusedTrainer``'s; the logged
    residual loss is L_r^c."""

    def __init__(self, model, batch_size: int, dataset: TabulatedProblem, causal: CausalWeighting, *, capacity: int = 0,
                 n_ic: int = None, n_bc: int = None, loss_weights=(2.0, 4.0, 2.0), max_norm=1.0, sampler: str = "device"):
        check_causal(model, dataset, causal, batch_size)
        if sampler != "device":
            raise ValueError("causal= draws its residual rows by slab on the device: sampler must be 'device'")
        self.causal = causal
        self._causal_cap = int(capacity)
        sorted_ds, self.slab_lo = causal.stratify(dataset)
        super().__init__(model, batch_size, capacity, sampler, n_ic=n_ic, n_bc=n_bc, loss_weights=loss_weights,
                         max_norm=max_norm, dataset=sorted_ds)
        self.fs.set_slabs(self.slab_lo)

    def _make_step(self):
        c = self.causal
        return _engine.CausalStep(self.eng, self.B_res, self.n_ic, self.n_bc, self.opt, c.n_slabs, c.eps, c.growth, c.eps_max,
                                  c.delta, capacity=self._causal_cap, counts=self.global_counts)

    def causal_weights(self):
        """(M,) float32 array: the slab weights W_i the last step used (a host read)."""
        return self.fs.read_state()["W"]

    def slab_losses(self):
        """(M,) float32 array: the mean squared residual L_i of every slab in the last step's batch (a host read)."""
        return self.fs.read_state()["L"]

    def epsilon(self):
        """(eps of the next step, how often it has been raised)."""
        rec = self.fs.read_state()
        return rec["eps"], rec["n_raised"]

    def causal_history(self, steps=None):
        """(steps, 1 + 2 M) array: row i holds (eps, W[M], L[M]) of the i-th step, next to ``opt.loss_history()[i]``."""
        return self.fs.history(steps)


def train_causal(model, batch_size, batches, dataset, causal):
    """The loop of ``trainer.diffusion_train.train`` over a ``CausalTrainer``."""
    steps = model.epochs + 1
    tr = CausalTrainer(model, batch_size, dataset, causal, capacity=steps)

    def extra_line(tr):
        eps, raised = tr.epsilon()
        w = tr.causal_weights()
        return f"  causal weights: min {float(w.min()):.3e} | eps (next step): {eps:.3e}, raised {raised} times"

    def finish(tr, steps):
        model.causal_history = tr.causal_history(steps)
    return run_fused_loop(model, tr, f"Starting training for {model.epochs} epochs with causal weights over "
                          f"{causal.n_slabs} time slabs...", batch_size, batches, load_with_targets, extra_line, finish)
