"""Fused training of a ``DVPDESolver`` under gradient-norm loss weights (``qc_fused_pinn_gradnorm_step``).

A PINN whose residual gradient dwarfs the gradients of its data terms fits the operator and ignores the initial and
boundary conditions.  The learning-rate annealing of Wang, Teng and Perdikaris (2021) sets the weight of each data term
from the ratio of the gradient statistics of this step,

    hat_k = max|grad L_r| / mean|grad L_k|,      lam_k <- (1 - alpha) lam_k + alpha hat_k,      k = BC, IC,

and descends along grad L_r + lam_bc grad L_bc + lam_ic grad L_ic.  The weights need the three per-class gradients of the
step itself, which a host loop gets from three backward passes.  Here every stage writes one gradient row per 64-point
tile as always; with the IC / BC boundary of the value batch on a tile boundary a row belongs to one loss term, the row
fold keeps the three classes apart, and one single-block launch forms the statistics, moves the weights and combines the
gradients ahead of the unchanged optimiser launch.  The logged loss is w_res L_r + w_bc L_bc + w_ic L_ic, as in every other
step; the lambda-weighted loss goes into the history of the weights.
"""
from __future__ import annotations

from ..hip import engine as _engine
from ..nn.loss_balance import GradNormWeighting
from .diffusion_train import FusedTrainer, _dist_info, check_fused_single, check_tt, load_with_targets, run_fused_loop


def check_gradnorm(model, dataset, gradnorm, batch_size, adaptive=None, lbfgs=None, balance=None, causal=None, operator=None,
                   n_ic=None, n_bc=None):
    """The argument errors of ``gradnorm=``: one ``ValueError`` per fault, none of which needs a GPU.  ``n_ic`` / ``n_bc``
    default to the trainer's split, ``batch_size // 3`` each."""
    if not isinstance(gradnorm, GradNormWeighting):
        raise ValueError("gradnorm= must be an nn.loss_balance.GradNormWeighting")
    if dataset is not None and hasattr(dataset, "terms"):
        raise ValueError("gradnorm= does not take a system of equations (a TabulatedSystem)")
    check_tt(None, dataset, **{"gradnorm=": gradnorm})
    if adaptive is not None:
        raise ValueError("gradnorm= cannot be combined with adaptive= sampling")
    if lbfgs is not None:
        raise ValueError("gradnorm= cannot be combined with an lbfgs= phase: the objective moves with the weights")
    if balance is not None:
        raise ValueError("gradnorm= cannot be combined with balance=")
    if causal is not None:
        raise ValueError("gradnorm= cannot be combined with causal=")
    if operator is not None:
        raise ValueError("gradnorm= cannot be combined with a learned operator (the inverse step)")
    check_fused_single(model, "gradnorm", _dist_info()[0])
    n3 = int(batch_size) // 3
    n_ic, n_bc = (n3 if n_ic is None else int(n_ic)), (n3 if n_bc is None else int(n_bc))
    if n_ic > 0 and n_bc > 0 and n_ic % 64:
        raise ValueError(f"gradnorm= needs n_ic a multiple of 64 when IC and BC points are both present (a 64-point tile of "
                         f"the value batch must not mix them), got n_ic = {n_ic}: choose it with GradNormTrainer(..., n_ic=, n_bc=)")


class GradNormTrainer(FusedTrainer):
    """``FusedTrainer`` with the class fold and the gradient-norm combination in the step: on the analytic problem
    (``dataset`` None), on a ``TabulatedProblem``, or on one with a coefficient table.  Everything else (optimiser record,
    loss history, batches, samplers) is ``FusedTrainer``'s."""

    def __init__(self, model, batch_size: int, gradnorm: GradNormWeighting, dataset=None, *, capacity: int = 0,
                 n_ic: int = None, n_bc: int = None, loss_weights=(2.0, 4.0, 2.0), max_norm=1.0, sampler: str = "device",
                 pde: dict = None, bc_faces=1):
        check_gradnorm(model, dataset, gradnorm, batch_size, n_ic=n_ic, n_bc=n_bc)
        self.gradnorm = gradnorm
        self._gradnorm_cap = int(capacity)
        super().__init__(model, batch_size, capacity, sampler, n_ic=n_ic, n_bc=n_bc, loss_weights=loss_weights,
                         max_norm=max_norm, dataset=dataset, pde=pde, bc_faces=bc_faces)

    def _make_step(self):
        g = self.gradnorm
        return _engine.GradNormStep(self.eng, self.B_res, self.n_ic, self.n_bc, self.opt, g.alpha, g.every, g.lam_max, g.init,
                                    capacity=self._gradnorm_cap, counts=self.global_counts)

    def weights(self):
        """(lam_bc, lam_ic) of the next step (a host read)."""
        rec = self.fs.read_state()
        return rec["lam_bc"], rec["lam_ic"]

    def gradient_stats(self):
        """{"m_r", "a_bc", "a_ic", "hat_bc", "hat_ic", "n_updates"} of the last update (a host read)."""
        rec = self.fs.read_state()
        return {k: rec[k] for k in ("m_r", "a_bc", "a_ic", "hat_bc", "hat_ic", "n_updates")}

    def gradnorm_history(self, steps=None):
        """(steps, 7) array: row i holds (lam_bc, lam_ic, m_r, a_bc, a_ic, lambda-weighted loss, updated) of the i-th step,
        next to ``opt.loss_history()[i]``."""
        return self.fs.history(steps)


def train_gradnorm(model, batch_size, batches, dataset, gradnorm):
    """The loop of ``trainer.diffusion_train.train`` over a ``GradNormTrainer``."""
    steps = model.epochs + 1
    tr = GradNormTrainer(model, batch_size, gradnorm, dataset, capacity=steps)

    def finish(tr, steps):
        model.gradnorm_history = tr.gradnorm_history(steps)
    return run_fused_loop(model, tr, f"Starting training for {model.epochs} epochs with gradient-norm loss weights "
                          f"(alpha {gradnorm.alpha}, every {gradnorm.every} steps)...", batch_size, batches,
                          load_with_targets if dataset is not None else (lambda tr, b: tr.load_batches(*b[:3])),
                          lambda tr: "  gradient-norm weights: lam_bc %.3e | lam_ic %.3e" % tr.weights(), finish)
