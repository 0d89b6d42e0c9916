"""Fused training of a ``DVPDESolver`` under learned loss weights (``qc_fused_pinn_balanced_step``).

The tabulated step minimises ``w_res L_r + w_bc L_bc + w_ic L_ic`` with weights fixed for the run.  Here the three terms
are balanced by one trainable log-variance each (``nn.loss_balance.AdaptiveMultiLoss``, the interface of the reference's
hybrid script):

    F = sum_k ( w_k exp(-s_k) L_k + s_k ),      s_k = scale_k p_k,      k = residual, BC, IC.

The weights of a step depend on the losses of the step before, so setting them from the host would cost a synchronisation
per step; a ``BalancedTrainer`` keeps the three ``p_k`` on the device behind the model's parameters and runs the whole
iteration, their gradient and their Adam update included, as one library call.  As in the reference, the gradient clip
covers the model's parameters only.  The reference's script uses AdamW; this step keeps the model's Adam.
"""
from __future__ import annotations

from ..data.tabulated import TabulatedProblem
from ..hip import engine as _engine
from ..nn.loss_balance import TERMS, AdaptiveMultiLoss
from .diffusion_train import _dist_info, check_fused_single, check_tt, load_with_targets, run_fused_loop
from .inverse_train import InverseTrainer


def check_balance(model, dataset, balancer, adaptive=None, lbfgs=None):
    """The argument errors of ``balance=``: one ``ValueError`` per fault, none of which needs a GPU."""
    if not isinstance(balancer, AdaptiveMultiLoss):
        raise ValueError("balance= must be an nn.loss_balance.AdaptiveMultiLoss")
    if sorted(balancer.names) != sorted(TERMS):
        raise ValueError(f"the balancer's names must be exactly the three loss terms {TERMS}, got {tuple(balancer.names)}")
    if not isinstance(dataset, TabulatedProblem):
        raise ValueError("balance= needs dataset= a TabulatedProblem: the analytic problems can be tabulated first")
    check_tt(None, dataset, **{"balance=": balancer})
    if dataset.coef_res is not None:
        raise ValueError("balance= does not take a per-point coefficient table (dataset.coef_res)")
    if adaptive is not None:
        raise ValueError("balance= cannot be combined with adaptive= sampling")
    if lbfgs is not None:
        raise ValueError("balance= cannot be combined with an lbfgs= phase")
    check_fused_single(model, "balance", _dist_info()[0])


class BalancedTrainer(InverseTrainer):
    """Device-resident training state of one single-output DVPDESolver and one AdaptiveMultiLoss: ONE flat buffer of
    ``NP + 3`` entries with the model's parameters in its head (``model.parameters()`` order, re-pointed at views of it)
    and the three ``log_vars`` in its tail, in the order residual, BC, IC, so ``model(X)``, ``save_state`` and
    ``balancer.weights()`` see the trained values with no copy; the optimiser record taken from the model's torch Adam /
    ReduceLROnPlateau (which the balancer joins as a second param group); and the step descriptor.  ``step()`` is one
    training iteration without host synchronisation.  Batches, sampling and the optimiser record are ``InverseTrainer``'s."""

    def __init__(self, model, batch_size: int, dataset: TabulatedProblem, balancer: AdaptiveMultiLoss, *, n_ic: int = None,
                 n_bc: int = None, loss_weights=(2.0, 4.0, 2.0), max_norm=1.0, capacity: int = 0, sampler: str = "device"):
        """``dataset``: the resident segments and the operator (``coeffs``, ``c_u``) of the tabulated step; ``batch_size``
        residual, ``n_ic`` / ``n_bc`` (default ``batch_size // 3``) value points per step; ``loss_weights`` = the base
        weights w_k (residual, BC, IC); ``capacity``: length of the histories of F and of the effective weights."""
        super().__init__(model, batch_size, dataset, balancer, n_ic=n_ic, n_bc=n_bc, loss_weights=loss_weights,
                         max_norm=max_norm, capacity=capacity, sampler=sampler)

    FLAT_ATTR = "_balanced_flat"
    _check = staticmethod(check_balance)
    balancer = property(lambda self: self.operator)

    @staticmethod
    def _own(balancer):
        """The three ``log_vars`` in the step's order (residual, BC, IC), whatever the balancer's."""
        return [balancer.log_vars[name] for name in TERMS]

    def _make_step(self):
        ds, bal = self.dataset, self.balancer
        scale = bal.scale.tolist()
        scale = [scale[bal.names.index(name)] for name in TERMS]      # the step's order, whatever the balancer's
        return _engine.BalancedStep(self.circuit, self.model.hidden_width, self.flat, scale, self.B_res, self.n_ic, self.n_bc,
                                    self.opt, ds.coeffs, ds.c_u, loss_weights=self.loss_weights)

    def weight_history(self, steps=None):
        """(steps, 3) tensor: row i holds the effective weights w_k exp(-s_k) (residual, BC, IC) the i-th step of THIS
        history buffer used, next to ``loss_history()[i]`` (default: all steps taken so far)."""
        return _engine.history_rows(self.fs.weight_hist, steps, self.opt.hist_cap, self.opt.read)

    def weights(self):
        """The current effective weights w_k exp(-s_k) as a dict over the three terms."""
        e = self.balancer.weights()
        return {name: w * e[name] for name, w in zip(TERMS, self.loss_weights)}

    def coefficient_history(self, steps=None):
        raise AttributeError("a BalancedTrainer trains no operator: see weight_history() and weights()")

    coefficients = coefficient_history


def train_balanced(model, batch_size, batches, dataset, balancer):
    """The loop of ``trainer.diffusion_train.train`` over a ``BalancedTrainer``: the logged loss is F."""
    tr = BalancedTrainer(model, batch_size, dataset, balancer, capacity=model.epochs + 1)
    return run_fused_loop(model, tr, f"Starting training for {model.epochs} epochs with learned loss weights...", batch_size,
                          batches, load_with_targets,
                          lambda tr: "  loss weights: " + ", ".join(f"{k} {v:.3e}" for k, v in tr.weights().items()))
