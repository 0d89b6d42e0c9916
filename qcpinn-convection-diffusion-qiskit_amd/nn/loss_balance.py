"""Learned loss weights (homoscedastic-uncertainty balancing, Kendall et al. 2018).

One trainable log-variance per loss term; the balanced objective is

    F = sum_k ( w_k exp(-s_k) L_k + s_k ),

with ``w_k`` fixed base weights (1 unless given).  A large ``L_k`` pushes ``s_k`` up and its weight down until
``w_k exp(-s_k) L_k = 1``; the ``+ s_k`` term keeps the weights from collapsing to zero.  ``BalancedTrainer`` runs this rule
inside the fused step (``qc_fused_pinn_balanced_step``); this module is the torch-side holder of the three values and the
float reference of F.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

TERMS = ("residual", "bc", "ic")      # the fused step's order: its loss columns and the weights of its optimiser record


class AdaptiveMultiLoss(torch.nn.Module):
    """``log_vars`` is a ``ParameterDict`` with one ``(1,)`` parameter per name, so the ``state_dict`` keys are
    ``log_vars.<name>`` (a balancer saved by the reference's hybrid script loads as it is, given the same names).

    ``scale`` (optional, one finite number per name, default 1): the parameter of term k then holds ``p_k`` and the
    log-variance is ``s_k = scale_k * p_k``.  Adam moves every ``p_k`` by about ``lr`` per step, so ``scale_k`` is the
    learning-rate multiplier of ``s_k``; ``scale_k = 0`` freezes the term at its base weight.  ``scale`` is not part of
    the ``state_dict``."""

    def __init__(self, names: Sequence[str] = TERMS, scale: Optional[Sequence[float]] = None):
        super().__init__()
        names = tuple(names)
        if len(set(names)) != len(names) or not names:
            raise ValueError(f"loss term names must be distinct and not empty, got {names}")
        scale = [1.0] * len(names) if scale is None else [float(s) for s in scale]
        if len(scale) != len(names) or not all(math.isfinite(s) for s in scale):
            raise ValueError(f"scale needs one finite number per loss term ({len(names)}), got {scale}")
        self.names = names
        self.log_vars = torch.nn.ParameterDict({name: torch.nn.Parameter(torch.zeros(1)) for name in names})
        self.register_buffer("scale", torch.tensor(scale, dtype=torch.float32), persistent=False)

    def log_variances(self) -> Dict[str, torch.Tensor]:
        """``s_k = scale_k * p_k`` per name, differentiable."""
        return {name: self.scale[k].to(self.log_vars[name].dtype) * self.log_vars[name] for k, name in enumerate(self.names)}

    def forward(self, losses: Dict[str, torch.Tensor], base_weights: Optional[Dict[str, float]] = None) -> torch.Tensor:
        """F over the terms named in ``losses``; ``base_weights``: the fixed ``w_k`` per name (default 1)."""
        s = self.log_variances()
        total = None
        for name, loss in losses.items():
            w = 1.0 if base_weights is None else float(base_weights[name])
            term = (w * torch.exp(-s[name]) * loss + s[name]).reshape(())
            total = term if total is None else total + term
        if total is None:
            raise ValueError("no loss terms given")
        return total

    @torch.no_grad()
    def weights(self) -> Dict[str, float]:
        """``exp(-s_k)`` per name: the factor on the term's base weight."""
        return {name: float(torch.exp(-s).item()) for name, s in self.log_variances().items()}


class GradNormWeighting:
    """Gradient-norm loss weights (Wang, Teng, Perdikaris 2021, "learning-rate annealing"): every ``every`` steps

        lam_k <- (1 - alpha) lam_k + alpha max|grad L_r| / mean|grad L_k|,      k = BC, IC,

    capped at ``lam_max``, and the step descends along grad L_r + lam_bc grad L_bc + lam_ic grad L_ic
    (``qc_fused_pinn_gradnorm_step``, ``trainer.gradnorm_train``).  ``init`` = the starting (lam_bc, lam_ic).  A plain
    value object: the weights are no parameters, nothing here reaches an optimiser."""

    def __init__(self, alpha: float = 0.1, every: int = 10, lam_max: float = 1e4, init=(1.0, 1.0)):
        if isinstance(every, bool) or not isinstance(every, int) or every < 1:
            raise ValueError(f"gradient-norm weighting: every must be an integer >= 1, got {every!r}")
        alpha, lam_max = float(alpha), float(lam_max)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"gradient-norm weighting: alpha must lie in [0, 1], got {alpha!r}")
        if not (math.isfinite(lam_max) and lam_max > 0.0):
            raise ValueError(f"gradient-norm weighting: lam_max must be a finite number > 0, got {lam_max!r}")
        try:
            init = tuple(float(v) for v in init)
        except TypeError:
            init = ()
        if len(init) != 2 or not all(math.isfinite(v) and v > 0.0 for v in init):
            raise ValueError(f"gradient-norm weighting: init must be two finite numbers > 0 (lam_bc, lam_ic), got {init!r}")
        self.alpha, self.every, self.lam_max, self.init = alpha, every, lam_max, init

    def __repr__(self):
        return f"GradNormWeighting(alpha={self.alpha}, every={self.every}, lam_max={self.lam_max}, init={self.init})"
