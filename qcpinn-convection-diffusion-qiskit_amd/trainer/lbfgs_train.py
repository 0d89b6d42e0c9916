"""L-BFGS as the second training phase of a ``DVPDESolver``: Adam gets into the basin, L-BFGS on a fixed batch takes the
loss down from there (the "Adam / L-BFGS" update of the reference's design note hybrid_testing/hybrid_qpinn.md).

``LbfgsTrainer`` attaches to an existing ``FusedTrainer`` and shares its parameters, batches, dataset and loss weights.  One
evaluation is the GRADS phase of the trainer's fused step followed by ``qc_lbfgs_step`` (include/qcpinn_hip.h) on the same
stream: the curvature history, the two-loop recursion and the line search all stay on the device, and no host read decides
whether a trial point is accepted.  The Adam moments and the scheduler record are not touched.

``LbfgsPhase`` is the argument of ``train(..., lbfgs=)``.
"""
from __future__ import annotations

from ..hip import engine as _engine
from ..hip import lib as _lib


class LbfgsPhase:
    """``train(model, ..., lbfgs=LbfgsPhase(evals=200))``: that many evaluations of L-BFGS behind the Adam epochs, on one
    fixed batch, or on a fresh one every ``new_batch_every`` evaluations.  ``options`` go to ``LbfgsTrainer`` (history,
    line_search, lr, c1, max_ls, shrink_lo, shrink_hi, curv_eps)."""

    OPTIONS = ("history", "line_search", "lr", "c1", "max_ls", "shrink_lo", "shrink_hi", "curv_eps", "keep_history")

    def __init__(self, evals: int, new_batch_every=None, **options):
        if int(evals) != evals or evals < 1:
            raise ValueError(f"LbfgsPhase needs evals >= 1, got {evals!r}")
        if new_batch_every is not None and (int(new_batch_every) != new_batch_every or new_batch_every < 1):
            raise ValueError(f"new_batch_every must be None or >= 1, got {new_batch_every!r}")
        unknown = sorted(set(options) - set(self.OPTIONS))
        if unknown:
            raise ValueError(f"unknown L-BFGS options {unknown}; known: {list(self.OPTIONS)}")
        self.evals, self.new_batch_every = int(evals), None if new_batch_every is None else int(new_batch_every)
        self.keep_history = bool(options.pop("keep_history", False))
        self.options = options


def _check_options(history, line_search, lr, c1, max_ls, shrink_lo, shrink_hi, curv_eps):
    """The argument errors of the hyper-parameters (the library refuses the same values with QC_ERR_ARG)."""
    if int(history) != history or not 1 <= history <= _lib.QC_LBFGS_MAX_HISTORY:
        raise ValueError(f"history must lie in 1..{_lib.QC_LBFGS_MAX_HISTORY}, got {history!r}")
    if line_search not in _engine.LBFGS_LINE_SEARCH:
        raise ValueError(f"line_search must be 'armijo', 'fixed' or None, got {line_search!r}")
    if int(max_ls) != max_ls or max_ls < 1:
        raise ValueError(f"max_ls must be >= 1, got {max_ls!r}")
    for name, v in (("lr", lr), ("c1", c1), ("shrink_lo", shrink_lo), ("shrink_hi", shrink_hi), ("curv_eps", curv_eps)):
        if not (v > 0 and v < float("inf")):
            raise ValueError(f"{name} must be positive and finite, got {v!r}")
    if shrink_lo > shrink_hi or shrink_hi >= 1:
        raise ValueError(f"need shrink_lo <= shrink_hi < 1, got {shrink_lo!r}, {shrink_hi!r}")


class LbfgsTrainer:
    """L-BFGS on the batches of ``fused_trainer`` (a ``FusedTrainer``).  ``step()`` = one evaluation: gradient and loss at
    the current parameters, then the state machine moves the parameters to the next point to evaluate.  ``finish()`` leaves
    the model at the last ACCEPTED point."""

    def __init__(self, fused_trainer, history=10, line_search="armijo", lr=1.0, c1=1e-4, max_ls=10, capacity=1024,
                 shrink_lo=0.1, shrink_hi=0.5, curv_eps=1e-10):
        _check_options(history, line_search, lr, c1, max_ls, shrink_lo, shrink_hi, curv_eps)
        if getattr(fused_trainer, "world", 1) > 1:
            raise ValueError("LbfgsTrainer runs on one rank: data-parallel L-BFGS is not supported (the library call itself "
                             "works on an all-reduced flat vector)")
        if getattr(fused_trainer, "tt", False):
            raise ValueError("LbfgsTrainer is not supported for a problem with d_tt: the seven-channel step "
                             "(qc_fused_pinn_coef_tt_step) has no L-BFGS form")
        if getattr(fused_trainer, "adaptive", None) is not None:
            raise ValueError("LbfgsTrainer needs a fixed objective: the trainer must not use adaptive= sampling")
        if int(capacity) != capacity or capacity < 0:
            raise ValueError(f"capacity must be >= 0, got {capacity!r}")
        self.tr = fused_trainer
        self.fs, self.eng = fused_trainer.fs, fused_trainer.eng
        self.state_dev = _engine.LbfgsState(self.eng.NP, fused_trainer.device, history=history, line_search=line_search, lr=lr,
                                            c1=c1, max_ls=max_ls, shrink_lo=shrink_lo, shrink_hi=shrink_hi, curv_eps=curv_eps,
                                            loss_weights=self.eng.loss_weights, capacity=int(capacity))
        self._theta_off = self.eng.NP - self.eng.n_theta
        self._batch_ready = bool(getattr(fused_trainer, "_explicit", False))

    # -- batches
    def new_batch(self, keep_history: bool = False) -> None:
        """A fresh batch from the trainer's sampler (drawn or gathered on the device, or by torch), then a restart: the next
        evaluation is a first evaluation at the current parameters."""
        tr = self.tr
        tr.sample()
        if not tr._explicit:        # the device sampler only arms the draw: fill the batches now, nothing else runs
            self.fs.run(_lib.QC_PHASE_SAMPLE)
        self._batch_ready = True
        self.state_dev.restart(keep_history)

    def load_batches(self, *args, keep_history: bool = False, **kw) -> None:
        self.tr.load_batches(*args, **kw)
        self._batch_ready = True
        self.state_dev.restart(keep_history)

    # -- one evaluation
    def evaluate_and_advance(self) -> None:
        if not self._batch_ready:
            self.new_batch()
        self.fs.run(_lib.QC_PHASE_GRADS)
        self.state_dev.advance(self.fs.flat_grad, self.eng.flat, self.eng.circuit, self._theta_off)

    step = evaluate_and_advance

    def state(self) -> dict:
        """The 128-byte record (a host read)."""
        return self.state_dev.read()

    def history(self, n=None):
        return self.state_dev.history(n)

    def accepted_losses(self, n=None):
        """Losses of the accepted evaluations so far, in order."""
        h = self.history(n)
        return [float(f) for f, _, acc in h if acc > 0.5]

    def finish(self) -> None:
        """The model at the last accepted point x_k (not at a pending trial), gates refreshed."""
        if self.state()["n_iter"] > 0:
            self.eng.flat.copy_(self.state_dev.x_k())
        self.eng.refresh_gates()


def run_phase(tr, phase: LbfgsPhase):
    """``phase.evals`` evaluations behind the Adam steps of the FusedTrainer ``tr``; returns the LbfgsTrainer (finished)."""
    lb = LbfgsTrainer(tr, capacity=phase.evals, **phase.options)
    lb.new_batch()
    for e in range(phase.evals):
        if phase.new_batch_every and e > 0 and e % phase.new_batch_every == 0:
            lb.finish()             # a new batch starts from the last accepted point
            lb.new_batch(phase.keep_history)
        lb.step()
    lb.finish()
    return lb
