"""Fused training of a ``DVPDESolver`` on an inverse problem (``qc_fused_pinn_inverse_step``).

Measurements of ``u`` are given and coefficients of the operator

    residual = c_u u + c_3 u^3 + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy)

are identified together with the network.  The reference's generic torch loop would serve this by handing the coefficient
to Adam as one more ``nn.Parameter``; an ``InverseTrainer`` keeps the coefficients on the device behind the model's
parameters and runs the whole iteration, their gradient and their Adam update included, as one library call.  The
observations of ``u`` go into the IC / BC segments of a ``data.tabulated.TabulatedProblem`` (value points may lie anywhere
in the domain), the residual points and their forcing values into its residual segment, the operator into a
``data.tabulated.LearnedOperator``.
"""
from __future__ import annotations

import torch

from ..data.tabulated import LearnedOperator, TabulatedProblem, _SCALARS
from ..hip import engine as _engine
from .diffusion_train import DatasetTrainer, _dist_info, check_tt, fill_batches


def pack_with_tail(model, tail, attr, dev):
    """One flat float32 buffer [model parameters | the tensors of ``tail``] on ``dev``, cached on the model as ``attr``: the
    model's own flat buffer becomes its head (a view), the way ``model._pack`` builds it, and the Parameters of ``tail``
    become views of what follows, in order.  Returns the buffer; rebuilt only when one of the views no longer holds."""
    if not model._packed_ok() or model._flat.device != dev:
        model._pack(dev)             # one flat buffer in model.parameters() order, parameters re-pointed at views
    NP = model._flat.numel()
    offs = [NP + sum(p.numel() for p in tail[:k]) for k in range(len(tail) + 1)]
    big = getattr(model, attr, None)
    if not (big is not None and big.device == dev and big.numel() == offs[-1] and model._flat.data_ptr() == big.data_ptr()
            and all(p.data_ptr() == big.data_ptr() + 4 * o for p, o in zip(tail, offs))):
        big = torch.cat([model._flat.detach()] + [p.detach().reshape(-1).to(device=dev, dtype=torch.float32) for p in tail])
        off = 0
        for p, k, pad in model._slots():
            p.data = big[off:off + k].view(p.shape)
            off += k
        model._flat = big[:NP]
        model._engines = {}
        setattr(model, attr, big)
        for p, o in zip(tail, offs):
            p.data = big[o:o + p.numel()].view(p.shape)
    return big


class InverseTrainer(DatasetTrainer):
    """Device-resident training state of one single-output DVPDESolver and one LearnedOperator: ONE flat buffer of
    ``NP + 7`` entries with the model's parameters in its head (``model.parameters()`` order, re-pointed at views of it)
    and ``operator.p`` in its tail, so ``model(X)``, ``model.residual``, ``save_state`` and ``operator.coefficients()`` see
    the trained values with no copy; the optimiser record taken from the model's torch Adam / ReduceLROnPlateau (which
    ``operator.p`` joins as a second param group); and the step descriptor.  ``step()`` is one training iteration without
    host synchronisation."""

    def __init__(self, model, batch_size: int, dataset: TabulatedProblem, operator: LearnedOperator, *, n_ic: int = None,
                 n_bc: int = None, loss_weights=(2.0, 4.0, 2.0), max_norm=1.0, capacity: int = 0, sampler: str = "device"):
        """``dataset``: the resident segments (empty segments serve ``load_batches`` only); its scalar coefficients stay at
        their defaults and it has no ``coef_res``: the operator is ``operator``.  ``batch_size`` residual, ``n_ic`` /
        ``n_bc`` (default ``batch_size // 3``) value points per step; ``loss_weights`` = (residual, BC, IC); ``max_norm``
        None: no clipping; ``capacity``: length of the loss and coefficient histories; ``sampler`` = "device" (the
        library's gather) or "torch" (``torch.randint`` rows and a copy)."""
        self._check(model, dataset, operator)
        self.operator = operator
        super().__init__(model, batch_size, dataset, n_ic, n_bc, loss_weights, max_norm, capacity, sampler)

    FLAT_ATTR = "_inverse_flat"     # where the model keeps the flat buffer [model parameters | own entries]

    @staticmethod
    def _check(model, dataset, operator):
        """The argument errors that need no GPU."""
        if not isinstance(dataset, TabulatedProblem):
            raise ValueError("InverseTrainer needs dataset= a TabulatedProblem (residual and observation segments)")
        if not isinstance(operator, LearnedOperator):
            raise ValueError("InverseTrainer needs operator= a LearnedOperator")
        check_tt(None, dataset, **{"InverseTrainer": operator})
        if dataset.coef_res is not None:
            raise ValueError("the dataset carries a per-point coefficient table (coef_res): an inverse problem takes its "
                             "coefficients from operator= (LearnedOperator(fixed=..., learn=...)), one global value each")
        defaults = tuple(float(_SCALARS[k]) for k in ("c_t", "c_x", "c_y", "d_xx", "d_yy"))
        if tuple(dataset.coeffs) != defaults or dataset.c_u != float(_SCALARS["c_u"]):
            raise ValueError("the dataset's scalar coefficients are not read by an inverse problem: leave them at their "
                             "defaults and give them to operator= (LearnedOperator(fixed=..., learn=...))")
        if getattr(model, "input_dim", 3) != 3 or int(getattr(model, "n_out", 1)) != 1:
            raise ValueError("InverseTrainer needs classic_network = [3, H, 1]")
        world, _ = _dist_info()
        if world > 1:
            raise ValueError("InverseTrainer is single-process: world_size > 1 is not supported")

    @staticmethod
    def _own(operator):
        """The trainable tensors behind the model's parameters, in the flat buffer's order."""
        return [operator.p]

    def _make_step(self):
        op = self.operator
        return _engine.InverseStep(self.circuit, self.model.hidden_width, self.flat, op.base.tolist(), op.scale.tolist(),
                                   self.B_res, self.n_ic, self.n_bc, self.opt, loss_weights=self.loss_weights)

    @classmethod
    def attach(cls, model, operator):
        """The own entries (``operator.p``; a balancer's ``log_vars``) join ``model.optimizer`` as a second param group with
        the hyper-parameters of the first, if they are not there yet (the constructor calls this; call it on a fresh model
        before loading a saved optimiser state)."""
        opt, own = model.optimizer, cls._own(operator)
        if not any(p is own[0] for g in opt.param_groups for p in g["params"]):
            g0 = opt.param_groups[0]
            opt.add_param_group({"params": own, **{k: v for k, v in g0.items() if k != "params"}})
            sch = model.scheduler
            sch.min_lrs = list(sch.min_lrs) + [sch.min_lrs[0]] * (len(opt.param_groups) - len(sch.min_lrs))

    def _params(self):
        return super()._params() + self._own(self.operator)

    def _pack(self):
        """One flat buffer [model parameters | own entries]: ``self.flat``, with ``self.NP`` model parameters in its head;
        the own entries join the optimiser behind it."""
        self.flat = pack_with_tail(self.model, self._own(self.operator), self.FLAT_ATTR, self.device)
        self.NP = self.model._flat.numel()
        for b in self.operator.buffers():       # base / scale follow to the device
            b.data = b.to(self.device)
        self.attach(self.model, self.operator)

    def load_batches(self, X_ic, X_bc, X_res, targets):
        """Use given batches: ``targets`` = (u_ic (n_ic,), u_bc (n_bc,), r_res (B_res,))."""
        if (X_ic.shape[0], X_bc.shape[0], X_res.shape[0]) != (self.n_ic, self.n_bc, self.B_res):
            raise ValueError(f"batches must hold ({self.n_ic}, {self.n_bc}, {self.B_res}) points")
        for y, n, name in zip(targets, (self.n_ic, self.n_bc, self.B_res), ("u_ic", "u_bc", "r_res")):
            if n and torch.as_tensor(y).numel() != n:
                raise ValueError(f"{name} must hold {n} values: one per point")
        self._explicit = True
        fill_batches(self.fs, (self.B_res, self.n_ic, self.n_bc), (X_ic, X_bc, X_res), targets)

    def coefficient_history(self, steps=None):
        """(steps, 7) tensor: row i holds the coefficients (``COEF_COLUMNS`` order) the i-th step of THIS history buffer
        used, next to ``loss_history()[i]`` (default: all steps taken so far)."""
        return _engine.history_rows(self.fs.coef_hist, steps, self.opt.hist_cap, self.opt.read)

    def coefficients(self):
        """The current effective coefficients as a dict over ``COEF_COLUMNS``."""
        return self.operator.coefficients()
