"""``train_ensemble(models, batch_size=128, *, pde=None, loss_weights=None)``: M ``DVPDESolver`` models of one architecture
trained together, one launch sequence per step for all of them (``qc_fused_pinn_ensemble_step``).

The reference's own configuration (4 qubits, H = 50, batch_size 64 or 128) is one residual tile and one value tile per
stage: a step is bound by its launches and leaves the chip idle.  Its users train it over seeds, learning rates, loss
weights and operator constants, or as a deep ensemble for an error bar on u; the ensemble step runs those M trainings with
the launches of one.  Member m trains exactly as ``trainer.diffusion_train.train`` trains it alone with the sampler key
``seed + m`` (seed: drawn once from torch's CPU generator, as there).

The members may differ in their initial parameters (``torch.manual_seed``), learning rate and optimiser / scheduler
settings, loss weights and the constants D, v_x, v_y of the operator; they must share the architecture, the gate program
and, where the ansatz uses them, the fixed two-wire unitaries (the ``seed`` key of ``args``).  After training every model
is a normally trained ``DVPDESolver``: parameters, Adam moments, scheduler state and ``loss_history`` are its own.
"""
from __future__ import annotations

import statistics
import time

import numpy as np
import torch

from ..hip import engine as _engine
from ..hip import lib as _lib
from .diffusion_train import opt_state_from_torch, sync_opt_state_to_torch


def member_flat(model) -> torch.Tensor:
    """The model's parameters as one flat vector in ``param_layout`` (= ``model.parameters()``) order, a copy."""
    return torch.cat([p.detach().reshape(-1).to(torch.float32) for p in model.parameters()])


def write_member(model, flat: torch.Tensor) -> None:
    """The inverse of ``member_flat``: the entries of ``flat`` into the model's parameters, in place."""
    off = 0
    with torch.no_grad():
        for p in model.parameters():
            k = p.numel()
            p.copy_(flat[off:off + k].view(p.shape).to(p.device))
            off += k
    if off != flat.numel():
        raise ValueError(f"flat vector has {flat.numel()} entries, the model holds {off}")


def check_members(models) -> None:
    """ValueError unless the models can share one ensemble step: DVPDESolver models with classic_network = [3, H, 1], the
    same hidden width, qubit count, encoding and gate program, no Fourier features, and the same fixed unitaries where
    the program applies them."""
    if len(models) < 1:
        raise ValueError("an ensemble needs at least one model")
    a = models[0]
    for k, b in enumerate(models):
        if not (hasattr(b, "_engine_for") and hasattr(b, "quantum_layer")):
            raise ValueError(f"member {k}: the ensemble step trains DVPDESolver models only")
        if getattr(b, "input_dim", 3) != 3 or int(getattr(b, "n_out", 1)) != 1:
            raise ValueError(f"member {k}: the ensemble step needs classic_network = [3, H, 1]")
        if getattr(b, "n_fourier", 0):
            raise ValueError(f"member {k}: Fourier features have no ensemble step")
        if list(b.classic_network) != list(a.classic_network) or b.num_qubits != a.num_qubits:
            raise ValueError(f"member {k}: architecture {b.classic_network} on {b.num_qubits} qubits differs from member 0's "
                             f"{a.classic_network} on {a.num_qubits}")
        qa, qb = a.quantum_layer, b.quantum_layer
        if qb.encoding != qa.encoding or not np.array_equal(qb.program.rows(), qa.program.rows()):
            raise ValueError(f"member {k}: its circuit (ansatz, layers, encoding) differs from member 0's; the members share "
                             "one gate program")
        if qa.program.use_haar and not np.array_equal(np.asarray(qb._haar), np.asarray(qa._haar)):
            raise ValueError(f"member {k}: its fixed two-wire unitaries (args['seed']) differ from member 0's; the members "
                             "share them")
        if [tuple(p.shape) for p in b.parameters()] != [tuple(p.shape) for p in a.parameters()]:
            raise ValueError(f"member {k}: parameter shapes differ from member 0's")


def _per_member(value, M, default, what):
    """``value`` (None, one setting for all, or a list of M) as a list of M settings."""
    if value is None:
        return [default] * M
    if isinstance(value, (list, tuple)) and any(isinstance(v, (list, tuple, dict)) for v in value):
        if len(value) != M:
            raise ValueError(f"{what}: a list needs one entry per member ({M}), got {len(value)}")
        return [default if v is None else v for v in value]
    return [value] * M


class EnsembleTrainer:
    """Device-resident training state of M models behind one ``EnsembleStep``.

    ``pde``: None, one dict {"D", "vx", "vy"[, "problem"]} or a list of M (None entries: the defaults D = 0.01, v = (1, 1),
    problem 0; the problem id is common to all members).  ``loss_weights``: None, one (residual, BC, IC) triple or a list
    of M.  ``max_norm``: the clip norm, one or M.  ``step_factory``: what builds the step (default ``EnsembleStep``)."""

    def __init__(self, models, batch_size: int, capacity: int, *, pde=None, loss_weights=None, max_norm=1.0, n_ic=None,
                 n_bc=None, step_factory=None):
        models = list(models)
        check_members(models)
        self.models, M = models, len(models)
        self.M = M
        pdes = _per_member(pde, M, None, "pde")
        self.loss_weights = [tuple(float(w) for w in lw) for lw in _per_member(loss_weights, M, (2.0, 4.0, 2.0), "loss_weights")]
        norms = max_norm if isinstance(max_norm, (list, tuple)) else [max_norm] * M
        if len(norms) != M:
            raise ValueError(f"max_norm: a list needs one entry per member ({M})")
        problems = {int(p.get("problem", 0)) if p else 0 for p in pdes}
        if len(problems) != 1 or not problems <= {0, 1, 2}:
            raise ValueError("the members share one analytic problem (0, 1 or 2)")
        problem = problems.pop()
        n3 = batch_size // 3
        self.B_res, self.n_ic, self.n_bc = int(batch_size), (n3 if n_ic is None else int(n_ic)), (n3 if n_bc is None else int(n_bc))
        if min(self.B_res, self.n_ic, self.n_bc) < 1:
            raise ValueError("the ensemble step needs residual, initial and boundary points")
        m0 = models[0]
        if step_factory is None:
            dev = m0._resolve_device(m0.device)
            if dev is None or dev.type != "cuda":
                raise _lib.QcError("training an ensemble of DVPDESolver models needs a GPU (HIP kernels, no CPU fallback)")
            circuit = m0._circuit(dev)
            step_factory = _engine.EnsembleStep
        else:
            dev, circuit = torch.device("cpu"), None
        self.device = dev
        counts = (self.B_res, self.n_ic, self.n_bc)
        self.pdes, self.opts, flats = [], [], []
        for model, p, lw, mn in zip(models, pdes, self.loss_weights, norms):
            D, vx, vy = (float(p[k]) for k in ("D", "vx", "vy")) if p else (0.01, 1.0, 1.0)
            self.pdes.append(_engine._pde_record((D, vx, vy, 1.0, vx, vy, D, D), lw, counts, problem, self.n_ic))
            self.opts.append(opt_state_from_torch(list(model.parameters()), model.optimizer, model.scheduler, dev, capacity,
                                                  mn, lw))
            flats.append(member_flat(model).to(dev))
        self.fs = step_factory(circuit, m0.hidden_width, flats, self.opts, self.pdes, self.B_res, self.n_ic, self.n_bc)
        self.fs.refresh_gates()
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # member m draws with the key seed + m
        self.fs.set_sampler(self.seed)
        self._explicit = False
        for m, model in enumerate(models):
            model._sync_fused_to_torch = lambda m=m: self.sync_member(m)

    # -- batches: drawn on the device inside the step, or given per member
    def load_batches(self, m: int, X_ic, X_bc, X_res) -> None:
        """Explicit batches of member ``m`` (all members need theirs before a ``step``)."""
        Xr, Xv = self.fs.points(m)
        take = lambda a: torch.as_tensor(a, dtype=torch.float32).to(Xr.device)
        Xv[: self.n_ic], Xv[self.n_ic:], Xr[:] = take(X_ic), take(X_bc), take(X_res)
        self._explicit = True

    def sample(self) -> None:
        self._explicit = False

    def step(self) -> None:
        draw = 0 if self._explicit else _lib.QC_PHASE_SAMPLE
        self.fs.run(draw | _lib.QC_PHASE_GRADS | _lib.QC_PHASE_UPDATE)

    # -- readers
    def losses(self):
        """Per member: ((loss, L_r, L_bc, L_ic), lr) of the last step."""
        out = []
        for m in range(self.M):
            rec = self.fs.read(m)
            out.append(((rec["loss"], rec["loss_res"], rec["loss_bc"], rec["loss_ic"]), rec["lr"]))
        return out

    def loss_history(self, m: int, steps=None):
        return self.fs.loss_history(m, steps)

    # -- back to the models
    def sync_member(self, m: int) -> None:
        """Member m's parameters into its model, and its device optimiser record into the model's torch optimiser and
        scheduler (``save_state`` calls this): the moments become views of the stacked state."""
        model = self.models[m]
        write_member(model, self.fs.params[m, : self.fs.NP])
        sync_opt_state_to_torch(self.fs.member(m), list(model.parameters()), model.optimizer, model.scheduler)

    def sync_to_torch(self) -> None:
        for m in range(self.M):
            self.sync_member(m)

    def predict(self, X):
        """(mean, std) of u over the members at the points ``X`` (B, 3): the members' own ``forward``, one after another
        (std: the population standard deviation; zeros for one member)."""
        with torch.no_grad():
            u = torch.stack([model(X) for model in self.models])
        return u.mean(0), u.std(0, unbiased=False)


def train_ensemble(models, batch_size=128, *, pde=None, loss_weights=None):
    """``epochs + 1`` ensemble steps (``models[0].epochs``; the members share it) on device-drawn batches with the reference's
    logging cadence (iteration 0 and every ``print_every``): min / median / max loss over the members.  Writes parameters,
    Adam moments, scheduler state and ``loss_history`` back into every model; returns the ``EnsembleTrainer``."""
    models = list(models)
    check_members(models)
    lead = models[0]
    if any(m.epochs != lead.epochs for m in models):
        raise ValueError("the members share the number of epochs")
    steps = lead.epochs + 1
    tr = EnsembleTrainer(models, batch_size, capacity=steps, pde=pde, loss_weights=loss_weights)
    t0 = time.time()
    lead.logger.print(f"Starting ensemble training of {tr.M} models for {lead.epochs} epochs...")
    lead.logger.print(f"Batch size: {batch_size}")
    pe = lead.args["print_every"]
    for it in range(steps):
        tr.sample()
        tr.step()
        if it % pe == 0 or it == 0:
            loss = [parts[0] for parts, _ in tr.losses()]
            el = time.time() - t0
            lead.logger.print("Epoch: %d/%d | Loss over %d members: min %.2e | median %.2e | max %.2e | Epoch_time: %.2fs | "
                              "Total: %.1fs" % (it, lead.epochs, tr.M, min(loss), statistics.median(loss), max(loss),
                                                el / (it + 1), el))
    for m, model in enumerate(models):
        model.loss_history.extend(tr.loss_history(m, steps))
    tr.sync_to_torch()
    total = time.time() - t0
    for model in models:
        model.total_training_time += total
    lead.logger.print(f"Ensemble training completed in {total:.2f} seconds ({total / 60:.2f} minutes)")
    return tr
