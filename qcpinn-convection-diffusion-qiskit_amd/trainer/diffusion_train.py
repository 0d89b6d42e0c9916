"""``train(model, nIter=10000, batch_size=128, log_NTK=False, update_lam=False)`` — the training
loop of the convection-diffusion DV path with the reference's signature and step semantics
(trainer/diffusion_train.py:8-93):

  per iteration (``epochs + 1`` of them, :52): sample IC (``batch_size//3``), BC1 (``batch_size//3``),
  residual (``batch_size``) points in that RNG order (:34-36); u on BC, u on IC, PDE residual (:40-43);
  ``loss = 2*MSE_res + 4*MSE_bc + 2*MSE_ic`` (:47); backward; ``clip_grad_norm_(1)`` (DV, :85); Adam;
  ``ReduceLROnPlateau.step(loss)``; ``loss_history.append`` (:86-90); log / checkpoint every
  ``print_every`` iterations (:56-79).  ``nIter``, ``log_NTK``, ``update_lam`` are unused, as there.

For a ``DVPDESolver`` the whole iteration is ONE call into ``libqcpinn_hip.so``
(``qc_fused_pinn_residual_step``): forward derivative channels, loss, adjoint sweep, row reduction,
clip + Adam + scheduler all run as HIP kernels on resident batches; the host never reads a value
back except at ``print_every``.  Under ``torch.distributed`` (one process per GPU, backend "nccl" =
RCCL) ``batch_size`` is the GLOBAL batch: every rank takes an equal shard of each of the three
batches, and the flat ``[gradient | 3 loss sums]`` vector is all-reduced once per step before the
(identical, replicated) optimiser update.

Any other model (the reference's duck type) runs the generic torch-autograd loop below.

``dataset=`` (keyword-only, a ``data.tabulated.TabulatedProblem``) trains towards the user's own targets instead of the
analytic ones: a ``DVPDESolver`` through ``qc_fused_pinn_data_step`` (minibatches gathered from the device-resident
dataset, targets read from memory, residual with the zeroth-order term ``c_u u``), any other model through the generic
loop on ``torch.randint`` minibatches of the same dataset and the same residual.  A dataset with a coefficient table
(``dataset.coef_res``: one operator row per residual point, with a cubic term) takes ``qc_fused_pinn_coef_step`` in the
same way; nothing else changes for the caller.

``adaptive=`` (keyword-only, a ``data.tabulated.AdaptiveSampling``, with ``dataset=``) draws the residual batch from the
dataset's residual rows with probability proportional to |res|^power / mean + floor instead of uniformly, the residual
re-evaluated on all rows every ``every`` steps: on the device for a ``DVPDESolver`` (``qc_dataset_scores``,
``qc_adapt_build``, ``qc_fused_pinn_adaptive_step``: still one call per iteration, no host read), with torch ops and
``torch.searchsorted`` on the same integer weights for any other model.

``balance=`` (keyword-only, an ``nn.loss_balance.AdaptiveMultiLoss``, with ``dataset=``) learns the three loss weights on
the device (``qc_fused_pinn_balanced_step``, ``trainer.balanced_train``): ``DVPDESolver`` models only, not together with
``adaptive=`` or ``lbfgs=``.

``causal=`` (keyword-only, a ``data.tabulated.CausalWeighting``, with ``dataset=``) weighs the residual of every time slab
by how well the earlier slabs are fitted, on the device (``qc_fused_pinn_causal_step``, ``trainer.causal_train``):
``DVPDESolver`` models only, not together with ``adaptive=``, ``lbfgs=`` or ``balance=``.

``gradnorm=`` (keyword-only, an ``nn.loss_balance.GradNormWeighting``, with ``dataset=`` or on the analytic problem) weighs
the BC and the IC term from the ratio of this step's per-class gradient statistics, on the device
(``qc_fused_pinn_gradnorm_step``, ``trainer.gradnorm_train``): ``DVPDESolver`` models only, alone.

A dataset with ``d_tt`` (``TabulatedProblem(..., d_tt=)``: the coefficient of u_tt, an equation second order in time over two
space dimensions) takes ``qc_fused_pinn_coef_tt_step``: seven derivative channels, rows of eight coefficients.  ``DVPDESolver``
models with 2 .. 5 qubits, angle encoding, without ``fourier_features`` and ``reupload``; single process; not together with
``adaptive=``, ``lbfgs=``, ``balance=``, ``causal=`` or ``gradnorm=`` (``check_tt`` raises ``ValueError`` with the reason).
"""
from __future__ import annotations

import os
import time

import torch

from ..data.diffusion_dataset import Sampler, box, r, u
from ..hip import engine as _engine
from ..hip import lib as _lib
from ..nn.pde import _grad, diffusion_operator


def fetch_minibatch(sampler, N):
    return sampler.sample(N)


# ---------------------------------------------------------------------------------------------
def _dist_info():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


def shard_count(total: int, world: int, rank: int) -> int:
    """Points of a global batch of ``total`` that rank ``rank`` of ``world`` owns."""
    return total // world + (1 if rank < total % world else 0)


def shard_slice(total: int, world: int, rank: int) -> slice:
    start = sum(shard_count(total, world, r_) for r_ in range(rank))
    return slice(start, start + shard_count(total, world, rank))


def _log_line(model, it, parts, lr, step_time, total_elapsed):
    loss, l_r, l_bc, l_ic = parts
    remaining = model.epochs - it
    model.logger.print(
        "Epoch: %d/%d [%.1f%%] | Loss: %.2e | Loss_res: %.2e | Loss_bcs: %.2e | loss_ics: %.2e | lr: %.2e | "
        "Epoch_time: %.2fs | Total: %.1fs | ETA: %.1fs"
        % (it, model.epochs, 100.0 * it / model.epochs if model.epochs > 0 else 0, loss, l_r, l_bc, l_ic, lr,
           step_time, total_elapsed, step_time * remaining))


# --------------------------------------------------------------------------------------------- shared by the trainers
def opt_state_from_torch(params, optimizer, scheduler, device, capacity, max_norm, loss_weights):
    """The device optimiser state over ``params`` (in the flat vector's order), continued from the torch Adam /
    ReduceLROnPlateau objects: hyper-parameters of the first param group, the moments of every parameter that has them."""
    params = list(params)
    g = optimizer.param_groups[0]
    st = _engine.OptimState(sum(p.numel() for p in params), float(g["lr"]), device, hist_cap=capacity,
                            betas=tuple(g["betas"]), eps=float(g["eps"]), max_norm=max_norm,
                            factor=float(scheduler.factor), patience=int(scheduler.patience),
                            threshold=float(scheduler.threshold), min_lr=float(scheduler.min_lrs[0]),
                            sched_eps=float(scheduler.eps), loss_weights=loss_weights)
    steps, off = 0, 0
    for p in params:
        s = optimizer.state.get(p, None)
        k = p.numel()
        if s:
            st.m[off:off + k] = s["exp_avg"].reshape(-1).to(device)
            st.v[off:off + k] = s["exp_avg_sq"].reshape(-1).to(device)
            steps = int(s["step"])
        off += k
    # a model trained before continues its Adam step count; the loss history of THIS run starts at index 0
    st.write(best=float(scheduler.best), num_bad=int(scheduler.num_bad_epochs), step=steps, hist_base=steps)
    return st


def sync_opt_state_to_torch(opt, params, optimizer, scheduler):
    """Mirror the device optimiser record ``opt`` into the torch optimiser / scheduler (``save_state`` calls this through
    the trainers' ``sync_to_torch``): the moments become views of the device state."""
    rec = opt.read()
    off = 0
    for p in params:
        k = p.numel()
        optimizer.state[p] = {"step": torch.tensor(float(rec["step"])),
                              "exp_avg": opt.m[off:off + k].view(p.shape),
                              "exp_avg_sq": opt.v[off:off + k].view(p.shape)}
        off += k
    for g in optimizer.param_groups:
        g["lr"] = rec["lr"]
    scheduler.best, scheduler.num_bad_epochs = rec["best"], rec["num_bad_epochs"]
    scheduler.last_epoch = rec["step"]
    scheduler._last_lr = [rec["lr"]] * len(optimizer.param_groups)


def batch_prologue(model, batch_size, n_ic, n_bc, sampler):
    """(B_res, n_ic, n_bc, device) of a single-process dataset trainer: ``n_ic`` / ``n_bc`` default to ``batch_size // 3``;
    raises for an unknown sampler, negative or all-zero batch sizes, and a model that is not on a GPU."""
    if sampler not in ("device", "torch"):
        raise ValueError("sampler must be 'device' or 'torch'")
    n3 = batch_size // 3
    B_res, n_ic, n_bc = int(batch_size), (n3 if n_ic is None else int(n_ic)), (n3 if n_bc is None else int(n_bc))
    if min(B_res, n_ic, n_bc) < 0 or B_res + n_ic + n_bc == 0:
        raise ValueError("batch sizes must be non-negative and not all zero")
    dev = model._resolve_device(model.device)
    if dev is None or dev.type != "cuda":
        raise _lib.QcError("training a DVPDESolver needs a GPU (HIP kernels, no CPU fallback)")
    return B_res, n_ic, n_bc, dev


def gather_rows(fs, segments, counts, batch_minor=False, coef=None):
    """The "torch" sampler over a resident dataset: ``torch.randint`` rows of ``segments`` = ((X_res, r), (X_ic, u_ic),
    (X_bc, u_bc)), drawn IC -> BC -> residual like the reference's batches, copied into the batches and targets of the step
    ``fs``.  ``counts`` = (B_res, n_ic, n_bc); ``batch_minor``: target rows [N, w] go into [w, B] targets (absent rows:
    none copied); ``coef``: the (N_res, 7) operator table whose drawn rows go into ``fs.coef_res``."""
    (Xr, Yr), (Xi, Yi), (Xb, Yb) = segments
    B_res, n_ic, n_bc = counts
    for X, Y, n, dX, dY, o in ((Xi, Yi, n_ic, fs.X_val, fs.target_val, 0), (Xb, Yb, n_bc, fs.X_val, fs.target_val, n_ic),
                               (Xr, Yr, B_res, fs.X_res, fs.target_res, 0)):
        if n:
            idx = torch.randint(0, X.shape[0], (n,), device=dX.device)
            dX[o:o + n] = X[idx]
            if batch_minor and Y is not None:
                dY[:, o:o + n] = Y[idx].t()
            elif Y is not None:
                dY[o:o + n] = Y[idx]
            if coef is not None and dX is fs.X_res:
                fs.coef_res[:, :n] = coef[idx].t()


def fill_batches(fs, counts, points, targets=None, batch_minor=False, coef=None, shard=None):
    """Given batches into the step ``fs``: ``points`` = (X_ic, X_bc, X_res) go to ``X_val[:n_ic]``, ``X_val[n_ic:n_ic + n_bc]``
    and ``X_res[:B_res]`` (``counts`` = (B_res, n_ic, n_bc)), ``targets`` = (y_ic, y_bc, y_res | None) to the matching
    slices of ``target_val`` / ``target_res``: one value per point, or with ``batch_minor`` rows [n, w] into [w, B]
    targets; ``coef``: the (n, 7) operator rows of ``X_res`` into ``fs.coef_res[:, :B_res]``.  ``shard`` = (world, rank):
    the arrays hold GLOBAL batches and this rank takes its ``shard_slice`` of each; None: they hold this step's batches."""
    B_res, n_ic, n_bc = counts
    for k, (n, dX, dY, o) in enumerate(((n_ic, fs.X_val, fs.target_val, 0), (n_bc, fs.X_val, fs.target_val, n_ic),
                                        (B_res, fs.X_res, fs.target_res, 0))):
        if not n:
            continue
        s = slice(None) if shard is None else shard_slice(points[k].shape[0], *shard)
        take = lambda a: torch.as_tensor(a, dtype=torch.float32)[s].to(dX.device)
        dX[o:o + n] = take(points[k])
        if targets is not None and targets[k] is not None:
            if batch_minor:
                dY[:, o:o + n] = take(targets[k]).t()
            else:
                dY[o:o + n] = take(torch.as_tensor(targets[k]).reshape(-1))
        if coef is not None and dX is fs.X_res:
            fs.coef_res[:, :n] = take(coef).t()


class StepTrainer:
    """What every fused trainer shares around its step descriptor ``fs`` and its optimiser record ``opt``: the bridge to
    the torch optimiser over ``_params()``, the end of the constructor, sampling from a resident dataset, ``step()`` and
    the readers of the loss.  A subclass sets ``model``, ``device``, ``optimizer``, ``scheduler``, ``max_norm``,
    ``loss_weights``, ``sampler``, ``dataset``, the batch sizes ``B_res`` / ``n_ic`` / ``n_bc``, ``opt`` and ``fs``."""

    world, _comm = 1, None              # single-process unless the subclass shards its batches (FusedTrainer)
    adaptive, _steps = None, 0          # an AdaptiveSampling and the sampled steps taken under it (FusedTrainer)
    _sampled = True                     # False: a dataset segment is empty behind a non-empty batch, load_batches only
    batch_minor = False                 # target rows [N, w] of the dataset go into [w, B] targets

    def _params(self):
        """The tensors behind the flat vector, in its order."""
        return list(self.model.parameters())

    def _coef_table(self):
        """The dataset's operator table whose rows travel with the residual batch, or None."""
        return getattr(self.dataset, "coef_res", None)

    # -- optimiser state: continue from the torch optimiser / scheduler objects
    def _make_opt_state(self, capacity):
        return opt_state_from_torch(self._params(), self.optimizer, self.scheduler, self.device, capacity, self.max_norm,
                                    self.loss_weights)

    def sync_to_torch(self):
        """Mirror the device optimiser record into the torch optimiser / scheduler so that ``save_state`` writes a
        checkpoint interchangeable with the reference's."""
        sync_opt_state_to_torch(self.opt, self._params(), self.optimizer, self.scheduler)

    def _arm(self, *offsets):
        """The end of every constructor: gate tables from the current parameters, the device sampler seeded once from
        torch's CPU generator (so ``torch.manual_seed`` still controls the run; ``offsets``: ``set_sampler``'s), sampled
        batches until ``load_batches`` says otherwise, and ``save_state``'s way back to the torch optimiser."""
        self.fs.refresh_gates()
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if self.world > 1:                                        # every rank must draw the same seed
            import torch.distributed as dist
            t = torch.tensor([seed], dtype=torch.int64, device=self.device)
            dist.broadcast(t, 0)
            seed = int(t.item())
        self.fs.set_sampler(seed, *offsets)
        self._explicit = False
        self.model._sync_fused_to_torch = self.sync_to_torch

    # -- batches
    def sample(self):
        """Rows of the dataset, drawn with replacement.  With the device sampler this only arms the next ``step()``; the
        "torch" sampler draws ``torch.randint`` rows IC -> BC -> residual and copies them."""
        if not self._sampled:
            raise ValueError("the dataset has an empty segment behind a non-empty batch: use load_batches(...)")
        self._explicit = False
        if self.sampler == "device":
            return
        self._explicit = True
        gather_rows(self.fs, self.dataset.segments(), (self.B_res, self.n_ic, self.n_bc), self.batch_minor, self._coef_table())

    def step(self):
        draw = 0 if self._explicit else _lib.QC_PHASE_SAMPLE
        if self.adaptive is not None:
            # scores of all residual rows and their CDF, enqueued ahead of the step on its stream: nothing is read back
            # (steps on explicit batches draw nothing and do not count towards the cadence)
            if draw:
                if self._steps % self.adaptive.every == 0:
                    self.fs.rescore()
                self._steps += 1
        if self.world == 1 or self._comm is not None:
            self.fs.run(draw | _lib.QC_PHASE_GRADS | _lib.QC_PHASE_UPDATE)
        else:
            import torch.distributed as dist
            self.fs.run(draw | _lib.QC_PHASE_GRADS)
            dist.all_reduce(self.fs.flat_grad)          # one small all-reduce: [grads | L_r, L_bc, L_ic]
            self.fs.run(_lib.QC_PHASE_UPDATE)

    def loss_history(self, steps=None):
        return self.opt.loss_history(steps)

    def losses(self):
        rec = self.opt.read()
        return (rec["loss"], rec["loss_res"], rec["loss_bc"], rec["loss_ic"]), rec["lr"]


class DatasetTrainer(StepTrainer):
    """A single-process trainer on a resident dataset whose step is built over the model's flat buffer and circuit (the
    system, the inverse and the balanced trainer).  The constructor runs, in this order: batch sizes and device
    (``batch_prologue``), the dataset to the device, ``_pack()`` (``flat`` and ``NP``), the circuit, the optimiser record,
    ``_make_step()``, the dataset handed to the step unless a segment is empty behind a non-empty batch, ``_arm()``.  A
    subclass raises its argument errors ahead of it and provides ``_make_step``."""

    def __init__(self, model, batch_size, dataset, n_ic, n_bc, loss_weights, max_norm, capacity, sampler):
        self.B_res, self.n_ic, self.n_bc, dev = batch_prologue(model, batch_size, n_ic, n_bc, sampler)
        self.model, self.device, self.sampler = model, dev, sampler
        self.dataset = dataset.to(dev)
        self.max_norm = max_norm
        self.loss_weights = tuple(float(w) for w in loss_weights)
        self.optimizer, self.scheduler = model.optimizer, model.scheduler
        self._pack()
        self.circuit = model._circuit(dev)
        self.opt = self._make_opt_state(int(capacity))
        self.fs = self._make_step()
        self._sampled = all(n_rows > 0 or n_batch == 0
                            for n_batch, n_rows in zip((self.B_res, self.n_ic, self.n_bc), self.dataset.sizes()))
        if self._sampled:
            self.fs.set_dataset(self.dataset.segments())
        self._arm()

    def _pack(self):
        """The model's own flat buffer (``model.parameters()`` order, the parameters re-pointed at views of it) as
        ``self.flat``, its ``self.NP`` entries."""
        if not self.model._packed_ok() or self.model._flat.device != self.device:
            self.model._pack(self.device)
        self.flat = self.model._flat
        self.NP = self.flat.numel()


# ---------------------------------------------------------------------------------------------
class FusedTrainer(StepTrainer):
    """Device-resident training state of one DVPDESolver: sampler boxes, optimiser record,
    the fused-step descriptor.  ``step()`` = one reference iteration, no host synchronisation.

    ``sampler="device"`` (default) draws the three batches inside the fused call with a counter-based
    Philox generator indexed by the global point index (seeded once from torch's CPU generator, so
    ``torch.manual_seed`` still controls the run); ``sampler="torch"`` uses three ``torch.rand`` calls
    like the reference (IC -> BC -> residual)."""

    tt, coef_cols = False, _lib.QC_COEF_COLS    # a dataset with d_tt: the seven-channel step, operator rows of eight columns

    def __init__(self, model, batch_size: int, capacity: int, sampler: str = "device", *, n_bc: int = None,
                 bc_faces=1, pde: dict = None, n_ic: int = None, loss_weights=(2.0, 4.0, 2.0), max_norm=1.0,
                 optimizer=None, scheduler=None, dataset=None, adaptive=None):
        """``n_bc`` / ``n_ic`` (default ``batch_size // 3`` each): GLOBAL boundary / initial points per step;
        ``bc_faces`` = 4 spreads the boundary points evenly over the faces x=0, x=1, y=0, y=1 (second workload,
        train_hybrid_qpinn.py:689-697), ``"random"`` puts each on a face drawn at random (trainer/train.py:118-135),
        instead of the x=0 face; ``pde`` = {"D", "vx", "vy", "problem"} overrides the engine's operator / targets;
        ``loss_weights`` = (residual, BC, IC) weights of the loss; ``max_norm`` None: no gradient clipping;
        ``optimizer`` / ``scheduler``: the torch objects the device state starts from and is mirrored into (default:
        the model's own).  ``dataset`` (a ``TabulatedProblem``): train towards its targets with its operator
        coefficients; ``sample()`` then arms the device gather from the dataset (``sampler="torch"``: ``torch.randint``
        indices and a copy), every rank holding the whole dataset and gathering its shard by GLOBAL point index.
        ``pde={"problem": 3, ...}`` (optional "coeffs" = (c_t, c_x, c_y, d_xx, d_yy) and "c_u") is the tabulated step
        without a dataset: batches and targets come through ``load_batches(..., targets=)`` only.  A dataset with
        ``coef_res`` (or ``pde={"problem": 3, "coef": True, ...}`` without one) selects the coefficient step: one operator
        row per residual point, gathered with the batch or given through ``load_batches(..., targets=, coef=)``.
        ``adaptive`` (an ``AdaptiveSampling``; needs ``dataset`` and the device sampler): residual rows are drawn in
        proportion to their current residual, rescored on sampled step 0 and then every ``adaptive.every`` sampled steps inside ``step()``
        (enqueued ahead of the step on its stream; every rank scores the whole dataset itself)."""
        # the fused step is the 3-D convection-diffusion step of trainer/diffusion_train.py:30-49 on a (t, x, y) -> u model;
        # the reference fails on any other shape (Linear(3, H) weight mismatch), and so does this trainer: a two-input
        # model keeps a zero-padded t column in W1 that the step would train, a K-output model has K last-layer rows
        if getattr(model, "input_dim", 3) != 3 or getattr(model, "n_out", 1) != 1:
            raise ValueError("train() / FusedTrainer need classic_network = [3, H, 1] (got input_dim = %s, n_out = %s): the "
                             "convection-diffusion step takes (t, x, y) points and one output"
                             % (getattr(model, "input_dim", None), getattr(model, "n_out", None)))
        _check_adaptive(adaptive, dataset, batch_size, sampler)
        self.tt = is_tt(dataset)
        check_tt(model, dataset, _dist_info()[0], **{"adaptive=": adaptive})
        dev = model._resolve_device(model.device)
        if dev is None or dev.type != "cuda":
            raise _lib.QcError("training a DVPDESolver needs a GPU (HIP kernels, no CPU fallback)")
        self.model, self.device = model, dev
        self.eng = model._engine_for(dev)
        self.eng.sigma = (1.0, 1.0, 1.0)          # the trainers call the operator with its default scalings
        self.eng.coeffs = None
        self.eng.loss_weights = self.loss_weights = tuple(float(w) for w in loss_weights)
        # a tabulated step leaves the engine as it found it: the descriptor built below keeps what it needs
        before = (self.eng.problem, self.eng.c_u)
        self.eng.coef_mode = False
        if pde:
            self.eng.D, self.eng.vx, self.eng.vy = float(pde["D"]), float(pde["vx"]), float(pde["vy"])
            self.eng.problem = int(pde["problem"])
            if self.eng.problem == _lib.QC_PROBLEM_TABULATED:
                self.eng.coeffs = tuple(float(c) for c in pde["coeffs"]) if "coeffs" in pde else None
                self.eng.c_u = float(pde.get("c_u", 0.0))
                self.eng.coef_mode = bool(pde.get("coef", False))
        self.dataset = None
        if dataset is not None:
            self.dataset = dataset.to(dev)
            self.eng.problem = _lib.QC_PROBLEM_TABULATED
            self.eng.coeffs, self.eng.c_u = self.dataset.coeffs, self.dataset.c_u
            self.eng.coef_mode = self.dataset.coef_res is not None
        self.coef_mode = self.eng.coef_mode or self.tt
        self.coef_cols = _lib.QC_COEF_TT_COLS if self.tt else _lib.QC_COEF_COLS
        self.tabulated = self.eng.problem == _lib.QC_PROBLEM_TABULATED
        self.optimizer = model.optimizer if optimizer is None else optimizer
        self.scheduler = model.scheduler if scheduler is None else scheduler
        self.max_norm = max_norm
        self.world, self.rank = _dist_info()
        n3 = batch_size // 3
        nb = n3 if n_bc is None else int(n_bc)
        ni = n3 if n_ic is None else int(n_ic)
        if bc_faces not in (1, 4, "random") or (bc_faces == 4 and nb % 4):
            raise ValueError("bc_faces must be 1, 4 (with n_bc divisible by 4) or 'random'")
        self.bc_face_points = nb // 4 if bc_faces == 4 else (_lib.QC_BC_RANDOM_FACE if bc_faces == "random" else 0)
        self.global_counts = (batch_size, ni, nb)                    # residual, IC, BC
        self.B_res = shard_count(batch_size, self.world, self.rank)
        self.n_ic = shard_count(ni, self.world, self.rank)
        self.n_bc = shard_count(nb, self.world, self.rank)
        self.bc_start = shard_slice(nb, self.world, self.rank).start
        self.opt = self._make_opt_state(capacity)
        self.fs = self._make_step()
        if self.tabulated:
            (self.eng.problem, self.eng.c_u), self.eng.coeffs = before, None
        self.eng.coef_mode = False
        if self.dataset is not None:
            for what, n_batch, n_rows in zip(("residual", "initial", "boundary"), self.global_counts, self.dataset.sizes()):
                if n_batch > 0 and n_rows == 0:
                    raise ValueError(f"the dataset's {what} segment is empty but the step takes {n_batch} {what} points")
            self.fs.set_dataset(self.dataset.segments(), self._coef_table())
        self.adaptive = adaptive
        if adaptive is not None:
            self.fs.set_adaptive(adaptive.power, adaptive.floor)
        self.lo = {k: box(k, dev)[0:1] for k in ("ics", "bc1", "dom")}
        self.span = {k: box(k, dev)[1:2] - box(k, dev)[0:1] for k in ("ics", "bc1", "dom")}
        if sampler not in ("device", "torch"):
            raise ValueError("sampler must be 'device' or 'torch'")
        self.sampler = sampler
        self._arm(shard_slice(batch_size, self.world, self.rank).start, shard_slice(ni, self.world, self.rank).start,
                  self.bc_start, self.bc_face_points)
        # QC_DP_COLLECTIVE=rccl: the all-reduce runs INSIDE the library call (qc_comm_*: RCCL on the step's own stream,
        # one host call per step); default: torch.distributed between the two phases
        if self.world > 1 and os.environ.get("QC_DP_COLLECTIVE", "torch") == "rccl":
            self._comm = self._make_comm()
            self.fs.set_comm(self._comm)

    def _make_step(self):
        """The step descriptor over this trainer's batch sizes (the engine holds what the constructor configured)."""
        if self.tt:
            return _engine.FusedStepTT(self.eng, self.B_res, self.n_ic, self.n_bc, self.opt, self.global_counts)
        return self.eng.fused(self.B_res, self.n_ic, self.n_bc, self.opt, self.global_counts)

    def _coef_table(self):
        return self.dataset.coef_tt if self.tt else self.dataset.coef_res

    def _make_comm(self):
        """One library-owned RCCL communicator over the ranks of the default process group (the 128-byte id travels
        through torch.distributed once, at construction)."""
        import ctypes as C
        import torch.distributed as dist
        lib = self.eng.lib
        buf = (C.c_ubyte * 128)()
        if self.rank == 0:
            _lib.check(lib.qc_comm_unique_id(buf), "qc_comm_unique_id")
        t = torch.tensor(list(buf), dtype=torch.uint8, device=self.device)
        dist.broadcast(t, 0)
        raw = bytes(t.cpu().tolist())
        comm = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.qc_comm_create(raw, self.world, self.rank, C.byref(comm)), "qc_comm_create")
        return comm

    def close(self):
        """Destroys the library-owned RCCL communicator (QC_DP_COLLECTIVE=rccl); idempotent."""
        comm, self._comm = getattr(self, "_comm", None), None
        if comm is not None:
            try:
                self.fs.set_comm(None)
                self.eng.lib.qc_comm_destroy(comm)
            except Exception:        # interpreter shutdown: the library may already be gone
                pass

    def __del__(self):
        self.close()

    # -- batches
    def sample(self):
        """IC -> BC -> residual, uniform in the reference's boxes (trainer/diffusion_train.py:9-20,34-36), or rows of the
        dataset.  With the device sampler this only arms the next ``step()``."""
        if self.tabulated:
            if self.dataset is None:
                raise ValueError("a tabulated step without dataset= has nothing to sample from: use load_batches(..., targets=)")
            return super().sample()
        self._explicit = False
        if self.sampler == "device":
            return
        self._explicit = True
        fs, dev = self.fs, self.device
        if self.n_ic:
            fs.X_val[: self.n_ic] = self.lo["ics"] + self.span["ics"] * torch.rand(self.n_ic, 3, device=dev)
        if self.n_bc and self.bc_face_points == _lib.QC_BC_RANDOM_FACE:      # a random face per point, one draw
            pts = torch.rand(self.n_bc, 3, device=dev)
            face = torch.randint(0, 4, (self.n_bc,), device=dev)
            pts[:, 1] = torch.where(face == 0, 0.0, torch.where(face == 1, 1.0, pts[:, 1]))
            pts[:, 2] = torch.where(face == 2, 0.0, torch.where(face == 3, 1.0, pts[:, 2]))
            fs.X_val[self.n_ic: self.n_ic + self.n_bc] = pts
        elif self.n_bc:
            pts = self.lo["bc1"] + self.span["bc1"] * torch.rand(self.n_bc, 3, device=dev)
            if self.bc_face_points:      # faces x=0, x=1, y=0, y=1 by GLOBAL boundary-point index
                pts = torch.rand(self.n_bc, 3, device=dev)
                face = (self.bc_start + torch.arange(self.n_bc, device=dev)) // self.bc_face_points
                pts[:, 1] = torch.where(face == 0, 0.0, torch.where(face == 1, 1.0, pts[:, 1]))
                pts[:, 2] = torch.where(face == 2, 0.0, torch.where(face == 3, 1.0, pts[:, 2]))
            fs.X_val[self.n_ic: self.n_ic + self.n_bc] = pts
        if self.B_res:
            fs.X_res[: self.B_res] = self.lo["dom"] + self.span["dom"] * torch.rand(self.B_res, 3, device=dev)

    def load_batches(self, X_ic, X_bc, X_res, targets=None, coef=None):
        """Use given GLOBAL batches (parity tests): this rank takes its contiguous shard.  ``targets`` =
        (u_ic, u_bc, r_res), one value per point: required by, and only accepted for, a tabulated step.  ``coef``: the
        (B_res, 7) operator rows of ``X_res``: required by, and only accepted for, a coefficient step."""
        if coef is not None and not self.coef_mode:
            raise ValueError("coef needs a coefficient step: a dataset with coef_res, or pde={'problem': 3, 'coef': True, ...}")
        if coef is None and self.coef_mode:
            raise ValueError(f"a coefficient step needs coef=(B_res, {self.coef_cols}) operator rows with its batches")
        if targets is not None and not self.tabulated:
            raise ValueError("targets need a tabulated step: construct the trainer with dataset= or pde={'problem': 3, ...}")
        if targets is None and self.tabulated:
            raise ValueError("a tabulated step needs targets=(u_ic, u_bc, r_res) with its batches")
        if targets is not None and tuple(torch.as_tensor(t).numel() for t in targets) != (X_ic.shape[0], X_bc.shape[0],
                                                                                          X_res.shape[0]):
            raise ValueError("targets=(u_ic, u_bc, r_res) must hold one value per point of (X_ic, X_bc, X_res)")
        if coef is not None and tuple(torch.as_tensor(coef).shape) != (X_res.shape[0], self.coef_cols):
            raise ValueError(f"coef must be ({X_res.shape[0]}, {self.coef_cols}): one operator row per point of X_res")
        self._explicit = True
        fill_batches(self.fs, (self.B_res, self.n_ic, self.n_bc), (X_ic, X_bc, X_res), targets, coef=coef,
                     shard=(self.world, self.rank))

    def dataset_scores(self):
        """The fp32 scores |res_j - r_j| of the dataset's residual rows as of the last rescoring (a device tensor; its
        mean is a held-out residual metric).  Adaptive sampling only."""
        if self.adaptive is None:
            raise ValueError("dataset_scores() needs adaptive= sampling")
        return self.fs.scores

    def adaptive_state(self):
        """{"total", "q_sum", "add", "max_p", "shift"} of the current CDF (reads 64 bytes back)."""
        if self.adaptive is None:
            raise ValueError("adaptive_state() needs adaptive= sampling")
        return self.fs.adaptive_state()


def is_tt(dataset) -> bool:
    """The dataset carries a ``d_tt`` column: its problem is second order in time (the seven-channel step)."""
    return getattr(dataset, "d_tt", None) is not None


def check_tt(model, dataset, world=1, **options):
    """The argument errors of a problem with ``d_tt``, one ``ValueError`` per fault, none of which needs a GPU: ``options``
    names the step variants asked for beside it (``adaptive=...``, ``balance=...``: any that is not None is refused), and
    the model must be one the seven-channel kernels serve."""
    if not is_tt(dataset):
        return
    for name, v in options.items():
        if v is not None:
            raise ValueError(f"{name} is not supported for a problem with d_tt: the seven-channel step "
                             "(qc_fused_pinn_coef_tt_step) has no such form")
    if world > 1:
        raise ValueError("a problem with d_tt trains in a single process: world_size > 1 is not supported")
    if model is None:
        return
    if not (hasattr(model, "_engine_for") and hasattr(model, "quantum_layer")):
        raise ValueError("a problem with d_tt runs in the fused step: it is only supported for DVPDESolver models")
    args = getattr(model, "args", None) or {}
    if args.get("fourier_features"):
        raise ValueError("a problem with d_tt does not take args['fourier_features']: the seven-channel pre stage reads plain inputs")
    if args.get("reupload") or getattr(model.quantum_layer, "reupload", False):
        raise ValueError("a problem with d_tt does not take args['reupload']: the seven-channel circuit stages have no EMBED gates")
    n = int(getattr(model, "num_qubits", 0))
    if not 2 <= n <= 5:
        raise ValueError(f"a problem with d_tt needs 2 .. 5 qubits (the register family of circuit kernels), got {n}")
    if str(getattr(model, "encoding", "angle")).lower().startswith("amp"):
        raise ValueError("a problem with d_tt needs angle encoding")


def _check_adaptive(adaptive, dataset, batch_size, sampler="device"):
    """The argument errors of ``adaptive=``, the same for the fused and the generic loop."""
    if adaptive is None:
        return
    if not hasattr(adaptive, "power") or not hasattr(adaptive, "floor") or not hasattr(adaptive, "every"):
        raise ValueError("adaptive= must be a data.tabulated.AdaptiveSampling")
    if dataset is None:
        raise ValueError("adaptive= samples the residual rows of a dataset: give dataset= too")
    if dataset.sizes()[0] == 0 or batch_size <= 0:
        raise ValueError("adaptive= needs residual points: the dataset's residual segment (or the residual batch) is empty")
    if sampler == "torch":
        raise ValueError("adaptive= draws on the device: it cannot be combined with sampler='torch'")


def check_fused_single(model, what, world):
    """The common tail of the argument checks of ``gradnorm=``, ``causal=`` and ``balance=``: single process (``world``
    = the caller's ``_dist_info()[0]``), a DVPDESolver, classic_network = [3, H, 1]."""
    if world > 1:
        raise ValueError(f"{what}= is single-process: world_size > 1 is not supported")
    if not (hasattr(model, "_engine_for") and hasattr(model, "quantum_layer")):
        raise ValueError(f"{what}= runs in the fused step: it is only supported for DVPDESolver models")
    if getattr(model, "input_dim", 3) != 3 or int(getattr(model, "n_out", 1)) != 1:
        raise ValueError(f"{what}= needs classic_network = [3, H, 1]")


def load_explicit(tr, batch):
    """A step's explicit batch (X_ic, X_bc, X_res[, targets[, coef]]) into a FusedTrainer."""
    tr.load_batches(*batch[:3], targets=batch[3] if len(batch) > 3 else None, coef=batch[4] if len(batch) > 4 else None)


def load_with_targets(tr, batch):
    """A step's explicit batch (X_ic, X_bc, X_res, targets) into a trainer on a dataset."""
    tr.load_batches(*batch[:3], targets=batch[3])


def run_fused_loop(model, tr, banner, batch_size, batches=None, load=load_explicit, extra_line=None, finish=None):
    """The training loop around a constructed fused trainer ``tr`` (``sample`` / ``load_batches``, ``step``, ``losses``,
    ``loss_history``, ``sync_to_torch``): ``model.epochs + 1`` steps on sampled batches or, with ``batches``, on
    ``load(tr, batches[it])``; the log line at iteration 0 and every ``print_every``, followed by ``extra_line(tr)`` if
    given; ``model.loss_history`` extended and ``save_state`` at every later multiple of ``print_every``; ``finish(tr,
    steps)`` (what else is stored on the model) ahead of the copy back to torch.  Returns ``tr``."""
    steps = model.epochs + 1
    t0 = time.time()
    model.logger.print(banner)
    model.logger.print(f"Batch size: {batch_size}")
    pe = model.args["print_every"]
    done = 0
    for it in range(steps):
        if batches is None:
            tr.sample()
        else:
            load(tr, batches[it])
        tr.step()
        if it % pe == 0 or it == 0:
            # the reference logs the loss of iteration `it` BEFORE its optimiser step; the fused step has
            # already applied it, and reports that same pre-update loss
            parts, lr = tr.losses()
            el = time.time() - t0
            _log_line(model, it, parts, lr, el / (it + 1), el)
            if extra_line is not None:
                model.logger.print(extra_line(tr))
            if it > 0 and it % pe == 0:
                hist = tr.loss_history(it + 1)
                model.loss_history.extend(hist[done:])
                done = len(hist)
                model.save_state()
    hist = tr.loss_history(steps)
    model.loss_history.extend(hist[done:])
    if finish is not None:
        finish(tr, steps)
    tr.sync_to_torch()
    total = time.time() - t0
    model.total_training_time += total
    model.logger.print(f"Training completed in {total:.2f} seconds ({total / 60:.2f} minutes)")
    return tr


def _train_fused(model, batch_size, batches=None, dataset=None, adaptive=None, lbfgs=None):
    if lbfgs is not None and adaptive is not None:
        raise ValueError("lbfgs= needs a fixed objective: it cannot be combined with adaptive= sampling")
    tr = FusedTrainer(model, batch_size, capacity=model.epochs + 1, dataset=dataset, adaptive=adaptive)

    def lbfgs_phase(tr, steps):
        # the second phase: L-BFGS evaluations on the batches of the last Adam step (explicit batches) or on a fresh draw;
        # the model is left at the last accepted point and the accepted losses continue the history
        from .lbfgs_train import run_phase
        lb = tr.lbfgs = run_phase(tr, lbfgs)
        model.loss_history.extend(lb.accepted_losses())
        rec = lb.state()
        model.logger.print("L-BFGS: %d evaluations, %d accepted, %d rejected trials, %d resets%s | Loss: %.2e"
                           % (rec["n_eval"], rec["n_iter"], rec["n_rejected"], rec["n_resets"],
                              ", stalled" if rec["stalled"] else "", rec["f0"]))
    return run_fused_loop(model, tr, f"Starting training for {model.epochs} epochs...", batch_size, batches,
                          finish=None if lbfgs is None else lbfgs_phase)


# ---------------------------------------------------------------------------------------------
class _RowSampler:
    """``Sampler`` over one segment of a TabulatedProblem: a ``torch.randint`` minibatch of its rows and targets."""

    def __init__(self, X, y, coef=None):
        self.X, self.y, self.coef = X, y.reshape(-1, 1), coef
        self.rows = None        # the coefficient rows of the last minibatch (residual segment of a coefficient dataset)
        self.cdf = None         # adaptive sampling: the (N,) int64 CDF of the rows' integer weights
        self.idx = None         # the rows of the last minibatch

    def sample(self, N):
        if self.cdf is not None:      # row min{j : cdf_j > t}, t uniform in [0, cdf[-1])
            t = torch.randint(0, int(self.cdf[-1]), (N,))
            idx = torch.searchsorted(self.cdf, t.to(self.cdf.device), right=True).to(self.X.device)
        else:
            idx = torch.randint(0, self.X.shape[0], (N,))
        self.idx = idx
        if self.coef is not None:
            self.rows = self.coef[idx]
        return self.X[idx], self.y[idx]


def tabulated_operator(model, t, x, y, coeffs, c_u, coef=None):
    """(u, c_u u + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy)) of a torch model by autograd.  With ``coef``
    ((N, 7) rows c_u, c_t, c_x, c_y, d_xx, d_yy, c_3 of the N points): the per-point operator with the cubic term
    c_3 u^3 instead; ``coeffs`` and ``c_u`` are then not read."""
    c_3 = 0.0
    if coef is not None:
        c_u, c_t, c_x, c_y, d_xx, d_yy, c_3 = (coef[:, k:k + 1] for k in range(7))
    else:
        c_t, c_x, c_y, d_xx, d_yy = coeffs
    for v in (t, x, y):
        v.requires_grad_(True)
    uu = model(torch.cat((t, x, y), 1))
    u_x, u_y = _grad(uu, x), _grad(uu, y)
    res = c_u * uu + c_t * _grad(uu, t) + c_x * u_x + c_y * u_y - (d_xx * _grad(u_x, x) + d_yy * _grad(u_y, y))
    if coef is not None:
        res = res + c_3 * uu ** 3
    return uu, res


def _rescore_generic(model, dataset, res, adaptive, chunk=65536):
    """Scores |res_j - r_j| of all residual rows of ``dataset`` by torch autograd (no gradient reaches the parameters) and
    the integer CDF of qc_adapt_build on them, left in ``res.cdf``."""
    from ..data.tabulated import adaptive_cdf
    out = []
    for k in range(0, dataset.X_res.shape[0], chunk):
        X = dataset.X_res[k:k + chunk]
        rows = None if dataset.coef_res is None else dataset.coef_res[k:k + chunk]
        with torch.enable_grad():
            _, pr = tabulated_operator(model, X[:, 0:1].clone(), X[:, 1:2].clone(), X[:, 2:3].clone(), dataset.coeffs,
                                       dataset.c_u, rows)
        out.append((pr.detach().reshape(-1) - dataset.r[k:k + chunk]).abs().float())
    res.scores = torch.cat(out)
    res.cdf = adaptive_cdf(res.scores, adaptive.power, adaptive.floor)


def _train_generic(model, batch_size, dataset=None, adaptive=None):
    """The reference algorithm for any duck-typed model, on torch autograd.  With ``dataset``: the same loop on
    torch.randint minibatches of its segments (IC -> BC -> residual) and its operator; with ``adaptive`` the residual
    rows are drawn from the CDF of their residuals, rescored every ``adaptive.every`` iterations."""
    _check_adaptive(adaptive, dataset, batch_size)
    dev = model.device
    if dataset is not None:
        dataset = dataset.to(dev if dev is not None else "cpu")
        for what, n_batch, n_rows in zip(("residual", "initial", "boundary"), (batch_size, batch_size // 3, batch_size // 3),
                                         dataset.sizes()):
            if n_batch > 0 and n_rows == 0:
                raise ValueError(f"the dataset's {what} segment is empty but the step takes {n_batch} {what} points")
        ics, bc1, res = _RowSampler(dataset.X_ic, dataset.u_ic), _RowSampler(dataset.X_bc, dataset.u_bc), \
            _RowSampler(dataset.X_res, dataset.r, dataset.coef_res)
    else:
        ics = Sampler(3, box("ics", dev), u, name="Initial Condition", device=dev)
        bc1 = Sampler(3, box("bc1", dev), u, name="Dirichlet BC1", device=dev)
        res = Sampler(3, box("dom", dev), r, name="Forcing", device=dev)
    t0 = time.time()
    model.logger.print(f"Starting training for {model.epochs} epochs...")
    model.logger.print(f"Batch size: {batch_size}")
    fwd_times = []
    for it in range(model.epochs + 1):
        t_it = time.time()
        if adaptive is not None and it % adaptive.every == 0:
            _rescore_generic(model, dataset, res, adaptive)
        if model.optimizer is not None:
            model.optimizer.zero_grad()
        X_ic, u_ic = fetch_minibatch(ics, batch_size // 3)
        X_bc, u_bc = fetch_minibatch(bc1, batch_size // 3)
        X_rs, r_rs = fetch_minibatch(res, batch_size)
        pred_bc = model.forward(X_bc)
        pred_ic = model.forward(X_ic)
        if dataset is not None:
            _, pred_r = tabulated_operator(model, X_rs[:, 0:1], X_rs[:, 1:2], X_rs[:, 2:3], dataset.coeffs, dataset.c_u,
                                           res.rows)
        else:
            _, pred_r = diffusion_operator(model, X_rs[:, 0:1], X_rs[:, 1:2], X_rs[:, 2:3])
        l_r, l_bc, l_ic = model.loss_fn(pred_r, r_rs), model.loss_fn(pred_bc, u_bc), model.loss_fn(pred_ic, u_ic)
        loss = 2.0 * l_r + 4.0 * l_bc + 2.0 * l_ic
        fwd_times.append(time.time() - t_it)
        if it % model.args["print_every"] == 0 or it == 0 or model.args.get("use_ibm_hardware", False):
            lr = model.optimizer.param_groups[0]["lr"] if model.optimizer else 0.0
            _log_line(model, it, (loss.item(), l_r.item(), l_bc.item(), l_ic.item()), lr,
                      sum(fwd_times) / len(fwd_times), time.time() - t0)
            if it > 0 and it % model.args["print_every"] == 0:
                model.save_state()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=0.1 if model.args["solver"] == "CV" else 1)
        if model.optimizer is not None:
            model.optimizer.step()
        if model.scheduler is not None:
            model.scheduler.step(loss)
        model.loss_history.append(loss.item())
    total = time.time() - t0
    model.logger.print(f"Training completed in {total:.2f} seconds ({total / 60:.2f} minutes)")


def train(model, nIter=10000, batch_size=128, log_NTK=False, update_lam=False, *, batches=None, dataset=None,
          adaptive=None, lbfgs=None, balance=None, causal=None, gradnorm=None):
    """``batches`` (keyword-only, not in the reference): a per-iteration list of
    ``(X_ic, X_bc, X_res)`` tensors to use instead of sampling — for parity tests; with a dataset each entry carries a
    fourth element, the targets ``(u_ic, u_bc, r_res)``.  ``dataset`` (keyword-only): a ``TabulatedProblem`` whose targets
    and operator replace the analytic problem (module docstring).  ``adaptive`` (keyword-only): an ``AdaptiveSampling``
    for the residual rows of ``dataset`` (module docstring).  ``lbfgs`` (keyword-only): a ``trainer.lbfgs_train.LbfgsPhase``,
    that many L-BFGS evaluations on the device behind the Adam epochs (``DVPDESolver`` models only); its accepted losses
    continue ``model.loss_history`` and the model ends at the last accepted point.  ``balance`` (keyword-only): an
    ``nn.loss_balance.AdaptiveMultiLoss`` over ("residual", "bc", "ic"); the three loss weights are then learned on the
    device (``trainer.balanced_train``; needs ``dataset``, ``DVPDESolver`` models only, not with ``adaptive`` or
    ``lbfgs``), and the logged loss is the balanced objective.  ``causal`` (keyword-only): a
    ``data.tabulated.CausalWeighting``; the residual of a late time slab is then held back on the device until the earlier
    slabs are fitted (``trainer.causal_train``; needs ``dataset`` and a batch size that is a multiple of 64 * n_slabs,
    ``DVPDESolver`` models only, not with ``adaptive``, ``lbfgs`` or ``balance``); ``model.causal_history`` receives the
    rows (eps, W, L) of the steps.  ``gradnorm`` (keyword-only): an ``nn.loss_balance.GradNormWeighting``; the BC and the IC
    term are then weighted on the device from the ratio of this step's per-class gradient statistics (Wang, Teng,
    Perdikaris 2021; ``trainer.gradnorm_train``; with ``dataset`` or, without one, on the analytic problem; ``DVPDESolver``
    models only, not with ``adaptive``, ``lbfgs``, ``balance`` or ``causal``; ``batch_size // 3`` must be a multiple of 64);
    ``model.gradnorm_history`` receives the rows (lam_bc, lam_ic, m_r, a_bc, a_ic, lambda-weighted loss, updated) of the
    steps.  ``update_lam`` stays unused: the reference carries the flag of this algorithm without reading it, and it
    switches nothing on here either.  A ``dataset`` with ``d_tt`` (second order in time): module docstring."""
    check_tt(None, dataset, **{"adaptive=": adaptive, "lbfgs=": lbfgs, "balance=": balance, "causal=": causal, "gradnorm=": gradnorm})
    if gradnorm is not None:
        from .gradnorm_train import check_gradnorm, train_gradnorm
        check_gradnorm(model, dataset, gradnorm, batch_size, adaptive, lbfgs, balance, causal)
        train_gradnorm(model, batch_size, batches, dataset, gradnorm)
        return
    if causal is not None:
        from .causal_train import check_causal, train_causal
        check_causal(model, dataset, causal, batch_size, adaptive, lbfgs, balance)
        train_causal(model, batch_size, batches, dataset, causal)
        return
    if balance is not None:
        from .balanced_train import check_balance, train_balanced
        check_balance(model, dataset, balance, adaptive, lbfgs)
        train_balanced(model, batch_size, batches, dataset, balance)
        return
    if lbfgs is not None and not (hasattr(lbfgs, "evals") and hasattr(lbfgs, "options")):
        raise ValueError("lbfgs= must be a trainer.lbfgs_train.LbfgsPhase")
    if hasattr(model, "_engine_for") and hasattr(model, "quantum_layer"):
        _train_fused(model, batch_size, batches, dataset, adaptive, lbfgs)
    else:
        if lbfgs is not None:
            raise ValueError("lbfgs= runs on the device: it is only supported for DVPDESolver models")
        if batches is not None:
            raise ValueError("explicit batches are only supported for DVPDESolver models")
        check_tt(model, dataset)
        _train_generic(model, batch_size, dataset, adaptive)
