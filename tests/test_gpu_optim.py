"""On-device optimiser block of the step (trainer/diffusion_train.py:81-90; nn/DVPDESolver.py:59-64): gradient
clipping, Adam and ReduceLROnPlateau, including the learning-rate REDUCTION branch the reference reaches in its
20 000-epoch runs (trainer/diffusion_hybrid_trainer.py:46) — compared step by step with torch's own
``clip_grad_norm_`` / ``Adam`` / ``ReduceLROnPlateau`` on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import pkg
from test_gpu_solver import Log, base_args

pytestmark = pytest.mark.gpu


def _loss_sequence(steps, rng):
    """Weighted losses that fall, stall (> patience bad steps in a row, several times) and jitter."""
    base = np.concatenate([np.linspace(3.0, 1.0, 6), np.full(9, 1.0), np.linspace(0.99, 0.8, 5), np.full(steps, 0.8)])[:steps]
    return base * (1.0 + 1e-5 * rng.standard_normal(steps))


@pytest.mark.parametrize("NP", [717, 4000])
def test_adam_clip_plateau_kernels_match_torch(NP, gpu_device):
    """qc_adam_step (k_adam_fast for NP + 3 <= 3072, k_adam beyond) on synthetic gradients: parameters, moments,
    lr, best, num_bad_epochs after EVERY step vs torch.  patience 2, scheduler eps chosen so that the third
    reduction is refused by the ``lr - new_lr <= eps`` guard.  (The fold + update launch of the fused step,
    k_adam_fast<FOLD>, is covered by the training test below.)"""
    L = pkg("hip.lib")
    engine = pkg("hip.engine")
    lib = L.load()
    rng = np.random.default_rng(5)
    steps = 40
    lr0, patience, factor, sched_eps, min_lr = 0.005, 2, 0.9, 4.2e-4, 0.0
    p0 = rng.standard_normal(NP).astype(np.float32)
    losses = _loss_sequence(steps, rng)
    # torch side
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt_t = torch.optim.Adam([pt], lr=lr0)
    sch_t = torch.optim.lr_scheduler.ReduceLROnPlateau(opt_t, mode="min", factor=factor, patience=patience,
                                                       eps=sched_eps, min_lr=min_lr)
    # device side
    prm = torch.from_numpy(p0.copy()).to(gpu_device)
    opt = engine.OptimState(NP, lr0, gpu_device, hist_cap=steps, patience=patience, factor=factor,
                            sched_eps=sched_eps, min_lr=min_lr)
    flat = torch.zeros(NP + 3, device=gpu_device)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    lrs = []
    for k in range(steps):
        scale = 3.0 if k % 3 == 0 else 0.01          # clipped and unclipped steps
        g = (scale * rng.standard_normal(NP)).astype(np.float32)
        l_r, l_bc, l_ic = 0.25 * losses[k], 0.0625 * losses[k], 0.125 * losses[k]   # 2, 4, 2 weights -> losses[k]
        # torch
        opt_t.zero_grad()
        pt.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_([pt], max_norm=1)
        opt_t.step()
        loss_t = torch.tensor(2.0 * np.float32(l_r) + 4.0 * np.float32(l_bc) + 2.0 * np.float32(l_ic))
        sch_t.step(loss_t)
        # device
        vec = np.concatenate([g, np.array([l_r, l_bc, l_ic], np.float32)])
        flat.copy_(torch.from_numpy(vec))
        L.check(lib.qc_adam_step(flat.data_ptr(), NP, prm.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(),
                                 opt.state.data_ptr(), C.byref(opt.hyper), opt.hist.data_ptr(), opt.hist_cap,
                                 None, 0, None, st), "qc_adam_step")
        rec = opt.read()
        lrs.append(rec["lr"])
        assert rec["step"] == k + 1
        assert rec["num_bad_epochs"] == sch_t.num_bad_epochs, (k, rec, sch_t.num_bad_epochs)
        assert abs(rec["lr"] - opt_t.param_groups[0]["lr"]) < 1e-9 + 1e-6 * lr0, (k, rec["lr"], opt_t.param_groups[0]["lr"])
        assert abs(rec["best"] - float(sch_t.best)) < 1e-6 * max(1.0, abs(float(sch_t.best))), (k, rec["best"], sch_t.best)
        assert abs(rec["loss"] - loss_t.item()) < 1e-6 * max(1.0, loss_t.item())
        dp = (prm.cpu() - pt.detach()).abs().max().item()
        assert dp < 2e-6 * (k + 1), (k, dp)
        assert (opt.m.cpu() - opt_t.state[pt]["exp_avg"]).abs().max().item() < 1e-6
        assert (opt.v.cpu() - opt_t.state[pt]["exp_avg_sq"]).abs().max().item() < 1e-6
    # the trajectory really exercised the branches under test
    distinct = sorted(set(round(v, 9) for v in lrs), reverse=True)
    assert len(distinct) == 3, distinct                      # two reductions applied, ...
    assert abs(distinct[-1] - lr0 * factor ** 2) < 1e-8
    assert lr0 * factor ** 2 - lr0 * factor ** 3 <= sched_eps  # ... the third refused by the eps guard
    assert len(opt.loss_history()) == steps


@pytest.mark.parametrize("split", [False, True])
def test_plateau_scheduler_trajectory_in_training_matches_oracle(split, gpu_device, tmp_path):
    """35 fused training steps with patience 2 on fresh batches of 64 points (sampling noise makes the loss
    stall repeatedly): lr / num_bad_epochs / best after every step and the loss history vs the CPU oracle running
    the reference loop with torch's scheduler.  ``split``: the two-call form of the step that data-parallel runs
    use (QC_PHASE_GRADS, [all-reduce], QC_PHASE_UPDATE -> qc_adam_step)."""
    from oracle import solver as osol
    L = pkg("hip.lib")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    trainer = pkg("trainer.diffusion_train")
    steps = 35
    args = base_args(epochs=steps - 1)
    torch.manual_seed(1)
    model = Solver(args, Log(tmp_path), device=gpu_device)
    torch.manual_seed(1)
    ref = osol.OracleSolver(args, device=torch.device("cpu"))
    for m in (model, ref):
        m.scheduler.patience = 2
        m.scheduler.eps = 4.2e-4            # third reduction refused: 0.00405 - 0.003645 <= eps
    torch.manual_seed(11)
    batches = [(osol.sample_box(osol.BOX_IC, 21), osol.sample_box(osol.BOX_BC1, 21), osol.sample_box(osol.BOX_DOM, 64))
               for _ in range(steps)]
    tr = trainer.FusedTrainer(model, 64, capacity=steps)
    lr_seen = set()
    for it in range(steps):
        osol.train_step(ref, 64, batches[it])
        tr.load_batches(*batches[it])
        if split:
            tr.fs.run(L.QC_PHASE_GRADS)
            tr.fs.run(L.QC_PHASE_UPDATE)
        else:
            tr.step()
        rec = tr.opt.read()
        sch = ref.scheduler
        assert rec["num_bad_epochs"] == sch.num_bad_epochs, (it, rec, sch.num_bad_epochs)
        assert abs(rec["lr"] - ref.optimizer.param_groups[0]["lr"]) < 1e-8, (it, rec["lr"])
        assert abs(rec["best"] - float(sch.best)) < 1e-4 * max(1.0, float(sch.best))
        lr_seen.add(round(rec["lr"], 9))
    got, want = np.array(tr.opt.loss_history()), np.array(ref.loss_history)
    assert np.abs(got - want).max() < 1e-4 * max(1.0, np.abs(want).max()), (got, want)
    assert len(lr_seen) >= 2, "no learning-rate reduction happened: the test would not cover the branch"


def test_second_train_call_continues_history_and_optimiser(gpu_device, tmp_path):
    """train() twice on one model: Adam / scheduler state continue (step count, moments), and loss_history is the
    concatenation of both runs — equal to the oracle stepping through all the batches once."""
    from oracle import solver as osol
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    trainer = pkg("trainer.diffusion_train")
    args = base_args(epochs=4)
    torch.manual_seed(1)
    model = Solver(args, Log(tmp_path), device=gpu_device)
    torch.manual_seed(1)
    ref = osol.OracleSolver(args, device=torch.device("cpu"))
    torch.manual_seed(21)
    batches = [(osol.sample_box(osol.BOX_IC, 21), osol.sample_box(osol.BOX_BC1, 21), osol.sample_box(osol.BOX_DOM, 64))
               for _ in range(10)]
    trainer.train(model, batch_size=64, batches=batches[:5])
    assert len(model.loss_history) == 5
    trainer.train(model, batch_size=64, batches=batches[5:])
    for b in batches:
        osol.train_step(ref, 64, b)
    got, want = np.array(model.loss_history), np.array(ref.loss_history)
    assert got.shape == want.shape == (10,)
    assert np.abs(got - want).max() < 1e-4 * max(1.0, np.abs(want).max()), (got, want)
    assert model.scheduler.last_epoch == 10
    assert int(next(iter(model.optimizer.state.values()))["step"]) == 10


# ---- qc_adam_step at its boundaries.  k_adam_fast keeps three elements per thread of one 1024-thread block and serves
# NP + 3 <= 3072: its boundaries sit at 1024, 2048 and 3069 (the last size it serves; k_adam from 3070 on).
SENTINEL = -777.25           # behind every buffer the kernel is handed; must come back bit-unchanged
GUARD, HIST_GUARD = 64, 16


class _PaddedOptim:
    """flat / prm / m / v with GUARD sentinel floats behind their last valid element (NP + 3 for flat, NP for the
    others), a history buffer with HIST_GUARD sentinels behind hist_cap, and one qc_adam_step per ``step``."""

    def __init__(self, NP, p0, device, hist_cap=0, lr=0.005, **opt_kw):
        self.L = pkg("hip.lib")
        self.lib = self.L.load()
        self.NP, self.hist_cap, self.device = NP, hist_cap, device
        self.opt = pkg("hip.engine").OptimState(NP + GUARD, lr, device, hist_cap=0, **opt_kw)     # m, v: NP + GUARD floats
        self.opt.m[NP:] = SENTINEL
        self.opt.v[NP:] = SENTINEL
        self.prm = torch.full((NP + GUARD,), SENTINEL, device=device)
        self.prm[:NP] = torch.from_numpy(np.asarray(p0, dtype=np.float32)).to(device)
        self.flat = torch.full((NP + 3 + GUARD,), SENTINEL, device=device)
        self.hist = torch.full((hist_cap + HIST_GUARD,), SENTINEL, device=device)

    def step(self, g, parts, hist=True):
        NP = self.NP
        vec = np.concatenate([np.asarray(g, dtype=np.float32), np.asarray(parts, dtype=np.float32)])
        self.flat[:NP + 3] = torch.from_numpy(vec).to(self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.qc_adam_step(self.flat.data_ptr(), NP, self.prm.data_ptr(), self.opt.m.data_ptr(), self.opt.v.data_ptr(),
                                   self.opt.state.data_ptr(), C.byref(self.opt.hyper), self.hist.data_ptr() if hist else None,
                                   self.hist_cap, None, 0, None, st)
        torch.cuda.synchronize()
        return rc

    def arrays(self):
        NP = self.NP
        return tuple(t[:n].cpu().numpy() for t, n in ((self.flat, NP + 3), (self.prm, NP), (self.opt.m, NP), (self.opt.v, NP)))

    def assert_guards(self):
        NP = self.NP
        for name, t, n in (("flat", self.flat, NP + 3), ("prm", self.prm, NP), ("m", self.opt.m, NP), ("v", self.opt.v, NP),
                           ("hist", self.hist, self.hist_cap)):
            tail = t[n:].cpu().numpy()
            assert np.array_equal(tail.view(np.int32), np.full(tail.size, SENTINEL, np.float32).view(np.int32)), (name, tail)


def _parts(loss):
    """(L_r, L_bc, L_ic) whose 2, 4, 2 weighted sum is ``loss``."""
    return np.array([0.25 * loss, 0.0625 * loss, 0.125 * loss], np.float32)


def _weighted(parts):
    return torch.tensor(2.0 * np.float32(parts[0]) + 4.0 * np.float32(parts[1]) + 2.0 * np.float32(parts[2]))


BOUNDARY_SIZES = [1, 63, 64, 1021, 1024, 1025, 2047, 2048, 2049, 3068, 3069, 3070, 3072, 3073]


@pytest.mark.parametrize("NP", BOUNDARY_SIZES)
def test_adam_kernels_at_size_boundaries_match_torch(NP, gpu_device):
    """Six steps at every size next to a boundary of the three-elements-per-thread kernel and of the hand-over to
    k_adam, clipped and unclipped gradients alternating, vs torch; nothing beyond NP (NP + 3 for flat) is touched."""
    rng = np.random.default_rng(100 + NP)
    lr0, steps = 0.005, 6
    p0 = rng.standard_normal(NP).astype(np.float32)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt_t = torch.optim.Adam([pt], lr=lr0)
    sch_t = torch.optim.lr_scheduler.ReduceLROnPlateau(opt_t, mode="min", factor=0.9, patience=1)
    dev = _PaddedOptim(NP, p0, gpu_device, hist_cap=steps, lr=lr0, patience=1)
    losses = [2.0, 1.5, 1.5, 1.5, 1.2, 1.2]                                   # one reduction on the way
    for k in range(steps):
        unit = rng.standard_normal(NP)
        unit /= np.linalg.norm(unit)
        g = ((3.0 if k % 2 == 0 else 0.3) * unit).astype(np.float32)          # norm 3 (clipped) / 0.3 (not clipped)
        parts = _parts(losses[k])
        opt_t.zero_grad()
        pt.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_([pt], max_norm=1)
        opt_t.step()
        sch_t.step(_weighted(parts))
        assert dev.step(g, parts) == 0
        dev.assert_guards()
        flat, prm, m, v = dev.arrays()
        rec = dev.opt.read()
        assert rec["step"] == k + 1 and rec["num_bad_epochs"] == sch_t.num_bad_epochs, (k, rec)
        assert abs(rec["lr"] - opt_t.param_groups[0]["lr"]) < 1e-9 + 1e-6 * lr0, (k, rec["lr"])
        assert abs(rec["grad_norm"] - np.linalg.norm(g.astype(np.float64))) < 1e-5
        assert np.abs(prm - pt.detach().numpy()).max() < 2e-6 * (k + 1), k
        assert np.abs(m - opt_t.state[pt]["exp_avg"].numpy()).max() < 1e-6
        assert np.abs(v - opt_t.state[pt]["exp_avg_sq"].numpy()).max() < 1e-6
        assert np.abs(flat[:NP] - pt.grad.numpy()).max() < 1e-6               # the clipped gradient is left in flat
        assert np.array_equal(flat[NP:], parts)
    assert abs(dev.opt.read()["lr"] - 0.9 * lr0) < 1e-8
    assert np.allclose(dev.hist[:steps].cpu().numpy(), losses, rtol=1e-6, atol=0)


@pytest.mark.parametrize("NP", [717, 4000])
def test_adam_zero_gradient_at_step_one_changes_nothing(NP, gpu_device):
    """g = 0 with m = v = 0: 0 / (0 + eps) = 0, so the parameters come back bit-identical; nothing non-finite."""
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(NP).astype(np.float32)
    dev = _PaddedOptim(NP, p0, gpu_device)
    assert dev.step(np.zeros(NP, np.float32), _parts(1.0)) == 0
    dev.assert_guards()
    flat, prm, m, v = dev.arrays()
    assert np.array_equal(prm.view(np.int32), p0.view(np.int32))
    assert not m.any() and not v.any() and not flat[:NP].any()
    rec = dev.opt.read()
    assert rec["grad_norm"] == 0.0 and rec["step"] == 1
    assert all(np.isfinite(x).all() for x in (flat, prm, m, v)) and all(np.isfinite(list(rec.values())))


@pytest.mark.parametrize("NP", [717, 4000])
def test_adam_clip_boundary(NP, gpu_device):
    """max_norm = 1 with gradients of norm 0.999 / 1.0 / 1.001: flat is left as g * min(1, 1 / (norm + 1e-6)).
    The device forms the norm in fp32 from a sum of squares whose longest chain of additions is T (per thread) + 6
    (wave) + 16 (waves) terms.  k_adam (NP = 4000 here) strides 1024 threads over NP: T = ceil(4000 / 1024) = 4, 26 in
    all.  k_adam_fast (NP = 717 here) keeps at most QC_ADAM_K = 3 elements per thread: T <= 3 at any size it serves and 1
    at 717, at most 25.  With 26: relative error <= 13 x 2^-24 after the square root, plus one rounding each for the
    root, the sum with 1e-6, the division and the product, under 20 x 2^-24 in all; the bound below, 32 x 2^-24 |g|,
    covers both kernels.
    At 0.999 the coefficient is 1 whatever the rounding, so flat comes back bit-identical.  With max_norm = None
    (+inf) flat is bit-identical at any norm."""
    rng = np.random.default_rng(4)
    unit = rng.standard_normal(NP)
    unit /= np.linalg.norm(unit)
    for norm in (0.999, 1.0, 1.001):
        g = (norm * unit).astype(np.float32)
        dev = _PaddedOptim(NP, np.zeros(NP, np.float32), gpu_device)
        assert dev.step(g, _parts(1.0)) == 0
        dev.assert_guards()
        flat = dev.arrays()[0][:NP]
        gn = np.linalg.norm(g.astype(np.float64))
        coef = min(1.0, 1.0 / (gn + 1e-6))
        assert (coef < 1.0) == (norm >= 1.0)
        assert np.all(np.abs(flat - g.astype(np.float64) * coef) <= 32 * 2.0 ** -24 * np.abs(g)), norm
        if norm < 1.0:
            assert np.array_equal(flat.view(np.int32), g.view(np.int32))
        else:
            assert np.abs(flat - g).max() > 0.0                    # clipped: even 1 / (1 + 1e-6) differs from 1 in fp32
        assert abs(dev.opt.read()["grad_norm"] - gn) < 2e-6
    g = (30.0 * unit).astype(np.float32)
    dev = _PaddedOptim(NP, np.zeros(NP, np.float32), gpu_device, max_norm=None)
    assert dev.step(g, _parts(1.0)) == 0
    dev.assert_guards()
    assert np.array_equal(dev.arrays()[0][:NP].view(np.int32), g.view(np.int32))
    assert abs(dev.opt.read()["grad_norm"] - 30.0) < 1e-4


@pytest.mark.parametrize("NP", [717, 4000])
def test_adam_late_steps_match_closed_form_and_torch(NP, gpu_device):
    """Steps 20 000 .. 20 002 (the reference trains 20 000 epochs; the bias correction qc_ipow runs its 15 squarings)
    from non-zero moments, vs Adam in closed form in float64 and vs torch with its state at the same step."""
    rng = np.random.default_rng(6)
    lr0, t0, b1, b2, eps = 0.005, 19999, 0.9, 0.999, 1e-8
    lr64 = float(np.float32(lr0))
    p0 = rng.standard_normal(NP).astype(np.float32)
    m0 = (0.1 * rng.standard_normal(NP)).astype(np.float32)
    v0 = (0.02 + 0.01 * rng.random(NP)).astype(np.float32)
    dev = _PaddedOptim(NP, p0, gpu_device, lr=lr0, max_norm=None)
    dev.opt.m[:NP] = torch.from_numpy(m0).to(gpu_device)
    dev.opt.v[:NP] = torch.from_numpy(v0).to(gpu_device)
    dev.opt.write(step=t0)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt_t = torch.optim.Adam([pt], lr=lr0)
    opt_t.state[pt] = {"step": torch.tensor(float(t0)), "exp_avg": torch.from_numpy(m0.copy()),
                       "exp_avg_sq": torch.from_numpy(v0.copy())}
    p, m, v = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    for k in range(3):
        g = (0.15 * rng.standard_normal(NP)).astype(np.float32)
        t = t0 + k + 1
        g64 = g.astype(np.float64)
        m = m + (1.0 - b1) * (g64 - m)
        v = b2 * v + (1.0 - b2) * g64 * g64
        p = p - lr64 / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
        opt_t.zero_grad()
        pt.grad = torch.from_numpy(g.copy())
        opt_t.step()
        assert dev.step(g, _parts(1.0)) == 0
        dev.assert_guards()
        _, prm, dm, dv = dev.arrays()
        assert dev.opt.read()["step"] == t and int(opt_t.state[pt]["step"]) == t
        assert np.isfinite(prm).all()
        assert np.abs(prm - p).max() < 2e-6, (k, np.abs(prm - p).max())
        assert np.abs(dm - m).max() < 1e-6 and np.abs(dv - v).max() < 1e-6
        assert np.abs(prm - pt.detach().numpy()).max() < 2e-6 * (k + 1)
        assert np.abs(dm - opt_t.state[pt]["exp_avg"].numpy()).max() < 1e-6
        assert np.abs(dv - opt_t.state[pt]["exp_avg_sq"].numpy()).max() < 1e-6
    assert np.abs(p - p0).max() > 1e-3                 # the three steps moved the parameters: the check is not vacuous


def _scheduler_run(NP, gpu_device, losses, **sched):
    """qc_adam_step and torch's ReduceLROnPlateau through the same losses: [(lr, num_bad, best)] of both after every step."""
    lr0 = 0.005
    rng = np.random.default_rng(8)
    pt = torch.nn.Parameter(torch.zeros(NP))
    opt_t = torch.optim.Adam([pt], lr=lr0)
    sch_t = torch.optim.lr_scheduler.ReduceLROnPlateau(opt_t, mode="min", factor=sched["factor"], patience=sched["patience"],
                                                       threshold=sched["threshold"], eps=sched["sched_eps"],
                                                       min_lr=sched["min_lr"])
    dev = _PaddedOptim(NP, np.zeros(NP, np.float32), gpu_device, hist_cap=len(losses), lr=lr0, **sched)
    out_dev, out_t = [], []
    for loss in losses:
        parts = _parts(loss)
        sch_t.step(_weighted(parts))
        assert dev.step((0.01 * rng.standard_normal(NP)).astype(np.float32), parts) == 0
        dev.assert_guards()
        rec = dev.opt.read()
        out_dev.append((rec["lr"], rec["num_bad_epochs"], rec["best"]))
        out_t.append((opt_t.param_groups[0]["lr"], sch_t.num_bad_epochs, float(sch_t.best)))
    return out_dev, out_t


@pytest.mark.parametrize("NP", [717, 4000])
def test_plateau_min_lr_clamp_matches_torch(NP, gpu_device):
    """factor 0.5, patience 0, min_lr 0.002 on a constant loss: 0.005 -> 0.0025 -> 0.002 (the fmaxf clamp), then the
    reduction is refused because lr - max(lr * factor, min_lr) = 0 <= eps."""
    lr0 = 0.005
    got, want = _scheduler_run(NP, gpu_device, [1.0] * 7, factor=0.5, patience=0, threshold=1e-4, min_lr=0.002, sched_eps=1e-8)
    for k, ((lr, bad, _), (lr_t, bad_t, _)) in enumerate(zip(got, want)):
        assert abs(lr - lr_t) < 1e-9 + 1e-6 * lr0, (k, lr, lr_t)
        assert bad == bad_t, (k, bad, bad_t)
    lrs = [g[0] for g in got]
    assert np.allclose(lrs, [0.005, 0.0025, 0.002, 0.002, 0.002, 0.002, 0.002], rtol=1e-6, atol=0), lrs
    assert [w[0] for w in want][2] == 0.002                      # torch took the clamp too


@pytest.mark.parametrize("NP", [717, 4000])
def test_plateau_relative_threshold_matches_torch(NP, gpu_device):
    """A loss that improves on ``best`` by half the relative threshold counts as bad, by twice the threshold as good.
    (Away from the boundary itself: torch compares in Python floats, the kernel in fp32.)"""
    thr, best, losses, kinds = 1e-4, 1.0, [1.0], "bbgbggbbbg"
    for kind in kinds:
        loss = best * (1.0 - (0.5 if kind == "b" else 2.0) * thr)
        losses.append(loss)
        best = loss if kind == "g" else best
    got, want = _scheduler_run(NP, gpu_device, losses, factor=0.9, patience=1000, threshold=thr, min_lr=0.0, sched_eps=1e-8)
    bads = [g[1] for g in got]
    assert bads == [w[1] for w in want]
    assert bads == [0, 1, 2, 0, 1, 0, 0, 1, 2, 3, 0], bads
    for (lr, _, b), (lr_t, _, b_t) in zip(got, want):
        assert abs(lr - lr_t) < 1e-9 + 1e-6 * 0.005
        assert abs(b - b_t) < 1e-6 * max(1.0, abs(b_t))


@pytest.mark.parametrize("NP", [717, 4000])
def test_loss_history_window(NP, gpu_device):
    """hist[s - 1 - hist_base] for the (1-based) step s when that index lies in [0, hist_cap), and nowhere else."""
    g = np.full(NP, 0.01, np.float32)
    zeros = np.zeros(NP, np.float32)
    losses = [3.0 - 0.25 * k for k in range(8)]

    def hist(dev):
        return dev.hist[:dev.hist_cap].cpu().numpy()

    # hist_cap = 5 over 8 steps: entries 0..4 hold the first five losses, the rest go nowhere
    dev = _PaddedOptim(NP, zeros, gpu_device, hist_cap=5)
    for loss in losses:
        assert dev.step(g, _parts(loss)) == 0
        dev.assert_guards()
    assert np.allclose(hist(dev), losses[:5], rtol=1e-6, atol=0)
    assert dev.opt.read()["step"] == 8
    # hist_base = 3 with step = 3: the next step writes entry 0
    dev = _PaddedOptim(NP, zeros, gpu_device, hist_cap=5)
    dev.opt.write(step=3, hist_base=3)
    assert dev.step(g, _parts(losses[0])) == 0
    dev.assert_guards()
    h = hist(dev)
    assert np.isclose(h[0], losses[0], rtol=1e-6) and np.all(h[1:] == np.float32(SENTINEL))
    assert dev.opt.read()["hist_base"] == 3 and dev.opt.read()["step"] == 4
    # hist_base = 6 with step = 3: three steps write nothing, the fourth writes entry 0
    dev = _PaddedOptim(NP, zeros, gpu_device, hist_cap=5)
    dev.opt.write(step=3, hist_base=6)
    for k in range(3):
        assert dev.step(g, _parts(losses[k])) == 0
        dev.assert_guards()
        assert np.all(hist(dev) == np.float32(SENTINEL)), k
    assert dev.step(g, _parts(losses[3])) == 0
    dev.assert_guards()
    h = hist(dev)
    assert np.isclose(h[0], losses[3], rtol=1e-6) and np.all(h[1:] == np.float32(SENTINEL))
    # no history buffer at all (NULL with hist_cap > 0): the call succeeds and the record still advances
    dev = _PaddedOptim(NP, zeros, gpu_device, hist_cap=5)
    for k in range(2):
        assert dev.step(g, _parts(losses[k]), hist=False) == 0
        dev.assert_guards()
    rec = dev.opt.read()
    assert rec["step"] == 2 and abs(rec["loss"] - losses[1]) < 1e-6 * losses[1]
    assert np.all(hist(dev) == np.float32(SENTINEL))
