"""L-BFGS without a GPU: the float64 restatement of the header's rule (tests/lbfgs_reference.py) against torch.optim.LBFGS,
its backtracking mode's invariants, the argument errors and layouts of the four exports, and the argument errors of
LbfgsTrainer / LbfgsPhase on stubs."""
import ctypes as C

import numpy as np
import pytest
import torch

import lbfgs_reference as LR
from conftest import pkg


def _torch_lbfgs(x0, m, lr=1.0):
    p = torch.nn.Parameter(torch.tensor(np.asarray(x0, dtype=np.float64)))
    opt = torch.optim.LBFGS([p], lr=lr, max_iter=1, history_size=m, tolerance_grad=0, tolerance_change=0, line_search_fn=None)
    return p, opt


def test_fixed_mode_equals_torch_lbfgs_on_a_convex_quartic():
    """N = 40, m = 5, 30 calls: one closure call per torch step, parameters equal to 1e-12 after every call."""
    N, m, calls = 40, 5, 30
    fg = LR.quartic(N, seed=1)
    x0 = np.random.default_rng(2).standard_normal(N) * 0.3
    p, opt = _torch_lbfgs(x0, m)
    ref = LR.LbfgsReference(N, m, LR.FIXED)
    x = x0.copy()
    n_closure = [0]

    def closure():
        n_closure[0] += 1
        f, g = fg(p.detach().numpy())
        p.grad = torch.from_numpy(g.copy())
        return torch.tensor(f)

    for k in range(calls):
        f, g = fg(x)
        x = ref.step(x, f, g)
        opt.step(closure)
        assert n_closure[0] == k + 1
        assert np.abs(x - p.detach().numpy()).max() < 1e-12, k
    assert ref.n_pairs == m and ref.n_eval == calls
    f_end, _ = fg(x)
    assert f_end < 1e-3 * fg(x0)[0]                 # the sequence converged: the comparison is not one of noise


def test_fixed_mode_equals_torch_when_a_pair_is_skipped():
    """Gradients from a list (not a function of x), one of them built so that y.s <= 0: torch and the reference both skip
    that pair and agree to 1e-12 on every call."""
    N, m, calls, bad = 12, 6, 14, 5
    rng = np.random.default_rng(3)
    ref = LR.LbfgsReference(N, m, LR.FIXED, lr=0.5)
    x = rng.standard_normal(N)
    x_start = x.copy()
    grads, xs, pairs = [], [], []
    g = rng.standard_normal(N)
    for k in range(calls):
        if k == bad:
            g = ref.g_k - 0.3 * ref.d                # y = -0.3 d, s = t d: y.s < 0
        elif k > 0:
            g = 0.6 * ref.g_k + 0.8 * ref.t * ref.d + 0.05 * rng.standard_normal(N)      # y.s > 0 by a wide margin
        grads.append(g.copy())
        before = ref.n_pairs
        x = ref.step(x, 1.0, g)
        pairs.append((before, ref.n_pairs))
        xs.append(x.copy())
    assert pairs[bad][1] == pairs[bad][0] < m         # the pair of call `bad` was skipped (the ring was not yet full)
    assert pairs[bad - 1][1] == pairs[bad - 1][0] + 1
    p, opt = _torch_lbfgs(x_start, m, lr=0.5)
    k_call = [0]

    def closure():
        p.grad = torch.from_numpy(grads[k_call[0]].copy())
        return torch.tensor(1.0)

    for k in range(calls):
        k_call[0] = k
        opt.step(closure)
        assert np.abs(xs[k] - p.detach().numpy()).max() < 1e-12, k


def test_armijo_mode_decreases_and_backtracks_inside_the_safeguards():
    N, m = 40, 5
    fg = LR.quartic(N, seed=1, cond=200.0)
    x = np.random.default_rng(4).standard_normal(N) * 2.0
    ref = LR.LbfgsReference(N, m, LR.ARMIJO)
    accepted, n_rej = [], 0
    for k in range(60):
        f, g = fg(x)
        t_before, trials = ref.t, ref.ls_trials
        x = ref.step(x, f, g)
        if ref.accepted:
            accepted.append(f)
        else:
            n_rej += 1
            assert trials + 1 == ref.ls_trials
            assert ref.lo * t_before <= ref.t <= ref.hi * t_before
    assert n_rej >= 1 and len(accepted) + n_rej == 60
    assert all(b < a for a, b in zip(accepted, accepted[1:]))
    assert accepted[-1] < 1e-6 * accepted[0]
    assert [r[2] for r in ref.rows].count(1) == len(accepted) == ref.n_iter


def test_armijo_exhaustion_resets_then_stalls():
    """A loss that never decreases: max_ls rejections reset to steepest descent from g_k, max_ls more set stalled, and the
    parameters then stay at x_k."""
    N = 6
    rng = np.random.default_rng(5)
    ref = LR.LbfgsReference(N, 4, LR.ARMIJO, max_ls=3)
    x0 = rng.standard_normal(N)
    g0 = rng.standard_normal(N)
    x = ref.step(x0, 1.0, g0)
    for k in range(3):
        x = ref.step(x, 2.0, g0)
    assert ref.n_resets == 1 and ref.sd_failed == 1 and not ref.stalled and ref.n_rejected == 3
    assert np.allclose(x, x0 - ref.t * g0)
    for k in range(3):
        x = ref.step(x, 2.0, g0)
    assert ref.stalled == 1 and np.array_equal(x, x0)
    x = ref.step(x, 0.5, g0)
    assert np.array_equal(x, x0) and ref.n_eval == 8 and ref.accepted == 0
    ref.restart(False)
    x = ref.step(x, 0.5, g0)
    assert ref.stalled == 0 and ref.accepted == 1 and not np.array_equal(x, x0)


# ---------------------------------------------------------------------------------------------- the C ABI
def _hyper(L, **kw):
    d = dict(history=5, line_search=L.QC_LBFGS_ARMIJO, max_ls=10, lr=1.0, c1=1e-4, shrink_lo=0.1, shrink_hi=0.5, curv_eps=1e-10,
             w_res=2.0, w_bc=4.0, w_ic=2.0)
    d.update(kw)
    return L.QcLbfgsHyper(**d)


def test_hyper_struct_and_workspace_layout():
    L = pkg("hip.lib")
    lib = L.load()
    assert C.sizeof(L.QcLbfgsHyper) == 44                       # 3 int + 8 float
    assert L.QcLbfgsHyper.lr.offset == 12 and L.QcLbfgsHyper.w_res.offset == 32
    assert L.QC_LBFGS_MAX_HISTORY == 32 and (L.QC_LBFGS_FIXED, L.QC_LBFGS_ARMIJO) == (0, 1)
    for NP, m in ((1, 1), (5, 32), (717, 10), (4000, 3)):
        assert lib.qc_lbfgs_workspace_bytes(NP, m) == 4 * (32 + 3 * NP + 2 * m * NP + m + 4 * m * m)
    sizes = [[lib.qc_lbfgs_workspace_bytes(NP, m) for m in range(1, 33)] for NP in (1, 2, 100, 717, 3069, 3070, 100000)]
    for row in sizes:
        assert all(b > a for a, b in zip(row, row[1:]))          # monotone in m
    for a, b in zip(sizes, sizes[1:]):
        assert all(y > x for x, y in zip(a, b))                  # monotone in NP
    assert lib.qc_lbfgs_workspace_bytes(0, 5) == 0 and lib.qc_lbfgs_workspace_bytes(5, 0) == 0
    assert lib.qc_lbfgs_workspace_bytes(5, 33) == 0


def test_argument_errors_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    ok = _hyper(L)
    assert lib.qc_lbfgs_init(None, 10, 5, None) == -1
    assert lib.qc_lbfgs_init(p, 0, 5, None) == -1
    assert lib.qc_lbfgs_init(p, 10, 0, None) == -1
    assert lib.qc_lbfgs_init(p, 10, 33, None) == -1
    assert lib.qc_lbfgs_init(p + 2, 10, 5, None) == -1
    assert lib.qc_lbfgs_restart(None, 0, None) == -1
    assert lib.qc_lbfgs_restart(p + 1, 0, None) == -1

    def step(flat=p, NP=10, prm=p, ws=p, hp=ok, hist_cap=0):
        return lib.qc_lbfgs_step(flat, NP, prm, ws, C.byref(hp) if hp is not None else None, None, hist_cap, None, 0, None, None)

    assert step(flat=None) == -1 and step(prm=None) == -1 and step(ws=None) == -1 and step(hp=None) == -1
    assert step(NP=0) == -1 and step(hist_cap=-1) == -1
    bad = [dict(history=0), dict(history=33), dict(line_search=2), dict(line_search=-1), dict(max_ls=0)]
    for name in ("lr", "c1", "shrink_lo", "shrink_hi", "curv_eps"):
        bad += [{name: 0.0}, {name: -1.0}, {name: float("nan")}, {name: float("inf")}]
    bad += [dict(shrink_lo=0.6, shrink_hi=0.5), dict(shrink_hi=1.0), dict(shrink_hi=1.5), dict(w_res=float("nan"))]
    for kw in bad:
        assert step(hp=_hyper(L, **kw)) == -1, kw


# ---------------------------------------------------------------------------------------------- the trainer's refusals
class _StubTrainer:
    world, adaptive, _explicit, device = 1, None, True, None


def test_lbfgs_trainer_and_phase_argument_errors():
    T = pkg("trainer.lbfgs_train")
    for kw, what in ((dict(history=0), "history"), (dict(history=33), "history"), (dict(line_search="wolfe"), "line_search"),
                     (dict(max_ls=0), "max_ls"), (dict(lr=0.0), "lr"), (dict(c1=float("nan")), "c1"),
                     (dict(shrink_lo=0.7), "shrink_lo"), (dict(shrink_hi=1.0), "shrink_lo"), (dict(curv_eps=-1.0), "curv_eps")):
        with pytest.raises(ValueError, match=what):
            T.LbfgsTrainer(_StubTrainer(), **kw)
    many = _StubTrainer()
    many.world = 2
    with pytest.raises(ValueError, match="one rank"):
        T.LbfgsTrainer(many)
    ada = _StubTrainer()
    ada.adaptive = object()
    with pytest.raises(ValueError, match="adaptive"):
        T.LbfgsTrainer(ada)
    with pytest.raises(ValueError, match="capacity"):
        T.LbfgsTrainer(_StubTrainer(), capacity=-1)
    for kw in (dict(evals=0), dict(evals=2.5), dict(evals=10, new_batch_every=0), dict(evals=10, momentum=0.9)):
        with pytest.raises(ValueError):
            T.LbfgsPhase(**kw)
    ph = T.LbfgsPhase(evals=30, new_batch_every=10, history=7, line_search="fixed", keep_history=True)
    assert (ph.evals, ph.new_batch_every, ph.keep_history, ph.options) == (30, 10, True, {"history": 7, "line_search": "fixed"})


def test_train_refuses_lbfgs_for_other_models_and_other_objects():
    train = pkg("trainer.diffusion_train").train
    T = pkg("trainer.lbfgs_train")

    class Duck(torch.nn.Module):
        pass

    with pytest.raises(ValueError, match="DVPDESolver"):
        train(Duck(), batch_size=12, lbfgs=T.LbfgsPhase(evals=3))
    with pytest.raises(ValueError, match="LbfgsPhase"):
        train(Duck(), batch_size=12, lbfgs=30)
