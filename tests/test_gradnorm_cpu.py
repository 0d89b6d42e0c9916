"""The gradient-norm step without a GPU: the record's layout, every argument error of the value object, of the trainer
and of the new entry points, the restatement of tests/gradnorm_reference.py against Algorithm 1 written directly on torch,
and that ``update_lam`` alone switches nothing on."""
import ctypes as C
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gradnorm_reference as GR
from conftest import pkg

NAMES = ("qc_gradnorm_init", "qc_gradnorm_fold", "qc_fused_pinn_gradnorm_step")


# ---- the library
def test_exports_load_and_step_gradnorm_matches_the_header_layout():
    L = pkg("hip.lib")
    lib = L.load()
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(lib, name)
    S = L.QcStepGradnorm
    assert C.sizeof(S) == 48 and L.QC_GRADNORM_STATE_WORDS == 16 and L.QC_GRADNORM_HIST_COLS == 7
    assert (S.alpha.offset, S.lam_max.offset, S.every.offset, S.lam0_bc.offset, S.lam0_ic.offset, S.state_dev.offset,
            S.hist_dev.offset, S.hist_cap.offset) == (0, 4, 8, 12, 16, 24, 32, 40)
    assert (GR.STATE_WORDS, GR.HIST_COLS) == (L.QC_GRADNORM_STATE_WORDS, L.QC_GRADNORM_HIST_COLS)
    assert lib.qc_version() == 4


FAKE = 4096


def _gn(L, **kw):
    g = L.QcStepGradnorm(0.1, 1e4, 10, 1.0, 1.0, FAKE, None, 0)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


NAN, INF = float("nan"), float("inf")
BAD_RECORDS = (dict(state_dev=None), dict(state_dev=FAKE + 2), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=NAN),
               dict(every=0), dict(every=-3), dict(lam_max=0.0), dict(lam_max=INF), dict(lam_max=NAN), dict(lam0_bc=0.0),
               dict(lam0_bc=-1.0), dict(lam0_bc=NAN), dict(lam0_ic=0.0), dict(lam0_ic=INF), dict(hist_cap=-1),
               dict(hist_cap=3, hist_dev=None))


def test_argument_errors_of_the_entry_points_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    ref = lambda s: None if s is None else C.byref(s)
    data = L.QcStepData(FAKE, FAKE, 0.0, FAKE, FAKE, 10, FAKE, FAKE, 10, FAKE, FAKE, 10)
    coef = L.QcStepCoef()
    assert lib.qc_gradnorm_init(None, ref(_gn(L)), None) == -1 and lib.qc_gradnorm_init(FAKE, None, None) == -1
    assert lib.qc_gradnorm_init(FAKE + 1, ref(_gn(L)), None) == -1
    for kw in BAD_RECORDS:
        if "state_dev" not in kw:
            assert lib.qc_gradnorm_init(FAKE, ref(_gn(L, **kw)), None) == -1, kw

    def fold(part=FAKE, rows=6, rows_res=2, rows_ic=2, stride=16, ncols=16, gn=_gn(L), flat=FAKE, cls=None):
        return lib.qc_gradnorm_fold(part, rows, rows_res, rows_ic, stride, ncols, ref(gn), flat, cls, None)
    assert fold(part=None) == -1 and fold(flat=None) == -1 and fold(gn=None) == -1
    assert fold(ncols=3, stride=3) == -1 and fold(stride=15) == -1 and fold(rows=0) == -1 and fold(rows=2 ** 31) == -1
    assert fold(rows_res=-1) == -1 and fold(rows_ic=-1) == -1 and fold(rows_res=7) == -1 and fold(rows_res=4, rows_ic=3) == -1
    for kw in BAD_RECORDS:
        assert fold(gn=_gn(L, **kw)) == -1, kw

    # the step: the record, the communicator and the split of the value batch ahead of everything the descriptor is asked
    def step(d, t=data, cf=None, gn=_gn(L), phases=L.QC_PHASE_GRADS):
        return lib.qc_fused_pinn_gradnorm_step(ref(d), ref(t), ref(cf), ref(gn), phases, None)
    desc = L.QcStepDesc()
    desc.B_res, desc.B_val, desc.n_ic = 128, 128, 64
    assert step(None) == -1 and step(desc, gn=None) == -1
    assert step(desc, t=None, cf=coef) == -1                     # a coefficient table without data
    for kw in BAD_RECORDS:
        assert step(desc, gn=_gn(L, **kw)) == -1, kw
        assert step(desc, t=None, gn=_gn(L, **kw)) == -1, kw
    desc.comm = FAKE
    assert step(desc) == -2 and step(desc, t=None) == -2         # QC_ERR_UNSUPPORTED: a communicator
    desc.comm = None
    for n_ic, B_val in ((21, 42), (63, 64), (65, 130), (1, 2), (-1, 10), (11, 10)):
        desc.n_ic, desc.B_val = n_ic, B_val
        assert step(desc) == -1, (n_ic, B_val)
    desc.n_ic, desc.B_val = 64, 128
    assert step(desc) == -1 and step(desc, t=None) == -1         # an empty descriptor: whatever the underlying step refuses
    assert lib.qc_error_string(-2).decode().startswith("unsupported")


# ---- the value object and the trainer's refusals
@pytest.mark.parametrize("kw", [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=NAN), dict(every=0), dict(every=2.0),
                                dict(every=True), dict(lam_max=0.0), dict(lam_max=INF), dict(init=(1.0,)), dict(init=(0.0, 1.0)),
                                dict(init=(1.0, NAN)), dict(init=3.0)])
def test_gradnorm_weighting_refuses_bad_arguments(kw):
    GW = pkg("nn.loss_balance").GradNormWeighting
    with pytest.raises(ValueError, match="gradient-norm weighting"):
        GW(**kw)


def test_gradnorm_weighting_is_a_plain_value_object():
    GW = pkg("nn.loss_balance").GradNormWeighting
    g = GW()
    assert (g.alpha, g.every, g.lam_max, g.init) == (0.1, 10, 1e4, (1.0, 1.0))
    assert not isinstance(g, torch.nn.Module) and not any(isinstance(v, torch.Tensor) for v in vars(g).values())
    assert "alpha=0.25" in repr(GW(alpha=0.25, every=3, init=(2, 5))) and GW(alpha=0.0).alpha == 0.0 and GW(alpha=1).alpha == 1.0


def test_gradnorm_trainer_and_train_refuse_what_is_out_of_scope(monkeypatch):
    from test_modules_cpu import Log, base_args
    tab, LB = pkg("data.tabulated"), pkg("nn.loss_balance")
    GT = pkg("trainer.gradnorm_train")
    train = pkg("trainer.diffusion_train").train
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    g = torch.Generator().manual_seed(0)
    Xr, Xi, Xb = (torch.rand(m, 3, generator=g) for m in (5, 3, 4))
    r, ui, ub = (torch.rand(m, generator=g) for m in (5, 3, 4))
    ds = tab.TabulatedProblem(Xr, r, Xi, ui, Xb, ub)
    gw = LB.GradNormWeighting()
    with tempfile.TemporaryDirectory() as d:
        model = Solver(base_args(classic_network=[3, 16, 1]), Log(d), device=torch.device("cpu"))
        for call in (lambda **kw: train(model, batch_size=kw.pop("batch", 192), gradnorm=kw.pop("gradnorm", gw), **kw),
                     lambda **kw: GT.GradNormTrainer(model, kw.pop("batch", 192), kw.pop("gradnorm", gw), kw.pop("dataset", None), **kw)):
            with pytest.raises(ValueError, match="GradNormWeighting"):
                call(dataset=ds, gradnorm=0.1)
            with pytest.raises(ValueError, match="system"):
                call(dataset=SimpleNamespace(terms=[]))
            for batch in (128, 64, 100, 193):                     # batch // 3 = 42, 21, 33, 64 + 1 / 3: no multiple of 64
                if batch // 3 % 64:
                    with pytest.raises(ValueError, match="n_ic a multiple of 64"):
                        call(dataset=ds, batch=batch)
                    with pytest.raises(ValueError, match=f"n_ic = {batch // 3}"):
                        call(batch=batch)                          # the analytic problem: the same split, the same error
        with pytest.raises(ValueError, match="n_ic = 21"):
            GT.GradNormTrainer(model, 128, gw, ds, n_ic=21, n_bc=21)
        with pytest.raises(ValueError, match="adaptive="):
            train(model, batch_size=192, dataset=ds, gradnorm=gw, adaptive=tab.AdaptiveSampling())
        with pytest.raises(ValueError, match="lbfgs="):
            train(model, batch_size=192, dataset=ds, gradnorm=gw, lbfgs=pkg("trainer.lbfgs_train").LbfgsPhase(4))
        with pytest.raises(ValueError, match="balance="):
            train(model, batch_size=192, dataset=ds, gradnorm=gw, balance=LB.AdaptiveMultiLoss())
        with pytest.raises(ValueError, match="causal="):
            train(model, batch_size=192, dataset=ds, gradnorm=gw, causal=tab.CausalWeighting(2))
        with pytest.raises(ValueError, match="inverse"):
            GT.check_gradnorm(model, ds, gw, 192, operator=tab.LearnedOperator(learn={"d_xx": 0.01}))
        wide = SimpleNamespace(_engine_for=None, quantum_layer=None, input_dim=3, n_out=2)
        with pytest.raises(ValueError, match=r"\[3, H, 1\]"):
            GT.check_gradnorm(wide, ds, gw, 192)
        with pytest.raises(ValueError, match="DVPDESolver"):
            GT.check_gradnorm(torch.nn.Linear(3, 1), ds, gw, 192)
        # one class of the value batch alone needs no tile boundary
        GT.check_gradnorm(model, ds, gw, 128, n_ic=21, n_bc=0)
        GT.check_gradnorm(model, ds, gw, 128, n_ic=0, n_bc=21)
        monkeypatch.setattr(GT, "_dist_info", lambda: (2, 0))
        with pytest.raises(ValueError, match="world_size"):
            train(model, batch_size=192, dataset=ds, gradnorm=gw)


def test_update_lam_alone_takes_the_path_it_took_before(monkeypatch):
    """The reference's flag stays unused: with it set and no gradnorm= the fused trainer runs as before, and only gradnorm=
    reaches the gradient-norm trainer (with or without the flag)."""
    DT, GT = pkg("trainer.diffusion_train"), pkg("trainer.gradnorm_train")
    calls = []
    monkeypatch.setattr(DT, "_train_fused", lambda *a: calls.append(("fused", a)))
    monkeypatch.setattr(DT, "_train_generic", lambda *a: calls.append(("generic", a)))
    monkeypatch.setattr(GT, "train_gradnorm", lambda *a: calls.append(("gradnorm", a)))
    monkeypatch.setattr(GT, "check_gradnorm", lambda *a, **k: None)
    fused = SimpleNamespace(_engine_for=None, quantum_layer=None)
    for flag in (False, True):
        calls.clear()
        DT.train(fused, batch_size=192, update_lam=flag)
        DT.train(torch.nn.Linear(3, 1), batch_size=192, update_lam=flag)
        assert [c[0] for c in calls] == ["fused", "generic"] and calls[0][1] == (fused, 192, None, None, None, None)
        calls.clear()
        gw = pkg("nn.loss_balance").GradNormWeighting()
        DT.train(fused, batch_size=192, update_lam=flag, gradnorm=gw)
        assert [c[0] for c in calls] == ["gradnorm"] and calls[0][1] == (fused, 192, None, None, gw)


# ---- the restatement against Algorithm 1 written directly
def test_restatement_equals_algorithm_1_on_a_three_term_toy_loss_exactly():
    """Two parameters, so that the mean of |g| is one commutative addition and every quantity has one evaluation order."""
    alpha, every, steps, lr = 0.3, 3, 25, 0.05
    A = [torch.tensor(a, dtype=torch.float64) for a in ([[3.0, 1.0], [0.5, 2.0]], [[0.2, -0.1], [0.3, 0.05]], [[0.01, 0.02], [-0.03, 0.04]])]
    b = [torch.tensor(v, dtype=torch.float64) for v in ([1.0, -2.0], [0.3, 0.1], [0.5, -0.2])]
    terms = lambda th: [((M @ th - v) ** 2).mean() for M, v in zip(A, b)]      # residual, BC, IC
    theta = torch.tensor([0.7, -0.4], dtype=torch.float64, requires_grad=True)
    th2 = theta.detach().clone()
    rec = GR.Record(alpha=alpha, every=every, lam_max=1e4, init=(1.0, 1.0), dtype=np.float64)
    lam_bc = lam_ic = 1.0
    seen = []
    for it in range(steps):
        # Algorithm 1, directly
        g_r, g_b, g_i = (torch.autograd.grad(t, theta)[0] for t in terms(theta))
        if it % every == 0:
            lam_bc = (1 - alpha) * lam_bc + alpha * (g_r.abs().max() / g_b.abs().mean()).item()
            lam_ic = (1 - alpha) * lam_ic + alpha * (g_r.abs().max() / g_i.abs().mean()).item()
        with torch.no_grad():
            theta -= lr * (g_r + lam_bc * g_b + lam_ic * g_i)
        # the restatement on the same three gradients
        p = th2.clone().requires_grad_(True)
        ts = terms(p)
        G = np.zeros((3, 5))
        for row, t in zip((0, 2, 1), ts):                          # rows: residual, IC, BC
            G[row, :2] = torch.autograd.grad(t, p, retain_graph=True)[0].numpy()
        G[0, 2], G[2, 3], G[1, 4] = (t.item() for t in ts)
        flat = rec.step(G)
        th2 = th2 - lr * torch.from_numpy(flat[:2])
        assert (float(rec.lam_bc), float(rec.lam_ic)) == (lam_bc, lam_ic), it
        assert np.array_equal(flat[2:], [t.item() for t in ts])
        seen.append((lam_bc, lam_ic))
    assert torch.equal(th2, theta.detach())
    h = rec.history()
    assert h.shape == (steps, 7) and h[:, 6].tolist() == [1.0 if it % every == 0 else 0.0 for it in range(steps)]
    assert rec.n_updates == 9 and len(set(seen)) == 9 and max(s[1] for s in seen) > 5.0      # the weights move, and far


def test_restatement_edge_values():
    G = np.zeros((3, 7))
    G[0, :4], G[1, :4], G[2, :4] = [1.0, -4.0, 2.0, 0.5], [0.1, 0.1, -0.2, 0.0], [0.5, 0.5, 0.5, 0.5]
    G[0, 4], G[2, 5], G[1, 6] = 3.0, 2.0, 1.0
    r = GR.Record(alpha=0.5, every=1, lam_max=1e4)
    flat = r.step(G)
    assert r.state()["m_r"] == 4.0 and r.state()["a_bc"] == 0.5 and r.state()["a_ic"] == pytest.approx(0.1)
    assert float(r.lam_bc) == 0.5 + 0.5 * 8.0 and float(r.lam_ic) == pytest.approx(0.5 + 0.5 * 40.0, rel=1e-6)
    assert np.allclose(flat[:4], G[0, :4] + 4.5 * G[2, :4] + float(r.lam_ic) * G[1, :4], rtol=1e-6) and flat[4:].tolist() == [3.0, 2.0, 1.0]
    assert GR.Record(alpha=0.5, every=1, lam_max=3.0).step(G) is not None
    r = GR.Record(alpha=0.5, every=1, lam_max=3.0)
    r.step(G)
    assert (float(r.lam_bc), float(r.lam_ic)) == (3.0, 3.0)                             # clamped
    r = GR.Record(alpha=0.0, every=1)
    assert np.array_equal(r.step(G)[:4], (G[0, :4] + G[2, :4] + G[1, :4]).astype(np.float32)) and float(r.lam_bc) == 1.0
    Z = G.copy()
    Z[2, :4] = 0.0
    r = GR.Record(alpha=0.5, every=1)
    r.step(Z)
    assert float(r.lam_bc) == 1.0 and float(r.lam_ic) > 1.0 and r.state()["hat_bc"] == 0.0     # an all-zero class keeps its weight
    Z = G.copy()
    Z[0, 1] = NAN
    r = GR.Record(alpha=0.5, every=1)
    r.step(Z)
    assert (float(r.lam_bc), float(r.lam_ic)) == (1.0, 1.0) and np.isnan(r.state()["m_r"])   # a NaN keeps both
    r = GR.Record(alpha=0.5, every=1)
    r.step(G, n_ic=0)
    assert float(r.lam_ic) == 1.0 and float(r.lam_bc) == 4.5                                # an empty class keeps its weight
