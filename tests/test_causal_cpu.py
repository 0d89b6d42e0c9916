"""The causal step without a GPU: the float64 replay of tests/causal_reference.py against torch autograd, the host's sort
and slab table, every argument error of the trainer and of the new entry points, the record's layout, and the conditions
the committed replays must meet for the GPU tests to tell right from wrong weights."""
import ctypes as C

import numpy as np
import pytest
import torch

import causal_reference as CR
import tabulated_reference as T
from conftest import pkg
from step_reference import haar_for


# ---- the replay
def test_slab_gradients_combined_equal_autograd_of_the_causal_loss_with_detached_weights():
    ans, n, L, B_res, M, n_ic, n_bc, eps = "cascade", 2, 1, 128, 2, 3, 2, 1.0
    P = int(pkg("circuits").params_per_layer(ans, n))
    flat, X_ic, X_bc, X_res, u_ic, u_bc, r_res = CR.step_case_inputs(ans, n, L, B_res, n_ic, n_bc)
    args = (flat, T.H, n, L * P, (L, P), ans, haar_for(n, 1), *(torch.as_tensor(x).double() for x in (X_ic, X_bc, X_res)),
            u_ic, u_bc, r_res, M)
    rec = CR.slab_gradients(*args)
    g, parts, W = CR.combine(rec, eps)
    want = CR.autograd_gradient(*args, eps)
    assert W[0] == 1.0 and 0.05 < W[1] < 0.9, W
    assert np.abs(g - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # neither all ones nor the weights attached passes: the first by the size of W_1, the second because d W_1 / d L_0 < 0
    unit = CR.combine(rec, eps, unit=True)[0]
    assert np.abs(unit - want).max() > 1e-4 * max(1.0, np.abs(want).max())
    assert parts[0] == pytest.approx(float((W * rec["L"]).mean()), rel=1e-15)


def test_record_arithmetic_weights_and_annealing():
    W32, W = CR.weights([0.5, 0.25, 2.0], 2.0)
    assert np.allclose(W, [1.0, np.exp(-1.0), np.exp(-1.5)], rtol=1e-15) and W32.dtype == np.float32
    assert CR.weights([3.0, 4.0], 0.0)[0].tolist() == [1.0, 1.0]
    assert CR.anneal(1.0, 0, 0.5, 1.5, 100.0, 0.25) == (np.float32(1.5), 1)
    assert CR.anneal(1.0, 3, 0.2, 1.5, 100.0, 0.25) == (np.float32(1.0), 3)
    assert CR.anneal(80.0, 0, 0.5, 1.5, 100.0, 0.25) == (np.float32(100.0), 1)      # capped
    assert CR.anneal(100.0, 1, 0.5, 1.5, 100.0, 0.25) == (np.float32(100.0), 1)     # at the cap: not raised


# ---- the host helper
def _problem(t):
    tab = pkg("data.tabulated")
    t = torch.as_tensor(t, dtype=torch.float32)
    n = t.numel()
    Xr = torch.stack([t, torch.arange(n, dtype=torch.float32), torch.zeros(n)], 1)
    return tab.TabulatedProblem(Xr, torch.arange(n, dtype=torch.float32) * 10, torch.rand(3, 3), torch.rand(3), torch.rand(2, 3),
                                torch.rand(2), c_u=0.7, d_xx=0.02)


def test_causal_weighting_sorts_stably_and_cuts_equal_width_slabs_with_ties_on_an_edge():
    tab = pkg("data.tabulated")
    #       row:  0     1    2    3     4    5    6     7
    t = [1.0, 0.0, 0.5, 0.25, 0.5, 0.75, 0.5, 0.125]
    ds = _problem(t)
    srt, lo = tab.CausalWeighting(2, eps=1.0).stratify(ds)
    # edges 0, 0.5, 1: the three rows AT 0.5 join the upper slab, in their original order (2, 4, 6)
    assert lo.tolist() == [0, 3, 8] and lo.dtype == torch.int64
    assert srt.X_res[:, 1].tolist() == [1, 7, 3, 2, 4, 6, 5, 0]
    assert srt.r.tolist() == [10, 70, 30, 20, 40, 60, 50, 0]
    assert srt.X_res[:, 0].tolist() == sorted(t) and ds.X_res[:, 0].tolist() == t      # a copy: the dataset is untouched
    assert (srt.coeffs, srt.c_u) == (ds.coeffs, ds.c_u) and srt.X_ic is ds.X_ic
    order, want = CR.slab_table(np.asarray(t, dtype=np.float32), 2)
    assert want.tolist() == lo.tolist() and order.tolist() == [1, 7, 3, 2, 4, 6, 5, 0]
    # four slabs of width 0.25: [0, .25) [.25, .5) [.5, .75) [.75, 1]
    assert tab.CausalWeighting(4).stratify(ds)[1].tolist() == [0, 2, 3, 6, 8]
    # a t_range narrower than the data: rows below the first edge join slab 0, rows at or above the last join slab M - 1
    assert tab.CausalWeighting(2, t_range=(0.2, 0.8)).stratify(ds)[1].tolist() == [0, 3, 8]
    with pytest.raises(ValueError, match="hold no residual point"):
        tab.CausalWeighting(2, t_range=(0.0, 4.0)).stratify(ds)
    with pytest.raises(ValueError, match="hold no residual point"):
        tab.CausalWeighting(8).stratify(_problem([0.0, 0.1, 0.9, 1.0]))
    with pytest.raises(ValueError, match="span no time"):
        tab.CausalWeighting(2).stratify(_problem([0.5, 0.5, 0.5]))


@pytest.mark.parametrize("kw", [dict(n_slabs=1), dict(n_slabs=65), dict(n_slabs=2.0), dict(n_slabs=True), dict(eps=-1.0),
                                dict(eps=float("nan")), dict(growth=0.0), dict(growth=float("inf")), dict(eps_max=-2.0),
                                dict(delta=0.0), dict(delta=float("nan")), dict(t_range=(1.0, 1.0)),
                                dict(t_range=(0.0, float("inf")))])
def test_causal_weighting_refuses_bad_arguments(kw):
    tab = pkg("data.tabulated")
    with pytest.raises(ValueError, match="causal weighting"):
        tab.CausalWeighting(**{"n_slabs": 2, **kw})


def test_slab_rule_rows_lie_in_the_slab_of_their_tile():
    (Xr, *_), lo = CR.sorted_dataset(4)
    rows = CR.slab_rows(0, 512, 4, lo, seed=12345, step=3)
    s = CR.slab_of_points(512, 4)
    assert ((rows >= lo[s]) & (rows < lo[s + 1])).all()
    edges = np.linspace(Xr[0, 0], Xr[-1, 0], 5)
    t = Xr[rows, 0]
    assert ((t >= edges[s] - 1e-7) & (t <= edges[s + 1] + 1e-7)).all()
    # a shard at a non-zero offset draws the rows of the whole batch
    assert np.array_equal(CR.slab_rows(256, 128, 4, lo, 12345, 3), rows[256:384])


# ---- the library
def test_exports_load_and_step_causal_matches_the_header_layout():
    L = pkg("hip.lib")
    lib = L.load()
    for name in ("qc_causal_init", "qc_sample_dataset_slabs", "qc_causal_fold", "qc_fused_pinn_causal_step"):
        assert name in L.EXPORTS and hasattr(lib, name)
    S = L.QcStepCausal
    assert C.sizeof(S) == 56 and L.QC_CAUSAL_MAX_SLABS == 64 and L.QC_CAUSAL_HEAD == 4
    assert (S.n_slabs.offset, S.eps0.offset, S.delta.offset, S.slab_lo_dev.offset, S.state_dev.offset, S.hist_dev.offset,
            S.hist_cap.offset) == (0, 4, 16, 24, 32, 40, 48)
    assert lib.qc_version() == 4


FAKE = 4096


def _causal(L, **kw):
    c = L.QcStepCausal(2, 1.0, 1.5, 100.0, 0.25, FAKE, FAKE, None, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


BAD_RECORDS = (dict(n_slabs=1), dict(n_slabs=65), dict(state_dev=None), dict(state_dev=FAKE + 2), dict(eps0=-0.5),
               dict(eps0=float("nan")), dict(eps_growth=0.0), dict(eps_growth=float("inf")), dict(eps_max=0.0),
               dict(eps_max=float("nan")), dict(delta=-1.0), dict(delta=float("inf")), dict(hist_cap=-1),
               dict(hist_cap=3, hist_dev=None))


def test_argument_errors_of_the_entry_points_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    ref = lambda s: None if s is None else C.byref(s)
    data = L.QcStepData(FAKE, FAKE, 0.0, FAKE, FAKE, 10, FAKE, FAKE, 10, FAKE, FAKE, 10)
    # the record's seed
    assert lib.qc_causal_init(None, ref(_causal(L)), None) == -1 and lib.qc_causal_init(FAKE, None, None) == -1
    assert lib.qc_causal_init(FAKE + 1, ref(_causal(L)), None) == -1
    for kw in BAD_RECORDS:
        if "state_dev" not in kw:
            assert lib.qc_causal_init(FAKE, ref(_causal(L, **kw)), None) == -1, kw

    # the gather
    def gather(n_res=128, off_res=0, M=2, lo=FAKE, t=data):
        return lib.qc_sample_dataset_slabs(FAKE, FAKE, n_res, off_res, FAKE, FAKE, 3, 0, 2, 0, ref(t), M, lo, 1, 1, None)
    assert gather(n_res=64) == -1 and gather(n_res=129) == -1 and gather(n_res=192, M=2) == -1      # not a multiple of 64 M
    assert gather(off_res=32) == -1 and gather(off_res=-64) == -1
    assert gather(M=1) == -1 and gather(M=65, n_res=64 * 65) == -1 and gather(lo=None) == -1 and gather(t=None) == -1

    # the fold
    def fold(part=FAKE, rows=6, rows_res=4, stride=16, ncols=16, cz=_causal(L), flat=FAKE):
        return lib.qc_causal_fold(part, rows, rows_res, stride, ncols, ref(cz), flat, None)
    assert fold(part=None) == -1 and fold(flat=None) == -1 and fold(cz=None) == -1
    assert fold(ncols=2, stride=2) == -1 and fold(stride=15) == -1 and fold(rows=0) == -1 and fold(rows=2 ** 31) == -1
    assert fold(rows_res=0) == -1 and fold(rows_res=8) == -1 and fold(rows_res=3) == -1             # 3: no multiple of M = 2
    for kw in BAD_RECORDS:
        assert fold(cz=_causal(L, **kw)) == -1, kw

    # the step: the record, the communicator and the batch's shape ahead of everything the descriptor is asked
    def step(d, t=data, cz=_causal(L), phases=L.QC_PHASE_GRADS):
        return lib.qc_fused_pinn_causal_step(ref(d), ref(t), ref(cz), phases, None)
    desc = L.QcStepDesc()
    desc.B_res = 128
    assert step(None) == -1 and step(desc, t=None) == -1 and step(desc, cz=None) == -1
    for kw in BAD_RECORDS:
        assert step(desc, cz=_causal(L, **kw)) == -1, kw
    desc.comm = FAKE
    assert step(desc) == -2                                       # QC_ERR_UNSUPPORTED: a communicator
    desc.comm = None
    for B in (0, 64, 129, 192):
        desc.B_res = B
        assert step(desc) == -1, B
    desc.B_res, desc.sample_off_res = 128, 32
    assert step(desc) == -1
    desc.sample_off_res = 0
    assert step(desc) == -1                                       # an empty descriptor: whatever the data step refuses
    assert lib.qc_error_string(-2).decode().startswith("unsupported")


# ---- the trainer's refusals
def test_causal_trainer_and_train_refuse_what_is_out_of_scope(monkeypatch):
    import tempfile
    from types import SimpleNamespace

    from test_modules_cpu import Log, base_args
    tab = pkg("data.tabulated")
    CT = pkg("trainer.causal_train")
    train = pkg("trainer.diffusion_train").train
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    g = torch.Generator().manual_seed(0)
    Xr, Xi, Xb = (torch.rand(m, 3, generator=g) for m in (5, 3, 4))
    r, ui, ub = (torch.rand(m, generator=g) for m in (5, 3, 4))
    ds = tab.TabulatedProblem(Xr, r, Xi, ui, Xb, ub)
    cw = tab.CausalWeighting(2)
    with tempfile.TemporaryDirectory() as d:
        model = Solver(base_args(classic_network=[3, 16, 1]), Log(d), device=torch.device("cpu"))
        for call in (lambda **kw: train(model, batch_size=kw.pop("batch", 128), causal=kw.pop("causal", cw), **kw),
                     lambda **kw: CT.CausalTrainer(model, kw.pop("batch", 128), kw.pop("dataset", None), kw.pop("causal", cw), **kw)):
            with pytest.raises(ValueError, match="needs dataset="):
                call()
            with pytest.raises(ValueError, match="coef_res"):
                call(dataset=tab.TabulatedProblem(Xr, r, Xi, ui, Xb, ub, coef_res=torch.zeros(5, 7)))
            with pytest.raises(ValueError, match="CausalWeighting"):
                call(dataset=ds, causal=2)
            for batch in (64, 100, 192, 0):
                with pytest.raises(ValueError, match=r"multiple of 64 \* n_slabs = 128"):
                    call(dataset=ds, batch=batch)
            with pytest.raises(ValueError, match="system"):
                call(dataset=SimpleNamespace(terms=[]))
        with pytest.raises(ValueError, match="adaptive="):
            train(model, batch_size=128, dataset=ds, causal=cw, adaptive=tab.AdaptiveSampling())
        with pytest.raises(ValueError, match="lbfgs="):
            train(model, batch_size=128, dataset=ds, causal=cw, lbfgs=pkg("trainer.lbfgs_train").LbfgsPhase(4))
        with pytest.raises(ValueError, match="balance="):
            train(model, batch_size=128, dataset=ds, causal=cw, balance=pkg("nn.loss_balance").AdaptiveMultiLoss())
        with pytest.raises(ValueError, match="inverse"):
            CT.check_causal(model, ds, cw, 128, operator=tab.LearnedOperator(learn={"d_xx": 0.01}))
        wide = SimpleNamespace(_engine_for=None, quantum_layer=None, input_dim=3, n_out=2)
        with pytest.raises(ValueError, match=r"\[3, H, 1\]"):
            CT.check_causal(wide, ds, cw, 128)
        with pytest.raises(ValueError, match="DVPDESolver"):
            CT.check_causal(torch.nn.Linear(3, 1), ds, cw, 128)
        with pytest.raises(ValueError, match="sampler must be 'device'"):
            CT.CausalTrainer(model, 128, ds, cw, sampler="torch")
        monkeypatch.setattr(CT, "_dist_info", lambda: (2, 0))
        with pytest.raises(ValueError, match="world_size"):
            train(model, batch_size=128, dataset=ds, causal=cw)


# ---- the committed replays: the conditions the issue sets on eps0, delta and the dataset
@pytest.mark.parametrize("config", list(CR.CONFIGS))
@pytest.mark.parametrize("case", list(CR.TRAIN_CASES))
def test_fp64_replay_meets_the_conditions_and_the_unit_control_misses(case, config):
    B_res, M, eps0, growth, eps_max, delta = CR.CONFIGS[config]
    ref, unit = CR.training_reference(case, config), CR.training_reference(case, config, unit=True)
    assert ref["loss"].shape == (CR.STEPS,) and ref["W"].shape == (CR.STEPS, M) and ref["L"].shape == (CR.STEPS, M)
    assert (ref["W"][:, 0] == 1.0).all() and (np.diff(ref["W"], axis=1) <= 0).all()
    assert 0.05 <= ref["W"][0, -1] <= 0.9, ref["W"][0]          # neither "all ones" nor "all zero" passes
    assert ref["raised"].any() and not ref["raised"].all(), ref["raised"]
    assert int(ref["n_raised"][0]) == int(ref["raised"].sum()) and ref["eps"][0] == np.float32(eps0)
    # no decision of the annealing hangs on the last bits: every W_{M-1} is at least 1 % away from delta
    assert (np.abs(ref["W"][:, -1] - delta) > 0.01 * delta).all(), ref["W"][:, -1] - delta
    gap = np.abs(ref["loss"] - unit["loss"]) / (1e-4 * np.maximum(1.0, np.abs(ref["loss"]).max()))
    print(case, config, "loss", ref["loss"], "unit weights", unit["loss"], "gap / tolerance", gap, "W_last", ref["W"][:, -1],
          "eps", ref["eps"], "->", ref["eps_end"])
    assert gap.max() > 1.0
