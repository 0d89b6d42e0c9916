"""The causal step on the GPU, through the C ABI and the trainer: the bits of the slab-stratified gather
(qc_sample_dataset_slabs), the causal fold on random matrices against float64 (qc_causal_fold), the step at eps = 0 against
qc_fused_pinn_data_step bit for bit, six training steps in the register family (merged), its n = 2 end and the lanes
family against the float64 replays of tests/causal_reference.py (loss, weights, annealing; the all-ones control must
miss), one GRADS-only step of the HBM family, and train(model, dataset=, causal=).

Tolerances: histories at the project's 1e-4 x max(1, |ref|); the one-step gradient block by block at 2e-4 x max(1, max |ref
block|) and the loss parts at 1e-4 (tests/test_gpu_tabulated.py); the fold by the error bound of its own summation, stated
at the test."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import causal_reference as CR
import tabulated_reference as T
import tabulated_training as TT
from conftest import pkg
from test_gpu_fullsize import Log
from test_gpu_tabulated import _errors, _load, _model

pytestmark = pytest.mark.gpu


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


# ---- 1. the gather
def _gather_dataset(M, dev, n_rows=300):
    g = np.random.default_rng(100 + M)
    Xr = g.random((n_rows, 3)).astype(np.float32)
    order, lo = CR.slab_table(Xr[:, 0], M)
    Xr = Xr[order]
    rr = np.arange(n_rows, dtype=np.float32)           # the target names the row
    Xi, Xb = g.random((40, 3)).astype(np.float32), g.random((50, 3)).astype(np.float32)
    ui, ub = 1000 + np.arange(40, dtype=np.float32), 2000 + np.arange(50, dtype=np.float32)
    L = pkg("hip.lib")
    keep = [_dev(a, dev) for a in (Xr, rr, Xi, ui, Xb, ub)]
    data = L.QcStepData(None, None, 0.0, keep[0].data_ptr(), keep[1].data_ptr(), n_rows, keep[2].data_ptr(), keep[3].data_ptr(), 40,
                        keep[4].data_ptr(), keep[5].data_ptr(), 50)
    return (Xr, rr), lo, data, keep


@pytest.mark.parametrize("mult", [1, 3])
@pytest.mark.parametrize("M", [2, 5])
def test_slab_gather_bits_slabs_value_batches_and_shards(M, mult, gpu_device):
    L = pkg("hip.lib")
    lib, dev, st = L.load(), gpu_device, _stream(gpu_device)
    (Xr, rr), lo, data, keep = _gather_dataset(M, dev)
    lo_dev = _dev(lo, dev, torch.int64)
    n_res, n_ic, n_bc, seed, step = 64 * M * mult, 21, 23, 0x1234567890ABCDEF, (1 << 33) + 5
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)

    def gather(n, off, slabs=True, off_ic=3, off_bc=7):
        X, tg, Xv, tv = nan(n, 3), nan(n), nan(n_ic + n_bc, 3), nan(n_ic + n_bc)
        if slabs:
            rc = lib.qc_sample_dataset_slabs(X.data_ptr(), tg.data_ptr(), n, off, Xv.data_ptr(), tv.data_ptr(), n_ic, off_ic, n_bc,
                                             off_bc, C.byref(data), M, lo_dev.data_ptr(), seed, step, st)
        else:
            rc = lib.qc_sample_dataset(X.data_ptr(), tg.data_ptr(), n, off, Xv.data_ptr(), tv.data_ptr(), n_ic, off_ic, n_bc,
                                       off_bc, C.byref(data), seed, step, st)
        L.check(rc, "gather")
        torch.cuda.synchronize(dev)
        return [a.cpu().numpy() for a in (X, tg, Xv, tv)]
    X, tg, Xv, tv = gather(n_res, 0)
    rows = CR.slab_rows(0, n_res, M, lo, seed, step)
    assert np.array_equal(tg, rr[rows]) and np.array_equal(X.view(np.uint32), Xr[rows].view(np.uint32))
    # every point of tile tau has t inside slab tau mod M (its rows, and so its t between the slab's edges)
    s = CR.slab_of_points(n_res, M)
    assert ((tg >= lo[s]) & (tg < lo[s + 1])).all()
    edges = torch.linspace(float(Xr[0, 0]), float(Xr[-1, 0]), M + 1, dtype=torch.float64).numpy()
    assert ((X[:, 0] >= edges[s]) & ((X[:, 0] < edges[s + 1]) | (s == M - 1))).all()
    assert len(set(rows.tolist())) > n_res // 4                  # a draw, not one row per slab
    # IC and BC: the uniform gather's, bit for bit
    _, _, Xv_u, tv_u = gather(n_res, 0, slabs=False)
    assert np.array_equal(Xv.view(np.uint32), Xv_u.view(np.uint32)) and np.array_equal(tv, tv_u)
    assert np.array_equal(tv[:n_ic], 1000 + T.dataset_indices(1, 3, n_ic, 40, seed, step))
    # shards at non-zero offsets: the matching rows of a batch that covers them
    whole = CR.slab_rows(0, 64 * M * 4, M, lo, seed, step)
    for off in (64, 64 * M, 64 * (M + 1)):
        Xs, tgs, _, _ = gather(64 * M, off)
        assert np.array_equal(tgs, rr[whole[off:off + 64 * M]]), off
        assert np.array_equal(Xs.view(np.uint32), Xr[whole[off:off + 64 * M]].view(np.uint32))


# ---- 2. the fold
def _causal_rec(L, M, state, eps0=1.0, growth=1.5, eps_max=100.0, delta=0.25, hist=None, lo=None):
    return L.QcStepCausal(M, eps0, growth, eps_max, delta, None if lo is None else lo.data_ptr(), state.data_ptr(),
                          None if hist is None else hist.data_ptr(), 0 if hist is None else hist.shape[0])


@pytest.mark.parametrize("rows_res,M,rows_val", [(2, 2, 0), (10, 2, 3), (10, 5, 1), (2304, 2, 0), (2304, 64, 0), (2304, 2, 40)])
def test_causal_fold_matches_fp64_and_is_bit_reproducible(rows_res, M, rows_val, gpu_device):
    """rows_res = 2304 exceeds the eight-row prefetch of the fold at its hop of 32 x 8 rows: the tail loop runs.
    Bound of column c: (k + 4) 2^-24 sum_r |w_r part[r][c]| with k the longest chain of additions one result passes through,
    ceil(rows / 256) per wave, 8 waves, 32 folded rows; 4 for the roundings of W, of the product and of the two partial sums."""
    L = pkg("hip.lib")
    lib, dev, st = L.load(), gpu_device, _stream(gpu_device)
    rows, ncols, stride = rows_res + rows_val, 70, 75
    g = np.random.default_rng(rows_res * 100 + M)
    part = g.standard_normal((rows, stride)).astype(np.float32)
    part[:rows_res, ncols - 3] = (g.random(rows_res) * 2.0 / rows_res).astype(np.float32)      # L_i around 1
    part[rows_res:, ncols - 3] = 0.0
    eps0 = np.float32(2.0 / M)
    # float64 reference from the float32 inputs
    slab = np.arange(rows_res) % M
    Lref = np.array([M * part[:rows_res, ncols - 3].astype(np.float64)[slab == i].sum() for i in range(M)])
    W32, W = CR.weights(Lref, eps0)
    w_row = np.concatenate([W[slab], np.ones(rows_val)])
    want = (w_row[:, None] * part[:, :ncols].astype(np.float64)).sum(0)
    bound = (math.ceil(rows / 256) + 8 + 32 + 4) * 2.0 ** -24 * (np.abs(w_row[:, None] * part[:, :ncols])).sum(0)

    def run():
        state = torch.full((L.QC_CAUSAL_HEAD + 2 * M,), float("nan"), dtype=torch.float32, device=dev)
        hist = torch.full((2, 1 + 2 * M), float("nan"), dtype=torch.float32, device=dev)
        cz = _causal_rec(L, M, state, eps0=float(eps0), hist=hist)
        L.check(lib.qc_causal_init(state.data_ptr(), C.byref(cz), st), "qc_causal_init")
        p, flat = _dev(part, dev), torch.full((ncols,), float("nan"), dtype=torch.float32, device=dev)
        L.check(lib.qc_causal_fold(p.data_ptr(), rows, rows_res, stride, ncols, C.byref(cz), flat.data_ptr(), st), "qc_causal_fold")
        torch.cuda.synchronize(dev)
        return flat.cpu().numpy(), state.cpu().numpy(), hist.cpu().numpy()
    flat, state, hist = run()
    err = np.abs(flat.astype(np.float64) - want) / bound
    print("rows", rows, "M", M, "largest error / bound", err.max(), "W", W32[[0, -1]], "L", Lref[[0, -1]])
    assert err.max() < 1.0
    assert flat[ncols - 3] == pytest.approx(float((W * Lref).sum() / M), rel=1e-5)      # the folded column is L_r^c
    H = L.QC_CAUSAL_HEAD
    gotW, gotL = state[H:H + M], state[H + M:H + 2 * M]
    assert np.allclose(gotL, Lref, rtol=2.0 ** -22, atol=0) and np.allclose(gotW, W, rtol=2.0 ** -22, atol=0)
    assert gotW[0] == 1.0
    # an all-ones fold misses the bound
    unit = part[:, :ncols].astype(np.float64).sum(0)
    assert (np.abs(unit - want) / bound).max() > 1.0
    # the record: the row of this step, the counters, eps for the next one
    ints = state.view(np.int32)
    eps_next, n_raised = CR.anneal(eps0, 0, gotW[-1], 1.5, 100.0, 0.25)
    assert state[0] == eps_next and ints[1] == n_raised and ints[2] == 1 and ints[3] == 0
    assert hist[0, 0] == eps0 and np.array_equal(hist[0, 1:1 + M], gotW) and np.array_equal(hist[0, 1 + M:], gotL)
    assert np.isnan(hist[1]).all()
    # two runs are bit-identical
    flat2, state2, hist2 = run()
    assert np.array_equal(flat.view(np.uint32), flat2.view(np.uint32)) and np.array_equal(state.view(np.uint32), state2.view(np.uint32))
    assert np.array_equal(hist.view(np.uint32), hist2.view(np.uint32))


# ---- the step through the engine
def _causal_step(eng, B_res, n_ic, n_bc, M, eps, growth=1.5, eps_max=100.0, delta=0.25, capacity=0, hist_cap=0):
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    eng.problem, eng.coeffs, eng.c_u, eng.coef_mode = L.QC_PROBLEM_TABULATED, T.COEFFS, T.C_U, False
    eng.refresh_gates()
    opt = engine.OptimState(eng.NP, 0.005, eng.device, hist_cap=hist_cap)
    return engine.CausalStep(eng, B_res, n_ic, n_bc, opt, M, eps, growth, eps_max, delta, capacity=capacity,
                             counts=(B_res, max(n_ic, 1), max(n_bc, 1)))


def _data_step(eng, B_res, n_ic, n_bc, hist_cap=0):
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    eng.problem, eng.coeffs, eng.c_u, eng.coef_mode = L.QC_PROBLEM_TABULATED, T.COEFFS, T.C_U, False
    eng.refresh_gates()
    return engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, eng.device, hist_cap=hist_cap),
                            (B_res, max(n_ic, 1), max(n_bc, 1)))


# ---- 3. eps = 0 is the data step, bit for bit
@pytest.mark.parametrize("ans,n", [("cascade", 4), ("layered", 6)], ids=["merged_cascade4", "two_stream_layered6"])
def test_eps_zero_equals_the_data_step_bit_for_bit(ans, n, gpu_device):
    L = pkg("hip.lib")
    B_res, M, n_ic, n_bc, steps = 128, 2, 21, 21, 3
    flat, *batch = CR.step_case_inputs(ans, n, 1, B_res, n_ic, n_bc)
    out = []
    for causal in (False, True):
        model, eng = _model(gpu_device, ans, n, 1, "None", flat)
        fs = _causal_step(eng, B_res, n_ic, n_bc, M, 0.0, hist_cap=steps) if causal else _data_step(eng, B_res, n_ic, n_bc, steps)
        _load(fs, *batch)
        grads = []
        for _ in range(steps):
            fs.run(L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE)
            grads.append(fs.flat_grad.cpu().numpy().copy())
        torch.cuda.synchronize(gpu_device)
        out.append((np.array(grads), eng.flat.detach().cpu().numpy().copy(), np.array(fs.opt.loss_history(steps), np.float32), fs))
    (g0, p0, h0, _), (g1, p1, h1, fs) = out
    assert np.isfinite(g0).all() and np.abs(p0 - np.asarray(flat, np.float32)).max() > 0
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32)) and np.array_equal(h0.view(np.uint32), h1.view(np.uint32))
    rec = fs.read_state()
    assert (rec["W"] == 1.0).all() and rec["n_steps"] == steps and (rec["L"] > 0).all()
    assert rec["L"].mean() == pytest.approx(float(fs.opt.read()["loss_res"]), rel=1e-5)


# ---- 4. training against the float64 replay
def _dataset():
    TP = pkg("data.tabulated").TabulatedProblem
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in TT.dataset_arrays())
    c_t, c_x, c_y, d_xx, d_yy = T.COEFFS
    return TP(Xr, rr, Xi, ui, Xb, ub, c_t=c_t, c_x=c_x, c_y=c_y, d_xx=d_xx, d_yy=d_yy, c_u=T.C_U)


def _trainer(gpu_device, tmp_path, case, config):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    CT, tab = pkg("trainer.causal_train"), pkg("data.tabulated")
    ans, n = CR.TRAIN_CASES[case]
    B_res, M, eps0, growth, eps_max, delta = CR.CONFIGS[config]

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(CR.base_args(ans, n, B_res), TmpLog(), device=gpu_device)
    torch.manual_seed(TT.TRAINER_SEED_AT)
    tr = CT.CausalTrainer(model, B_res, _dataset(), tab.CausalWeighting(M, eps=eps0, growth=growth, eps_max=eps_max, delta=delta),
                          capacity=CR.STEPS, n_ic=CR.N_IC, n_bc=CR.N_BC)
    assert tr.fs.desc.sample_seed == TT.trainer_seed()
    return model, tr


@pytest.mark.parametrize("config", list(CR.CONFIGS))
@pytest.mark.parametrize("case", list(CR.TRAIN_CASES))
def test_training_matches_the_fp64_replay_loss_weights_and_annealing(case, config, gpu_device, tmp_path):
    B_res, M, eps0, growth, eps_max, delta = CR.CONFIGS[config]
    model, tr = _trainer(gpu_device, tmp_path, case, config)
    assert np.array_equal(tr.slab_lo.numpy(), CR.sorted_dataset(M)[1])
    batches = []
    for _ in range(CR.STEPS):
        tr.sample()
        tr.step()
        fs = tr.fs
        Xv, tv = fs.X_val.cpu().numpy(), fs.target_val.cpu().numpy()
        batches.append((Xv[:CR.N_IC], Xv[CR.N_IC:CR.N_IC + CR.N_BC], fs.X_res.cpu().numpy()[:B_res], tv[:CR.N_IC],
                        tv[CR.N_IC:CR.N_IC + CR.N_BC], fs.target_res.cpu().numpy()[:B_res]))
    for got, want in zip(batches, CR.expected_batches(config)):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    ref, unit = CR.training_reference(case, config, batches), CR.training_reference(case, config, batches, unit=True)
    got_l = np.array(tr.opt.loss_history())
    hist = tr.causal_history().astype(np.float64)
    assert got_l.shape == (CR.STEPS,) and hist.shape == (CR.STEPS, 1 + 2 * M)
    got_eps, got_W, got_L = hist[:, 0], hist[:, 1:1 + M], hist[:, 1 + M:]
    rel = lambda got, want: float((np.abs(got - want) / (1e-4 * np.maximum(1.0, np.abs(want)))).max())
    err_l = float(np.abs(got_l - ref["loss"]).max() / (1e-4 * max(1.0, np.abs(ref["loss"]).max())))
    err_u = float(np.abs(got_l - unit["loss"]).max() / (1e-4 * max(1.0, np.abs(unit["loss"]).max())))
    print(case, config, "loss", got_l, ref["loss"], "error / tolerance", err_l, "against unit weights", err_u)
    print(case, config, "W error / tolerance", rel(got_W, ref["W"]), "L", rel(got_L, ref["L"]), "W_last", got_W[:, -1], "eps", got_eps)
    assert err_l < 1.0 and rel(got_W, ref["W"]) < 1.0 and rel(got_L, ref["L"]) < 1.0
    assert err_u > 1.0
    assert rel(got_W, np.ones_like(got_W)) > 1.0
    # annealing: eps of every step and at the end, and the count, are the replay's
    assert np.array_equal(hist[:, 0].astype(np.float32), ref["eps"])
    eps_end, n_raised = tr.epsilon()
    assert np.float32(eps_end) == ref["eps_end"][0] and n_raised == int(ref["n_raised"][0]) and 0 < n_raised < CR.STEPS
    assert np.array_equal(tr.causal_weights(), hist[-1, 1:1 + M].astype(np.float32))
    assert np.array_equal(tr.slab_losses(), hist[-1, 1 + M:].astype(np.float32))
    # the logged residual part is L_r^c
    assert tr.losses()[0][1] == pytest.approx(float((got_W[-1] * got_L[-1]).mean()), rel=1e-5)


# ---- 5. the HBM family
def test_hbm_family_one_grads_step_matches_fp64(gpu_device):
    L = pkg("hip.lib")
    ans, n, Lq, B_res, M, n_ic, n_bc = CR.HBM_CASE
    flat, *batch = CR.step_case_inputs(ans, n, Lq, B_res, n_ic, n_bc)
    rec = CR.hbm_reference()
    model, eng = _model(gpu_device, ans, n, Lq, "None", flat)
    fs = _causal_step(eng, B_res, n_ic, n_bc, M, CR.HBM_EPS)
    _load(fs, *batch)
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize(gpu_device)
    got = fs.flat_grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    g, parts, W = CR.combine(rec, CR.HBM_EPS)
    err = _errors(got, g, parts, n, eng.n_theta)
    gu, pu, _ = CR.combine(rec, CR.HBM_EPS, unit=True)
    berr = _errors(got, gu, pu, n, eng.n_theta)
    st = fs.read_state()
    print("hbm", {k: round(float(v), 4) for k, v in err.items()}, "unit weights", {k: round(float(v), 2) for k, v in berr.items()},
          "W", st["W"], W, "L", st["L"], rec["L"])
    assert max(err.values()) < 1.0, err
    assert max(berr.values()) > 1.0 and 0.05 < W[-1] < 0.9
    assert np.abs(st["W"] - W).max() < 1e-4 and (np.abs(st["L"] - rec["L"]) / np.maximum(1.0, rec["L"])).max() < 1e-4
    assert st["n_steps"] == 1
    # a shard whose first tile is global tile 1: the two tiles change slabs (row r belongs to slab (r + 1) mod 2)
    fs.desc.sample_off_res = 64
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize(gpu_device)
    got1 = fs.flat_grad.cpu().numpy().astype(np.float64)
    swapped = dict(rec, g_slab=rec["g_slab"][::-1], L=rec["L"][::-1])
    eps1, raised = CR.anneal(CR.HBM_EPS, 0, st["W"][-1], 1.5, 100.0, 0.25)      # the first call annealed eps for this one
    assert (st["eps"], st["n_raised"]) == (eps1, raised)
    g1, parts1, W1 = CR.combine(swapped, eps1)
    err1, st1 = _errors(got1, g1, parts1, n, eng.n_theta), fs.read_state()
    print("hbm, tile offset 1", {k: round(float(v), 4) for k, v in err1.items()}, "W", st1["W"], W1)
    assert max(err1.values()) < 1.0, err1
    assert max(_errors(got1, g, parts, n, eng.n_theta).values()) > 1.0          # the unshifted weights miss
    assert np.abs(st1["W"] - W1).max() < 1e-4 and np.abs(st1["L"] - swapped["L"]).max() < 1e-4 * max(1.0, swapped["L"].max())
    assert st1["n_steps"] == 2


# ---- 6. train(model, dataset=, causal=)
def test_train_routes_to_the_causal_trainer_and_fills_the_histories(gpu_device, tmp_path):
    trainer, tab = pkg("trainer.diffusion_train"), pkg("data.tabulated")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    lines = []

    class TmpLog(Log):
        def print(self, *a):
            lines.append(" ".join(str(x) for x in a))

        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(dict(CR.base_args("cascade", 4, 128), print_every=2), TmpLog(), device=gpu_device)
    before = [p.detach().clone() for p in model.parameters()]
    trainer.train(model, batch_size=128, dataset=_dataset(), causal=tab.CausalWeighting(2, eps=1.0, growth=1.5, delta=0.25),
                  update_lam=True)
    assert len(model.loss_history) == CR.STEPS and np.isfinite(model.loss_history).all()
    h = model.causal_history
    assert h.shape == (CR.STEPS, 5) and np.isfinite(h).all() and (h[:, 1] == 1.0).all() and (h[:, 2] < 1.0).all()
    assert (h[:, 3:] > 0).all() and h[0, 0] == 1.0 and (np.diff(h[:, 0]) >= 0).all()
    assert any("causal weights" in s for s in lines) and any("time slabs" in s for s in lines)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
