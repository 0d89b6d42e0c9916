"""Residual-adaptive sampling without a GPU: the numpy restatement of include/qcpinn_hip.h's rule
(tests/adaptive_reference.py) draws rows with the frequencies of its weights and never a row of weight zero; its edge
cases; the argument errors of AdaptiveSampling, FusedTrainer and the C entry points; the struct layout; and the generic
torch loop with adaptive=."""
import ctypes as C

import numpy as np
import pytest
import torch

import adaptive_reference as AR
from conftest import pkg
from test_tabulated_cpu import Tiny, _desc

SEED, STEP, OFFSET, DRAWS, ROWS = 0x1234567890ABCDEF, 3, 2 ** 32 - 5, 65536, 64


def _scores():
    e = np.abs(np.random.default_rng(5).standard_normal(ROWS)).astype(np.float32)
    e[7] = 0.0
    e[40] *= 8.0
    return e


# ---- 1. the draw follows the weights
@pytest.mark.parametrize("power,floor", [(1, 1.0), (2, 0.0), (2, 0.25)])
def test_frequencies_follow_the_weights(power, floor):
    """Per row, |count - B w_j / T| <= 5 sigma, sigma^2 = B p_j (1 - p_j).  The cap is derived: for a fair draw a row's
    count is Binomial(B, p_j), and 5 sigma (two-sided tail 6e-7) over the 3 x 64 rows checked here leaves a chance of
    about 1e-4 that a correct sampler fails; the draw is a fixed Philox stream, so the outcome is fixed too."""
    w, rec = AR.weights(_scores(), power, floor)
    _, cdf, _ = AR.build(_scores(), power, floor)
    idx = AR.indices(cdf, OFFSET, DRAWS, SEED, STEP)
    assert idx.min() >= 0 and idx.max() < ROWS
    count = np.bincount(idx, minlength=ROWS).astype(np.float64)
    p = w.astype(np.float64) / float(cdf[-1])
    sigma = np.sqrt(DRAWS * p * (1 - p))
    dev = np.abs(count - DRAWS * p) / np.where(sigma > 0, sigma, 1.0)
    print(power, floor, "largest deviation in sigma:", dev.max())
    assert dev.max() <= 5.0
    assert (count[w == 0] == 0).all()          # zero-weight rows are never drawn
    if floor == 0.0:
        assert w[7] == 0 and count[7] == 0
    else:
        assert w[7] == rec["add"] > 0 and count[7] > 0
    assert count[40] == count.max()


def test_hot_rows_and_flat_spots_are_found():
    for hot in (0, 1024, 2049):
        e = np.zeros(2050, np.float32)
        e[hot] = 2.5
        _, cdf, coarse = AR.build(e, 1, 0.0)
        assert coarse.size == 3 and int(cdf[-1]) == int(coarse[-1])
        assert (AR.indices(cdf, 0, 200, SEED, STEP) == hot).all()
    idx = AR.indices(np.array([1, 1, 2], np.uint64), OFFSET, 4000, SEED, STEP)
    assert set(idx.tolist()) == {0, 2}
    assert abs(int((idx == 0).sum()) - 2000) < 5 * np.sqrt(1000)


# ---- 2. edge cases of the build rule
SIZES = (1, 2, 1023, 1024, 1025, 2 * 1024 + 1)


@pytest.mark.parametrize("N", SIZES)
def test_equal_scores_carry_past_32_bits(N):
    rec, cdf, coarse = AR.build(np.full(N, 3.0, np.float32), 1, 0.25)
    q = 3 << 22          # 3.0 = 1.5 * 2^1 -> s = 22, q = 1.5 * 2^23
    a = int(0.25 * q)
    assert rec == {"q_sum": q * N, "add": a, "max_p": np.float32(3.0), "shift": 22, "total": (q + a) * N}
    assert [int(c) for c in cdf[[0, -1]]] == [q + a, (q + a) * N]
    assert int(coarse[0]) == (q + a) * min(N, 1024) and int(coarse[-1]) == (q + a) * N
    if N >= 1025:
        assert q * N > 2 ** 32


@pytest.mark.parametrize("power", [1, 2, 3, 4])
def test_special_scores(power):
    M = np.float32(4.0)          # a power of two: q_max = 2^23, so 1.5 * 2^-23 M quantises to floor(1.5) = 1
    e = np.array([M, M / 2, 1.5 * 2.0 ** -23 * M, 1.5 * 2.0 ** -24 * M, 0.0, np.nan, -1.0], np.float32)
    w, rec = AR.weights(e, power, 0.0)
    assert rec["max_p"] == np.float32(4.0) ** power and int(w[0]) == 2 ** 23
    assert w[4] == 0 and w[5] == 0                                   # zero and NaN
    assert int(w[6]) == (0 if power % 2 else int(np.ldexp(1.0, rec["shift"])))      # (-1)^power: negative -> 0
    if power == 1:
        assert int(w[1]) == int(w[0]) // 2 and w[2] == 1 and w[3] == 0
    # +inf: its power is capped at FLT_MAX and becomes the maximum
    w, rec = AR.weights(np.append(e, np.float32(np.inf)), power, 0.0)
    assert rec["max_p"] == AR.FLT_MAX and rec["shift"] == 23 - 127 and int(w[-1]) == 2 ** 24 - 1 and w[:7].max() == 0
    # the whole list at once with M = 2^127: +inf caps at FLT_MAX, the small scores still quantise to 1 and 0
    F = np.float32(2.0 ** 127)
    w, _ = AR.weights(np.array([F, F / 2, 1.5 * 2.0 ** -23 * F, 1.5 * 2.0 ** -24 * F, 0, np.nan, np.inf, -1], np.float32), 1, 0.0)
    assert [int(v) for v in w] == [2 ** 23, 2 ** 22, 1, 0, 0, 0, 2 ** 24 - 1, 0]


@pytest.mark.parametrize("floor", [0.0, 0.25, 1.0])
def test_all_zero_scores_give_uniform_weights(floor):
    rec, cdf, coarse = AR.build(np.zeros(1025, np.float32), 2, floor)
    a = 0 if floor == 0 else 1          # Q / N = 1: 0.25 truncates to 0 and is raised to 1
    assert rec["add"] == a and rec["shift"] == 0 and rec["q_sum"] == 1025
    assert np.array_equal(cdf, (1 + a) * np.arange(1, 1026, dtype=np.uint64))
    assert [int(c) for c in coarse] == [(1 + a) * 1024, (1 + a) * 1025]


def test_pack_and_unpack_are_inverse():
    e = _scores()
    rec, cdf, coarse = AR.build(e, 2, 0.25)
    buf = AR.pack(rec, cdf, coarse)
    assert buf.size == AR.nbytes(ROWS)
    r2, c2, k2 = AR.unpack(buf, ROWS)
    assert r2 == rec and np.array_equal(c2, cdf) and np.array_equal(k2, coarse)


@pytest.mark.parametrize("power,floor", [(1, 1.0), (2, 0.0), (3, 0.25), (4, 1.0)])
def test_torch_rule_of_the_generic_loop_is_the_same_rule(power, floor):
    ac = pkg("data.tabulated").adaptive_cdf
    e = _scores()
    e[3] = np.nan
    for sc in (e, np.zeros(5, np.float32), np.full(1025, 3.0, np.float32)):
        assert np.array_equal(ac(torch.from_numpy(sc), power, floor).numpy().astype(np.uint64), AR.build(sc, power, floor)[1])


# ---- 3. arguments
def test_adaptive_sampling_validates():
    AS = pkg("data.tabulated").AdaptiveSampling
    a = AS()
    assert (a.power, a.floor, a.every) == (1, 1.0, 100)
    for kw, word in ((dict(power=0), "power"), (dict(power=5), "power"), (dict(power=2.0), "power"), (dict(floor=-0.1), "floor"),
                     (dict(floor=float("nan")), "floor"), (dict(floor=float("inf")), "floor"), (dict(every=0), "every"),
                     (dict(every=1.5), "every")):
        with pytest.raises(ValueError, match=word):
            AS(**kw)


def _dataset(n_res=6):
    TP = pkg("data.tabulated").TabulatedProblem
    g = torch.Generator().manual_seed(2)
    X = lambda n: torch.rand(n, 3, generator=g)
    return TP(X(n_res), torch.zeros(n_res), X(4), torch.zeros(4), X(4), torch.zeros(4))


def test_trainer_argument_errors_name_the_reason():
    trainer = pkg("trainer.diffusion_train")
    AS = pkg("data.tabulated").AdaptiveSampling
    model = type("M", (), {"input_dim": 3, "n_out": 1})()
    with pytest.raises(ValueError, match="dataset="):
        trainer.FusedTrainer(model, 12, 4, adaptive=AS())
    with pytest.raises(ValueError, match="residual"):
        trainer.FusedTrainer(model, 12, 4, dataset=_dataset(0), adaptive=AS())
    with pytest.raises(ValueError, match="sampler='torch'"):
        trainer.FusedTrainer(model, 12, 4, sampler="torch", dataset=_dataset(), adaptive=AS())
    with pytest.raises(ValueError, match="AdaptiveSampling"):
        trainer.FusedTrainer(model, 12, 4, dataset=_dataset(), adaptive=True)
    with pytest.raises(ValueError, match="dataset="):
        trainer.train(Tiny(), batch_size=12, adaptive=AS())
    with pytest.raises(ValueError, match="residual"):
        trainer.train(Tiny(), batch_size=12, dataset=_dataset(0), adaptive=AS())


def test_struct_layout_and_host_side_refusals():
    L = pkg("hip.lib")
    lib = L.load()
    assert C.sizeof(L.QcStepAdapt) == 16 and L.QcStepAdapt.n_rows.offset == 8
    assert L.QC_ADAPT_BLOCK == AR.BLOCK == 1024
    for n in (1, 1024, 1025, 2 ** 31 - 1):
        assert lib.qc_adapt_bytes(n) == AR.nbytes(n)
    assert lib.qc_adapt_bytes(0) == 0 and lib.qc_adapt_bytes(2 ** 31) == 0
    fake = 4096
    ok = (fake, 10, 1, 0.0, fake, None)
    bad = lambda **kw: lib.qc_adapt_build(*[kw.get(k, v) for k, v in zip(("score", "n", "power", "floor", "buf", "st"), ok)])
    for kw in (dict(score=None), dict(buf=None), dict(buf=fake + 4), dict(n=0), dict(n=2 ** 31), dict(power=0), dict(power=5),
               dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=257.0)):
        assert bad(**kw) == -1, kw
    # the step, the gather and the scores: refused on the host, nothing dereferenced.  (The descriptor has no program, so
    # none of these could be accepted here: each check below is one the entry point makes BEFORE it looks at the program;
    # tests/test_gpu_adaptive_scores.py repeats them on a descriptor that is accepted.)
    d = _desc(L, L.QC_PROBLEM_TABULATED, 8, 2, 2)
    data = L.QcStepData(fake, fake, 0.0, fake, fake, 10, fake, fake, 10, fake, fake, 10)
    ad = lambda **kw: L.QcStepAdapt(kw.get("buf", fake), kw.get("n", 10))
    step = lambda desc, a: lib.qc_fused_pinn_adaptive_step(C.byref(desc), C.byref(data), None, a, L.QC_PHASE_GRADS, None)
    assert step(d, None) == -1
    for a in (ad(buf=None), ad(buf=fake + 4), ad(n=9), ad(n=11)):
        assert step(d, C.byref(a)) == -1
    assert step(_desc(L, L.QC_PROBLEM_TABULATED, 0, 2, 2), C.byref(ad())) == -1          # B_res = 0
    gather = lambda a, n_rows=10: lib.qc_sample_dataset_adaptive(fake, fake, 4, 0, fake, fake, 1, 0, 1, 0, None, C.byref(data), None,
                                                                 a, 1, 1, None)
    assert gather(None) == -1
    for a in (ad(buf=None), ad(n=9), ad(buf=fake + 1)):
        assert gather(C.byref(a)) == -1
    coef = L.QcStepCoef(None, fake)
    assert lib.qc_sample_dataset_adaptive(fake, fake, 4, 0, fake, fake, 1, 0, 1, 0, None, C.byref(data), C.byref(coef),
                                          C.byref(ad()), 1, 1, None) == -1          # a table but nowhere to put its rows
    scores = lambda desc, row0, rows, out=fake, cf=None: lib.qc_dataset_scores(C.byref(desc), C.byref(data), cf, row0, rows, out, None)
    for args in ((d, -1, 2), (d, 0, 0), (d, 0, 11), (d, 10, 1), (d, 5, 6)):
        assert scores(*args) == -1, args[1:]
    assert scores(d, 0, 10, out=None) == -1
    assert scores(_desc(L, L.QC_PROBLEM_TABULATED, 0, 2, 2), 0, 10) == -1
    assert scores(_desc(L, L.QC_PROBLEM_CONVECTION_DIFFUSION, 8, 2, 2), 0, 10) == -1
    assert scores(d, 0, 10, cf=C.byref(L.QcStepCoef(fake, None))) == -1


# ---- 4. the generic loop
def test_generic_loop_draws_only_rows_of_non_zero_weight(monkeypatch):
    """floor = 0 and NaN targets on every third residual row: their score is NaN, their weight 0.  The loop must never draw
    them (a single one would turn the loss into NaN), and must draw from the CDF it rebuilt."""
    trainer = pkg("trainer.diffusion_train")
    tab = pkg("data.tabulated")
    g = torch.Generator().manual_seed(4)
    X = lambda n: torch.rand(n, 3, generator=g)
    r = torch.randn(60, generator=g)
    r[::3] = float("nan")
    ds = tab.TabulatedProblem(X(60), r, X(10), torch.zeros(10), X(10), torch.zeros(10))
    drawn, cdfs = [], []
    plain = trainer._RowSampler.sample

    def spy(self, N):
        out = plain(self, N)
        if self.cdf is not None:
            drawn.append(self.idx.clone())
            cdfs.append(self.cdf.clone())
        return out
    monkeypatch.setattr(trainer._RowSampler, "sample", spy)
    torch.manual_seed(0)
    m = Tiny()
    m.epochs = 4
    torch.manual_seed(1)
    trainer.train(m, batch_size=12, dataset=ds, adaptive=tab.AdaptiveSampling(power=2, floor=0.0, every=2))
    assert len(m.loss_history) == 5 and np.isfinite(m.loss_history).all()
    rows = torch.cat(drawn)
    assert rows.numel() == 5 * 12 and (rows % 3 != 0).all() and rows.unique().numel() > 5
    # rescored before iterations 0, 2 and 4
    same = [torch.equal(a, b) for a, b in zip(cdfs, cdfs[1:])]
    assert same == [True, False, True, False]
    # and the CDF is the restatement's on the loop's own scores
    w = torch.diff(cdfs[0], prepend=torch.zeros(1, dtype=torch.int64))
    assert (w[::3] == 0).all() and (w[1::3] > 0).any()
