"""qc_sample_dataset_adaptive on the GPU, bit for bit against the numpy restatement of its draw
(tests/adaptive_reference.py::indices): on hand-written buffers (the layout is public: 64-byte record, CDF, coarse table)
and on buffers qc_adapt_build filled.  The IC and BC rows must be those of qc_sample_dataset on the same seed and step;
every output sits in front of NaN sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

import adaptive_reference as AR
import coef_reference as CR
from conftest import pkg
from test_gpu_adaptive_cdf import gpu_build
from test_gpu_tabulated import _dataset, _gather, _step_data

pytestmark = pytest.mark.gpu

SEED, STEP = 0x1234567890ABCDEF, (1 << 33) + 3
N_IC, N_BC = 9, 5          # rows of the value segments


def _adaptive_gather(dev, ten, table, parts, counts, offs, seed=SEED, step=STEP):
    """-> [X_res, target_res, X_val, target_val, coef rows (n_res, 7) or None] of one call on the buffer ``parts`` =
    (record, cdf, coarse); ``table`` (N, 7) device tensor or None."""
    L = pkg("hip.lib")
    lib = L.load()
    n_res, n_ic, n_bc = counts
    N = ten[0][0].shape[0]
    raw = AR.pack(*parts)
    buf = torch.from_numpy(np.concatenate([raw, np.full(64, 0xFF, np.uint8)])).to(dev)
    assert buf.data_ptr() % 8 == 0
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    Xr, tr, Xv, tv, cf = nan(n_res + 3, 3), nan(n_res + 3), nan(n_ic + n_bc + 3, 3), nan(n_ic + n_bc + 3), nan(7 * n_res + 5)
    data = _step_data(L, ten)
    coef = None if table is None else L.QcStepCoef(cf.data_ptr(), table.data_ptr())
    ad = L.QcStepAdapt(buf.data_ptr(), N)
    L.check(lib.qc_sample_dataset_adaptive(Xr.data_ptr(), tr.data_ptr(), n_res, offs[0], Xv.data_ptr(), tv.data_ptr(), n_ic,
                                           offs[1], n_bc, offs[2], None if coef is None else cf.data_ptr(), C.byref(data),
                                           None if coef is None else C.byref(coef), C.byref(ad), seed, step,
                                           torch.cuda.current_stream(dev).cuda_stream), "qc_sample_dataset_adaptive")
    torch.cuda.synchronize(dev)
    assert np.array_equal(buf.cpu().numpy()[:raw.size], raw)          # the buffer is only read
    out = [t.cpu().numpy() for t in (Xr, tr, Xv, tv, cf)]
    sizes = (n_res, n_res, n_ic + n_bc, n_ic + n_bc, 7 * n_res if coef is not None else 0)
    for a, m in zip(out, sizes):
        assert np.isnan(a[m:]).all(), "the gather wrote past its batch"
    out = [a[:m] for a, m in zip(out, sizes)]
    out[4] = out[4].reshape(7, n_res).T if coef is not None else None
    return out


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(dev, arr, ten, table, parts, n_res, off, with_table, n_val=(4, 3)):
    tab_dev = torch.from_numpy(table).to(dev) if with_table else None
    counts, offs = (n_res, *n_val), (off, 2, 6)
    got = _adaptive_gather(dev, ten, tab_dev, parts, counts, offs)
    k = AR.indices(parts[1], off, n_res, SEED, STEP)
    (X, r) = arr[0]
    assert _bits(got[0], X[k]) and _bits(got[1], r[k])
    if with_table:
        assert _bits(got[4], table[k])
    else:
        assert got[4] is None
    # the value rows are the uniform gather's
    L = pkg("hip.lib")
    plain = _gather(L.load(), L, dev, _step_data(L, ten), counts, offs, SEED, STEP)
    assert _bits(got[2], plain[2]) and _bits(got[3], plain[3])
    return k, plain


@pytest.mark.parametrize("N", [1, 3, 1025, 70000])
def test_rows_targets_and_operator_rows_match_the_restatement(N, gpu_device):
    arr, ten = _dataset(gpu_device, (N, N_IC, N_BC), seed=N)
    table = CR.coef_star(arr[0][0])
    g = np.random.default_rng(N + 1)
    score = np.abs(g.standard_normal(N)).astype(np.float32)
    score[::5] = 0.0
    if N == 1:
        score[:] = 2.0
    built = gpu_build(gpu_device, score, 2, 0.0)
    assert built[0] == AR.build(score, 2, 0.0)[0]
    w_hand = g.integers(0, 2 ** 40, N, dtype=np.uint64) * (g.random(N) < 0.7).astype(np.uint64)      # zeros among them
    w_hand[-1] += np.uint64(1)
    hand = AR.from_cdf(np.cumsum(w_hand, dtype=np.uint64))
    seen = 0
    for parts in (built, hand):
        for n_res, off, with_table in ((1, 0, True), (65, 1 << 32, False), (257, (1 << 32) + 12345, True)):
            k, plain = _check(gpu_device, arr, ten, table, parts, n_res, off, with_table)
            w = np.diff(parts[1], prepend=np.uint64(0))
            assert (w[k] > 0).all()          # no row of weight zero
            if N > 3 and n_res == 257:
                assert np.unique(k).size > 100 and not np.array_equal(arr[0][1][k], plain[1])      # not the uniform draw
                seen += 1
    assert seen == (2 if N > 3 else 0)


@pytest.mark.parametrize("with_table", [False, True], ids=["rows", "table"])
@pytest.mark.parametrize("counts", [(65, 300, 200), (257, 0, 3), (255, 1, 0)], ids=lambda c: "x".join(map(str, c)))
def test_blocks_of_value_points_only_and_empty_batches(counts, with_table, gpu_device):
    """Launch shapes no other case has: blocks that hold value points only (65 + 300 + 200 points: the second and third
    block of 256 skip the staging of the coarse table and its barrier), a residual batch that ends one point into the
    second block with no IC points behind it, and a last block filled to its last thread with no BC points.  1025 rows:
    two coarse entries, the second over a single row that holds a third of the weight.  The uniform gathers (the other
    instantiations of the same kernel) fill the same shapes, against the numpy restatement of their draw."""
    from test_gpu_coef import _expected_coef, _gather_coef
    N = AR.BLOCK + 1
    arr, ten = _dataset(gpu_device, (N, N_IC, N_BC), seed=21)
    table = CR.coef_star(arr[0][0])
    g = np.random.default_rng(22)
    w = g.integers(0, 2 ** 20, N, dtype=np.uint64) * (g.random(N) < 0.7).astype(np.uint64)
    w[-1] = w[:-1].sum() // np.uint64(2)
    parts = AR.from_cdf(np.cumsum(w, dtype=np.uint64))
    assert parts[2].size == 2
    off = (1 << 32) + 7
    k, plain = _check(gpu_device, arr, ten, table, parts, counts[0], off, with_table, counts[1:])
    assert (w[k] > 0).all() and (k == N - 1).any() and (k < N - 1).any()
    offs = (off, 2, 6)
    L = pkg("hip.lib")
    want = _expected_coef(arr, table, offs, counts, SEED, STEP)
    got = _gather_coef(L.load(), L, gpu_device, _step_data(L, ten), torch.from_numpy(table).to(gpu_device), counts, offs, SEED, STEP)
    for a, b in zip(list(plain) + got, want[:4] + want):
        assert _bits(a, b)


def test_flat_spots_and_single_hot_rows(gpu_device):
    """cdf = [1, 1, 2] yields rows {0, 2} only; all weight on the first row, the last row and the first row of a coarse
    block (1024, and 2048 of 2050 rows) is always found."""
    arr, ten = _dataset(gpu_device, (3, N_IC, N_BC), seed=1)
    k, _ = _check(gpu_device, arr, ten, None, AR.from_cdf([1, 1, 2]), 257, (1 << 32) - 5, False)
    assert set(k.tolist()) == {0, 2}
    arr, ten = _dataset(gpu_device, (2050, N_IC, N_BC), seed=2)
    table = CR.coef_star(arr[0][0])
    for hot in (0, 1024, 2048, 2049):
        cdf = np.zeros(2050, np.uint64)
        cdf[hot:] = 7
        k, _ = _check(gpu_device, arr, ten, table, AR.from_cdf(cdf), 65, 0, True)
        assert (k == hot).all()
        e = np.zeros(2050, np.float32)
        e[hot] = 0.3
        k, _ = _check(gpu_device, arr, ten, table, gpu_build(gpu_device, e, 1, 0.0), 65, 5, False)
        assert (k == hot).all()


def test_coarse_table_too_large_for_lds_is_searched_in_global_memory(gpu_device):
    """More than 4096 coarse entries (4096 * 1024 + 1 rows) take the kernel's other instantiation, which searches the
    coarse table where it lies.  A sparse hand-written CDF: weight on about a thousand rows, among them the first row, the
    first and the last row of the last full block, and the single row of the last block."""
    N = 4096 * AR.BLOCK + 1
    arr, ten = _dataset(gpu_device, (N, N_IC, N_BC), seed=11)
    g = np.random.default_rng(12)
    w = np.zeros(N, np.uint64)
    hot = np.concatenate([g.integers(0, N, 1000), [0, N - 1 - AR.BLOCK, N - 2, N - 1]])
    w[hot] = g.integers(1, 2 ** 30, hot.size, dtype=np.uint64)
    parts = AR.from_cdf(np.cumsum(w, dtype=np.uint64))
    assert parts[2].size == 4097
    k, _ = _check(gpu_device, arr, ten, None, parts, 257, (1 << 32) - 100, False)
    assert (w[k] > 0).all() and np.unique(k).size > 100
    # all weight on the last row: the one-row block behind the 4096 full ones
    cdf = np.zeros(N, np.uint64)
    cdf[-1] = 5
    k, _ = _check(gpu_device, arr, ten, None, AR.from_cdf(cdf), 65, 0, False)
    assert (k == N - 1).all()


def test_refusals(gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    arr, ten = _dataset(gpu_device, (10, N_IC, N_BC), seed=3)
    buf = torch.from_numpy(AR.pack(*AR.from_cdf(np.arange(1, 11)))).to(gpu_device)
    out = torch.full((64,), float("nan"), device=gpu_device)
    data = _step_data(L, ten)
    p = out.data_ptr()
    call = lambda ad, d=data: lib.qc_sample_dataset_adaptive(p, p, 4, 0, p, p, 1, 0, 1, 0, None, C.byref(d), None, ad, 1, 1, None)
    for ad in (L.QcStepAdapt(None, 10), L.QcStepAdapt(buf.data_ptr(), 9), L.QcStepAdapt(buf.data_ptr(), 11),
               L.QcStepAdapt(buf.data_ptr() + 4, 10)):
        assert call(C.byref(ad)) == -1
    assert call(None) == -1
    bad = type(data).from_buffer_copy(data)
    bad.ds_X_ic = None
    assert call(C.byref(L.QcStepAdapt(buf.data_ptr(), 10)), bad) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert call(C.byref(L.QcStepAdapt(buf.data_ptr(), 10))) == 0
    torch.cuda.synchronize()
