"""qc_adapt_build on the GPU against the numpy restatement of its rule (tests/adaptive_reference.py): record, CDF and
coarse table bit for bit (the results are integers, so no summation order can show), behind sentinels.

Sizes: the ends and the middle of one block of QC_ADAPT_BLOCK = 1024 rows, more than one block, and both sides of the
second level's tile boundary (its one block scans 1024 coarse entries per pass: 1024 * 1024 rows are one pass,
one row more is two)."""
import numpy as np
import pytest
import torch

import adaptive_reference as AR
from conftest import pkg

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
TILE_ROWS = 1024 * AR.BLOCK          # rows behind one pass of the second-level loop


def gpu_build(dev, score, power, floor_c, pad=64):
    """The buffer qc_adapt_build fills for ``score`` as (record, cdf, coarse), after checking the bytes behind it."""
    L = pkg("hip.lib")
    lib = L.load()
    N = score.size
    need = int(lib.qc_adapt_bytes(N))
    assert need == AR.nbytes(N)
    buf = torch.full((need + pad,), SENTINEL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 8 == 0
    sc = torch.from_numpy(np.ascontiguousarray(score, dtype=np.float32)).to(dev)
    L.check(lib.qc_adapt_build(sc.data_ptr(), N, power, floor_c, buf.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "qc_adapt_build")
    torch.cuda.synchronize(dev)
    raw = buf.cpu().numpy()
    assert (raw[need:] == SENTINEL).all(), "qc_adapt_build wrote past its buffer"
    assert (raw[32:64] == 0).all()          # the record's padding
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), np.asarray(score, np.float32).view(np.uint32))
    return AR.unpack(raw, N)


def check(dev, score, power, floor_c):
    got, want = gpu_build(dev, score, power, floor_c), AR.build(score, power, floor_c)
    assert got[0] == want[0], (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    return want


@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025, 2 * 1024 + 1, TILE_ROWS, TILE_ROWS + 1])
def test_equal_scores_carry_past_32_bits(N, gpu_device):
    """All scores 3.0: q = 1.5 * 2^23 per row, so the sum of q passes 2^32 from N = 1025 on."""
    rec, cdf, coarse = check(gpu_device, np.full(N, 3.0, np.float32), 1, 0.25)
    if N >= 1025:
        assert rec["q_sum"] > 2 ** 32 and int(cdf[-1]) == rec["total"] > 2 ** 32
    assert coarse.size == (N + 1023) // 1024


@pytest.mark.parametrize("floor_c", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("power", [1, 2, 3, 4])
def test_random_and_special_scores(power, floor_c, gpu_device):
    g = np.random.default_rng(10 * power + int(4 * floor_c))
    for N in (1, 1023, 1025, 2 * 1024 + 1):
        e = np.abs(g.standard_normal(N)).astype(np.float32) * np.float32(10.0 ** g.integers(-6, 6))
        e[g.integers(0, N)] = 0.0
        check(gpu_device, e, power, floor_c)
    for M in (np.float32(4.0), np.float32(2.0 ** 127), np.float32(2.0 ** -100)):
        e = np.array([M, M / 2, 1.5 * 2.0 ** -23 * M, 1.5 * 2.0 ** -24 * M, 0.0, np.nan, np.inf, -1.0], np.float32)
        rec, cdf, _ = check(gpu_device, e, power, floor_c)
        assert rec["max_p"] == AR.FLT_MAX          # +inf caps at FLT_MAX and is the maximum
        rec, cdf, _ = check(gpu_device, np.delete(e, 6), power, floor_c)
        if power == 1:          # M a power of two: q = 2^23, 2^22, 1, 0, 0, 0 (NaN), 0 (negative)
            w = np.diff(np.concatenate([[0], cdf.astype(np.int64)])) - rec["add"]
            assert w.tolist() == [2 ** 23, 2 ** 22, 1, 0, 0, 0, 0]
    # all zero: uniform weights
    rec, cdf, _ = check(gpu_device, np.zeros(1025, np.float32), power, floor_c)
    assert rec["max_p"] == 0 and rec["shift"] == 0 and int(cdf[-1]) == 1025 * (1 + rec["add"])


def test_tile_boundary_with_varied_scores(gpu_device):
    """Both sides of the second level's tile boundary again, with scores that differ row by row and a zero floor."""
    g = np.random.default_rng(3)
    for N in (TILE_ROWS, TILE_ROWS + 1):
        e = np.abs(g.standard_normal(N)).astype(np.float32)
        e[::7] = 0.0
        check(gpu_device, e, 2, 0.0)
