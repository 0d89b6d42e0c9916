"""qc_reduce_rows (k_reduce_rows, csrc/qc_optim.hip) on its own, exactly.

The partial rows hold seeded integers in [-512, 512] stored as fp32: every partial sum of up to 4097 of them stays below
2^22, so fp32 addition is exact in any order and the expected column sum is the int64 sum, compared with
``np.array_equal``.  A lost or doubled row cannot hide under a tolerance.

Row counts sit on both sides of the per-wave stride (16 waves: wave w takes rows w, w + 16, ...) and of the entry
condition of the 4-way unrolled loop (r + 48 < rows, step 64) for waves 0 and 15; column counts on both sides of the
64-column block.  With stride > ncols the padding columns hold NaN, which must never reach the output, and 64 sentinel
floats behind the output must stay as they were."""
import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

ROWS = [1, 2, 15, 16, 17, 47, 48, 49, 63, 64, 65, 79, 80, 81, 113, 128, 129, 1000, 4097]
NCOLS = [1, 63, 64, 65, 130]
PAD = 7
SENTINEL = -12345.0


def _cases():
    """Every row count with two column counts (rotating, so every column count meets several row counts and the
    largest row counts meet more than one block), each with both strides: 19 x 2 x 2 of the 19 x 5 x 2 grid."""
    out = []
    for i, rows in enumerate(ROWS):
        for ncols in (NCOLS[i % 5], NCOLS[(i + 2) % 5]):
            for pad in (0, PAD):
                out.append((rows, ncols, pad))
    return out


CASES = _cases()


def test_case_grid_keeps_every_size_with_each_stride():
    for pad in (0, PAD):
        assert {c[0] for c in CASES if c[2] == pad} == set(ROWS)
        assert {c[1] for c in CASES if c[2] == pad} == set(NCOLS)


@pytest.fixture(scope="module")
def reduce_all(gpu_device):
    """All cases in one pass over the device (one synchronisation): case -> (part as int64, out incl. sentinels)."""
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    pending = {}
    for k, (rows, ncols, pad) in enumerate(CASES):
        rng = np.random.default_rng(1000 + k)
        stride = ncols + pad
        vals = rng.integers(-512, 513, size=(rows, ncols), dtype=np.int64)
        part = np.full((rows, stride), np.nan, dtype=np.float32)
        part[:, :ncols] = vals
        d_part = torch.from_numpy(part).to(gpu_device)
        d_out = torch.full((ncols + 64,), SENTINEL, dtype=torch.float32, device=gpu_device)
        L.check(lib.qc_reduce_rows(d_part.data_ptr(), rows, stride, ncols, d_out.data_ptr(), st), "qc_reduce_rows")
        pending[(rows, ncols, pad)] = (vals, d_part, d_out)
    torch.cuda.synchronize()
    return {k: (vals, d_out.cpu().numpy()) for k, (vals, _, d_out) in pending.items()}


@pytest.mark.parametrize("rows,ncols,pad", CASES, ids=[f"r{r}_c{c}_s{c + p}" for r, c, p in CASES])
def test_reduce_rows_is_the_exact_column_sum(rows, ncols, pad, reduce_all):
    vals, out = reduce_all[(rows, ncols, pad)]
    assert np.abs(vals).sum(axis=0).max() < 2 ** 22                 # exact in fp32 in any order
    want = vals.sum(axis=0)
    got = out[:ncols]
    assert np.isfinite(got).all()
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), \
        np.argwhere(got != want)[:4]
    assert np.all(out[ncols:] == np.float32(SENTINEL))
    # host-side controls: a sum that loses one row, or counts one twice, is told apart (no generated row is all zero
    # against the sum in every column)
    for r in sorted({0, rows // 2, rows - 1}):
        assert np.any(vals[r] != 0)
        assert not np.array_equal(got, (want - vals[r]).astype(np.float32))
        assert not np.array_equal(got, (want + vals[r]).astype(np.float32))


def test_reduce_rows_refuses_bad_arguments(gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    buf = torch.zeros(64, device=gpu_device)
    for rows, stride, ncols in ((0, 4, 4), (1, 3, 4), (1, 4, 0)):
        assert lib.qc_reduce_rows(buf.data_ptr(), rows, stride, ncols, buf.data_ptr(), None) != 0
