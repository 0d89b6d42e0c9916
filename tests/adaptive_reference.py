"""Numpy restatement of residual-adaptive sampling as include/qcpinn_hip.h defines it (qc_adapt_build,
qc_sample_dataset_adaptive), written from the header text; it is not a port of the kernels.

Scores -> CDF (``build``):
  1. p_j = score_j ** power by left-to-right float32 multiplication, power in 1..4; a p_j that is NaN or negative counts
     as 0, one above FLT_MAX as FLT_MAX.
  2. M = max p_j.  M = 0: q_j = 1.  Otherwise s = 23 - ilogb(M) and q_j = floor(p_j * 2**s): the largest in [2**23, 2**24).
  3. Q = sum q_j; a = int(float64(floor_c) * float64(Q) / float64(N)), raised to 1 when floor_c > 0 and it truncates to 0;
     w_j = q_j + a.
  4. cdf_j = sum_{i <= j} w_i (uint64); coarse[b] = cdf[min(N, (b + 1) * 1024) - 1].
  buffer = 64-byte record {uint64 total, q_sum, add; float32 max_p; int32 shift; pad} | cdf[N] | coarse[ceil(N / 1024)].

Draw (``indices``): residual point with global index g takes the Philox4x32-10 block of the uniform gather (counter
(g lo, g hi, step lo, step hi), key = seed), r64 = word 0 << 32 | word 1, t = (r64 * T) >> 64 with T = cdf[N - 1], and
row min{j : cdf_j > t}.
"""
import math

import numpy as np

import philox_reference as PR

BLOCK = 1024
FLT_MAX = np.float32(3.4028234663852886e38)
RECORD_BYTES = 64


def powers(score, power):
    """(N,) float32 p_j."""
    assert 1 <= power <= 4
    e = np.asarray(score, dtype=np.float32)
    with np.errstate(all="ignore"):
        p = e.copy()
        for _ in range(power - 1):
            p = (p * e).astype(np.float32)
        p = np.where(p > 0, p, np.float32(0))          # NaN, negative and -0 -> 0
        p = np.minimum(p, FLT_MAX)
    return p.astype(np.float32)


def weights(score, power, floor_c):
    """-> (w (N,) Python-int-exact uint64, record dict)."""
    p = powers(score, power)
    N = p.size
    M = np.float32(p.max())
    if M == 0:
        q, s = np.ones(N, dtype=np.uint64), 0
    else:
        s = 23 - (math.frexp(float(M))[1] - 1)         # ilogb(M) = frexp exponent - 1, subnormals included
        q = np.floor(np.ldexp(p.astype(np.float64), s)).astype(np.uint64)      # exact in float64: below 2**24
        assert 2 ** 23 <= int(q.max()) < 2 ** 24
    Q = int(q.sum(dtype=np.uint64))
    a = int(np.float64(np.float32(floor_c)) * np.float64(Q) / np.float64(N))
    if floor_c > 0 and a == 0:
        a = 1
    w = q + np.uint64(a)
    return w, {"q_sum": Q, "add": a, "max_p": M, "shift": s}


def build(score, power, floor_c):
    """-> (record dict incl. total, cdf (N,) uint64, coarse (ceil(N / 1024),) uint64)."""
    w, rec = weights(score, power, floor_c)
    cdf = np.cumsum(w, dtype=np.uint64)
    N = cdf.size
    ends = np.minimum(N, (np.arange((N + BLOCK - 1) // BLOCK) + 1) * BLOCK) - 1
    rec["total"] = int(cdf[-1])
    return rec, cdf, cdf[ends]


def nbytes(N):
    return RECORD_BYTES + 8 * (N + (N + BLOCK - 1) // BLOCK)


def pack(rec, cdf, coarse):
    """The buffer's bytes as a uint8 array."""
    head = np.zeros(RECORD_BYTES, dtype=np.uint8)
    head[0:24] = np.array([rec["total"], rec["q_sum"], rec["add"]], dtype=np.uint64).view(np.uint8)
    head[24:28] = np.array([rec["max_p"]], dtype=np.float32).view(np.uint8)
    head[28:32] = np.array([rec["shift"]], dtype=np.int32).view(np.uint8)
    return np.concatenate([head, np.asarray(cdf, dtype=np.uint64).view(np.uint8), np.asarray(coarse, dtype=np.uint64).view(np.uint8)])


def unpack(buf, N):
    """uint8 buffer -> (record dict, cdf, coarse)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    u64 = buf[0:24].view(np.uint64)
    rec = {"total": int(u64[0]), "q_sum": int(u64[1]), "add": int(u64[2]), "max_p": buf[24:28].view(np.float32)[0],
           "shift": int(buf[28:32].view(np.int32)[0])}
    nb = (N + BLOCK - 1) // BLOCK
    body = buf[RECORD_BYTES:RECORD_BYTES + 8 * (N + nb)].view(np.uint64)
    return rec, body[:N].copy(), body[N:].copy()


def from_cdf(cdf):
    """A hand-written buffer: any non-decreasing uint64 CDF with its coarse table (the record carries the total)."""
    cdf = np.asarray(cdf, dtype=np.uint64)
    N = cdf.size
    ends = np.minimum(N, (np.arange((N + BLOCK - 1) // BLOCK) + 1) * BLOCK) - 1
    rec = {"total": int(cdf[-1]), "q_sum": 0, "add": 0, "max_p": np.float32(0), "shift": 0}
    return rec, cdf, cdf[ends]


def indices(cdf, offset, count, seed, step):
    """(count,) int64 rows of the residual points with global indices offset .. offset + count - 1."""
    cdf = np.asarray(cdf, dtype=np.uint64)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    g = np.uint64(offset) + np.arange(count, dtype=np.uint64)
    ctr = (g & PR.MASK, g >> PR.S32, step & 0xFFFFFFFF, step >> 32)          # segment 0
    w = PR.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    T = int(cdf[-1])
    t = np.array([((int(a) << 32 | int(b)) * T) >> 64 for a, b in zip(w[0], w[1])], dtype=np.uint64)
    return np.searchsorted(cdf, t, side="right").astype(np.int64)          # first j with cdf_j > t
