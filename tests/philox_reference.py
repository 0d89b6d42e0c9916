"""Numpy restatement of the device sampler: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
SC'11; the Random123 library's ``philox4x32_10``) and the collocation-point draw documented in include/qcpinn_hip.h and
csrc/qc_philox.h.  uint64 arithmetic, vectorised over the point index; tests/test_philox_reference.py pins the round
function to the Random123 known-answer vectors, the GPU tests then compare the device's points with it bit for bit.

The draw of global point ``g`` of segment ``seg`` (0 residual, 1 IC, 2 BC):
  counter = (g & 0xffffffff, g >> 32, step & 0xffffffff, (step >> 32) ^ (seg << 30)),  key = (seed & 0xffffffff, seed >> 32)
  (t, x, y) = float32((word >> 8) * 2**-24) of output words 0, 1, 2;  t = 0 for IC points;
  a BC point lies on face g // bc_face_points (bc_face_points > 0), face 0 (bc_face_points = 0) or face word3 >> 30
  (QC_BC_RANDOM_FACE); faces 0..3 are x = 0, x = 1, y = 0, y = 1.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # round multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)          # key increments (Weyl sequence)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
QC_BC_RANDOM_FACE = -1


def philox4x32_10(ctr, key):
    """ctr: four arrays (or ints) of 32-bit words, key: two -> the four output words as uint64 arrays (values < 2^32)."""
    c0, c1, c2, c3 = [np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK for c in ctr]
    k0, k1 = [np.uint64(int(k) & 0xFFFFFFFF) for k in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                                 # 32 x 32 -> 64 bit products: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def u01(word):
    """The device's uniform in [0, 1): the top 24 bits of a word, exact in float32."""
    return ((word >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def draw(seg, offset, count, seed, step, bc_face_points=0):
    """(count, 3) float32 points (t, x, y) of global indices offset .. offset + count - 1 of one segment."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    g = np.uint64(offset) + np.arange(count, dtype=np.uint64)
    ctr = (g & MASK, g >> S32, step & 0xFFFFFFFF, (step >> 32) ^ ((seg << 30) & 0xFFFFFFFF))
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    t, x, y = u01(r[0]), u01(r[1]), u01(r[2])
    if seg == 1:
        t = np.zeros_like(t)
    if seg == 2:
        if bc_face_points == QC_BC_RANDOM_FACE:
            face = (r[3] >> np.uint64(30)).astype(np.int64)
        elif bc_face_points > 0:
            face = (g // np.uint64(bc_face_points)).astype(np.int64)
        else:
            face = np.zeros(count, dtype=np.int64)
        x = np.where(face == 0, np.float32(0), np.where(face == 1, np.float32(1), x))
        y = np.where(face == 2, np.float32(0), np.where(face >= 3, np.float32(1), y))
    return np.stack([t, x, y], axis=1).astype(np.float32)


def collocation(n_res, off_res, n_ic, off_ic, n_bc, off_bc, bc_face_points, seed, step):
    """(X_res, X_val) as qc_sample_collocation_faces fills them: X_val holds the IC points first, then the BC points."""
    X_res = draw(0, off_res, n_res, seed, step)
    X_val = np.concatenate([draw(1, off_ic, n_ic, seed, step), draw(2, off_bc, n_bc, seed, step, bc_face_points)])
    return X_res, X_val
