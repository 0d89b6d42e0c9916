"""tests/philox_reference.py against the Random123 known-answer vectors of philox4x32_10 (kat_vectors of the Random123
distribution), and the properties of the draw the GPU tests rely on.  No GPU."""
import numpy as np
import pytest

import philox_reference as PR

KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox4x32_10_known_answers(ctr, key, want):
    got = tuple(int(w[0]) for w in PR.philox4x32_10(ctr, key))
    assert got == want, [hex(w) for w in got]


def test_philox_is_vectorised_over_the_counter():
    """The three vectors as ONE call per key differ only in the counter arrays: element i equals the scalar call."""
    for ctr, key, want in KAT:
        arr = [np.array([0, c, 1], dtype=np.uint64) for c in ctr]
        got = PR.philox4x32_10(arr, key)
        assert tuple(int(w[1]) for w in got) == want
        assert tuple(int(w[0]) for w in got) != tuple(int(w[2]) for w in got)


def test_draw_places_index_step_seed_and_segment_in_the_documented_words():
    """Global index -> counter words 0, 1; step -> word 2 and (xor the segment's two top bits) word 3; seed -> key."""
    seed, step, g = 0x299F31D0A4093822, (0x03707344 << 32) | 0x13198A2E, (0x85A308D3 << 32) | 0x243F6A88
    words = KAT[2][2]
    want = [np.float32((w >> 8) * 2.0 ** -24) for w in words[:3]]
    got = PR.draw(0, g, 1, seed, step)[0]
    assert list(got) == want
    # segment 2 flips bit 31 of counter word 3 (0x03707344 -> 0x83707344): another point altogether, on the x = 0 face
    bc = PR.draw(2, g, 1, seed, step)[0]
    r = PR.philox4x32_10((g & 0xFFFFFFFF, g >> 32, step & 0xFFFFFFFF, 0x83707344), (seed & 0xFFFFFFFF, seed >> 32))
    assert bc[0] == np.float32((int(r[0][0]) >> 8) * 2.0 ** -24) and bc[1] == 0.0
    assert bc[2] == np.float32((int(r[2][0]) >> 8) * 2.0 ** -24)
    ic = PR.draw(1, g, 1, seed, step)[0]
    assert ic[0] == 0.0 and ic[1] != got[1]


def test_draw_ranges_faces_and_shards():
    X = PR.draw(0, 2 ** 32 - 500, 1000, 77, 5)
    assert X.dtype == np.float32 and X.shape == (1000, 3) and X.min() >= 0.0 and X.max() < 1.0
    assert abs(X.mean() - 0.5) < 0.03
    # a shard indexed by the global point index is a slice of the whole batch, across the 2^32 boundary of the index
    assert np.array_equal(PR.draw(0, 2 ** 32 - 100, 300, 77, 5), X[400:700])
    assert not np.array_equal(PR.draw(0, 2 ** 32 - 500, 1000, 77, 2 ** 32 + 5), X)       # the step's high word counts
    assert not np.array_equal(PR.draw(0, 2 ** 32 - 500, 1000, 77 + 2 ** 32, 5), X)       # and the seed's
    assert not np.array_equal(PR.draw(0, 0, 500, 77, 5), X[500:])                        # and the index's
    B = PR.draw(2, 0, 260, 77, 5, 65)
    for f, (col, val) in enumerate(((1, 0.0), (1, 1.0), (2, 0.0), (2, 1.0))):
        blk = B[65 * f:65 * (f + 1)]
        assert np.all(blk[:, col] == val)
        free = blk[:, [c for c in (0, 1, 2) if c != col]]
        assert free.min() >= 0.0 and free.max() < 1.0 and free.std() > 0.2
    assert np.all(PR.draw(2, 0, 260, 77, 5, 0)[:, 1] == 0.0)
    R = PR.draw(2, 0, 4000, 77, 5, PR.QC_BC_RANDOM_FACE)
    on = np.stack([R[:, 1] == 0.0, R[:, 1] == 1.0, R[:, 2] == 0.0, R[:, 2] == 1.0])
    assert np.all(on.sum(axis=0) == 1)                        # exactly one coordinate pinned (u01 < 1; 0 has odds 2^-24)
    assert np.all(np.abs(on.mean(axis=1) - 0.25) < 0.03)      # 4000 points: sigma = 0.007
    Xr, Xv = PR.collocation(10, 0, 4, 7, 6, 3, 0, 1, 2)
    assert Xr.shape == (10, 3) and Xv.shape == (10, 3) and np.all(Xv[:4, 0] == 0.0) and np.all(Xv[4:, 1] == 0.0)
