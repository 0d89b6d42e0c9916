"""The reverse pass of the pre network (k_pre_bwd_body, csrc/qc_mlp.hip) stages a tile's cotangents by whole rows: a wave
requests a chunk of rows, its row of the X values and the thread's weights before the first LDS store, a chunk loop takes
the rows a narrow block has left, and the sums over the point groups read a chunk of groups ahead of the first add.
These cases put every shape of that staging behind a float64 torch evaluation of the same network on the same cotangents.

Driven: qc_pre_backward / qc_pre_backward_map stand-alone, and stage 4 (QC_STAGE_PRE_BWD) through qc_fused_step_stage,
on buffers the test fills itself (cotangents, and for the mapped network the angle jets, from seeded generators and the
float64 reference; no other kernel runs first).

Shapes:
  H = 7    HB = 7, 36 point groups of two points, 256 threads: many groups, several trips of the group sums
  H = 50   HB = 50, 5 groups, 256 threads: the benchmark's geometry
  H = 129  one group, 192 threads: three waves, a chunk of four row pairs serves the 3 n pairs of n <= 4, not of n = 5
  H = 300  HB = 320, two groups, 640 threads: more waves than rows at n = 2
  n = 2, 4, 5; six-channel (residual) and one-channel (value) tiles; the identity map and a = pi tanh(v)
  B = 1, 63, 65, 129: one live point; a partial tile; one point past a full tile; two full tiles plus one point

Every cotangent buffer ends in 64 NaNs past its last row, and the rows lie B apart, so a lane past the batch's end that
reached a sum would bring in a NaN or a neighbouring row's value.  The tile rows are NaN before the launch: the columns of
W1, b1, W2, b2 must come back finite and equal to the reference, every other column and row must still be NaN.  In the
merged stage the angle-jet buffers of the identity map stay NaN as well: they must not be read.

Tolerance: ROW_TOL of tests/test_gpu_mlp_shapes.py (2e-4 relative to max(1, max |reference|) of the compared rows), the
bound the network-kernel tests apply to these columns."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hybrid_pinn_reference as HR
import mlp_reference as R
import test_gpu_mlp_shapes as S
from conftest import pkg

ROW_TOL = S.ROW_TOL
WIDTHS = (7, 50, 129, 300)
QUBITS = (2, 4, 5)
BATCHES = (1, 63, 65, 129)
STAGE_SHAPES = ((1, 63), (63, 65), (65, 129), (129, 1))      # (B_res, B_val)
NAMES = ("W1", "b1", "W2", "b2")


def _ids(c):
    return "H{}_n{}".format(*c)


CASES = [(H, n) for H in WIDTHS for n in QUBITS]


def _n_cols(H, n):
    return 3 * H + H + n * H + n          # W1, b1, W2, b2 lead the flat vector


@functools.lru_cache(maxsize=None)
def _net(H, n):
    """Flat float32 parameters (torch's default Linear scales) in the layout of a cascade program of one layer."""
    lay, NP = R.layout(H, n, 3 * n)
    rng = np.random.default_rng(1000 * H + n)
    flat = np.zeros(NP, np.float32)
    for k, (o, s) in lay.items():
        fan = {"W1": 3, "b1": 3, "W2": H, "b2": H, "W3": n, "b3": n, "W4": H, "b4": H}.get(k, 1)
        flat[o:o + int(np.prod(s))] = rng.uniform(-1, 1, int(np.prod(s))) / np.sqrt(fan)
    flat.setflags(write=False)
    return flat


@functools.lru_cache(maxsize=None)
def _case(H, n, nch, mapped, B):
    """Inputs of one launch and its float64 rows: X (B, 3), abar (nch, n, B), the angle jets aj (mapped only, float32 of
    the reference's), rows (tiles, columns of W1 b1 W2 b2)."""
    rng = np.random.default_rng(7 * H + 31 * n + 101 * nch + 1009 * B + int(mapped))
    X = rng.random((B, 3)).astype(np.float32)
    abar = rng.standard_normal((nch, n, B)).astype(np.float32)
    P = R.unpack(_net(H, n), H, n, 3 * n)
    a = R.pre_jets(P, X, nch)
    if mapped:
        a = HR.angle_map_fwd(a)
    obj = (torch.from_numpy(abar).double() * a).sum(dim=(0, 1))
    rows = np.stack([np.concatenate([g.numpy().reshape(-1) for g in gr])
                     for gr in R.tile_grads(obj, [P[k] for k in NAMES], B)])
    assert rows.shape == ((B + 63) // 64, _n_cols(H, n)) and np.isfinite(rows).all()
    aj = a.detach().numpy().astype(np.float32) if mapped else None
    for arr in (X, abar, rows) + ((aj,) if mapped else ()):
        arr.setflags(write=False)
    return X, abar, aj, rows


def _poisoned(arr, dev):
    """The array, flat, on the device, with 64 NaNs behind it."""
    t = S._nan(dev, arr.size + 64)
    t[:arr.size] = torch.from_numpy(np.array(arr)).reshape(-1).to(dev)       # (a writable copy of the cached array)
    return t


def _compare(tag, got, want):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    scale = max(1.0, np.abs(want).max())
    err = np.abs(got.astype(np.float64) - want).max() / (ROW_TOL * scale)
    print(f"{tag}: error / tolerance {err:.3f} (max |reference| {np.abs(want).max():.3g})")
    assert np.abs(want).max() > 100 * ROW_TOL, tag          # the comparison is not vacuous
    assert err < 1.0, (tag, err)


def test_shapes_reach_both_sides_of_the_chunking():
    """No GPU: the block geometry of hidden_geometry (csrc/qc_mlp.hip) at the widths above."""
    def geometry(H, target=256):
        if H <= target:
            HB, PS = H, min(64, target // H)
        else:
            HB = 64 * ((H + 63) // 64)
            ps = 1024 // HB
            PS = 4 if ps >= 4 else (2 if ps >= 2 else 1)
        return HB, PS, 64 * ((HB * PS + 63) // 64)
    assert geometry(7) == (7, 36, 256) and geometry(50) == (50, 5, 256)
    assert geometry(129) == (129, 1, 192) and geometry(300) == (320, 2, 640)
    # rows per wave of a six-channel tile (3 n channel pairs) against the chunk of four: below, at and above it
    per_wave = {(H, n): -(-3 * n // (geometry(H)[2] // 64)) for H, n in CASES}
    assert min(per_wave.values()) == 1 and 4 in per_wave.values() and max(per_wave.values()) == 5
    assert {b % 64 for b in BATCHES} == {1, 63} and {(b + 63) // 64 for b in BATCHES} == {1, 2, 3}
    assert {r for r, _ in STAGE_SHAPES} == set(BATCHES) == {v for _, v in STAGE_SHAPES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_standalone_pre_backward(case, gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    dev = gpu_device
    st = torch.cuda.current_stream(dev).cuda_stream
    H, n = case
    n_theta = 3 * n
    NP = R.layout(H, n, n_theta)[1]
    cols = np.arange(_n_cols(H, n))
    prm = torch.from_numpy(_net(H, n).copy()).to(dev)
    for nch in (1, 6):
        for mapped in (False, True):
            for B in BATCHES:
                X, abar, aj, want = _case(H, n, nch, mapped, B)
                Xd = torch.from_numpy(X.copy()).to(dev)
                abar_d = _poisoned(abar, dev)
                part = S._nan(dev, S.ROW0 + (B + 63) // 64 + 2, NP + 3 + S.STRIDE_PAD)
                if mapped:
                    aj_d = _poisoned(aj, dev)
                    L.check(lib.qc_pre_backward_map(Xd.data_ptr(), prm.data_ptr(), H, n, n_theta, L.QC_ANGLE_MAP_TANH_PI,
                                                    aj_d.data_ptr(), abar_d.data_ptr(), part.data_ptr(), part.shape[1],
                                                    S.ROW0, B, nch, st), "qc_pre_backward_map")
                else:
                    L.check(lib.qc_pre_backward(Xd.data_ptr(), prm.data_ptr(), H, n, n_theta, abar_d.data_ptr(),
                                                part.data_ptr(), part.shape[1], S.ROW0, B, nch, st), "qc_pre_backward")
                torch.cuda.synchronize(dev)
                got = S._rows(part, B, cols, NP)        # finite inside, NaN everywhere else
                _compare(f"stand-alone H{H} n{n} nch{nch} map{int(mapped)} B{B}", got, want)


def _step(dev, H, n, mapped, B_res, B_val):
    circuits, engine, L = pkg("circuits"), pkg("hip.engine"), pkg("hip.lib")
    prog = circuits.build_program("cascade", n, 1, False)
    assert prog.n_params == 3 * n
    circ = engine.Circuit(prog, None, dev, angle_map=L.QC_ANGLE_MAP_TANH_PI if mapped else L.QC_ANGLE_MAP_NONE)
    eng = engine.SolverEngine(circ, H, torch.from_numpy(_net(H, n).copy()).to(dev))
    n_ic = (B_val + 1) // 2
    return eng, engine.FusedStep(eng, B_res, n_ic, B_val - n_ic, engine.OptimState(eng.NP, 0.005, dev))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_merged_stage_pre_backward(case, gpu_device):
    L = pkg("hip.lib")
    dev = gpu_device
    st = torch.cuda.current_stream(dev).cuda_stream
    H, n = case
    n_own = _n_cols(H, n)
    for mapped in (False, True):
        for B_res, B_val in STAGE_SHAPES:
            Xr, abr, ajr, want_r = _case(H, n, 6, mapped, B_res)
            Xv, abv, ajv, want_v = _case(H, n, 1, mapped, B_val)
            eng, fs = _step(dev, H, n, mapped, B_res, B_val)
            for buf in (fs.part, fs.ws_res, fs.ws_val):
                buf.fill_(float("nan"))
            fs.X_res[:B_res] = torch.from_numpy(Xr.copy()).to(dev)
            fs.X_val[:B_val] = torch.from_numpy(Xv.copy()).to(dev)
            fs.ws_res[3].copy_(torch.from_numpy(abr.copy()).to(dev))
            fs.ws_val[3].copy_(torch.from_numpy(abv.copy()).to(dev).reshape(1, n, B_val))
            if mapped:
                fs.ws_res[0].copy_(torch.from_numpy(ajr.copy()).to(dev))
                fs.ws_val[0].copy_(torch.from_numpy(ajv.copy()).to(dev).reshape(1, n, B_val))
            assert eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_PRE_BWD, st) == 0   # the merged form serves it
            torch.cuda.synchronize(dev)
            part = fs.part.cpu().numpy()
            rows_res = (B_res + 63) // 64
            assert part.shape == (rows_res + (B_val + 63) // 64, eng.NP + 3)
            assert np.isfinite(part[:, :n_own]).all(), "the stage left part of its columns unwritten (or non-finite)"
            assert np.isnan(part[:, n_own:]).all(), "the stage wrote outside its columns"
            tag = f"stage 4 H{H} n{n} map{int(mapped)} r{B_res} v{B_val}"
            _compare(tag + " residual tiles", part[:rows_res, :n_own], want_r)
            _compare(tag + " value tiles", part[rows_res:, :n_own], want_v)
