"""qc_gradnorm_fold on synthetic row matrices: the class fold and the combination launch without a model.

(a) the class sums against float64 within the bound of their own summation, (n_c - 1) 2^-24 sum_rows |x| per column (every
partial sum of n_c terms is bounded by the sum of the magnitudes, and a chain of any shape over n_c terms rounds at most
n_c - 1 times); (b) from the device's own class sums, the record to 2^-22 relative and the combination to 2^-23 relative
per entry against the float32 restatement (tests/gradnorm_reference.py); (c) the update period; (d) edge values; (e)
bit-reproducibility; (f) nothing outside the survivors' rows and the first ncols columns is written."""
import ctypes as C

import numpy as np
import pytest
import torch

import gradnorm_reference as GR
from conftest import pkg

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)


class Fold:
    """A record, its history and the two launches on a copy of ``part``."""

    def __init__(self, dev, cap=8, **cfg):
        self.L = pkg("hip.lib")
        self.lib, self.dev = self.L.load(), dev
        self.cfg = dict(dict(alpha=0.5, every=1, lam_max=1e4, init=(1.0, 1.0)), **cfg)
        c = self.cfg
        self.state = torch.full((self.L.QC_GRADNORM_STATE_WORDS,), NAN, dtype=torch.float32, device=dev)
        self.hist = torch.full((cap, self.L.QC_GRADNORM_HIST_COLS), NAN, dtype=torch.float32, device=dev)
        self.gn = self.L.QcStepGradnorm(c["alpha"], c["lam_max"], c["every"], c["init"][0], c["init"][1], self.state.data_ptr(),
                                        self.hist.data_ptr(), cap)
        self.L.check(self.lib.qc_gradnorm_init(self.state.data_ptr(), C.byref(self.gn), _stream(dev)), "qc_gradnorm_init")

    def run(self, part, n_res, n_ic, n_bc, ncols, classes=True):
        rows, stride = part.shape
        assert rows == n_res + n_ic + n_bc
        p = _dev(part, self.dev)
        flat = torch.full((ncols + 5,), NAN, dtype=torch.float32, device=self.dev)
        cls = torch.full((3, ncols), NAN, dtype=torch.float32, device=self.dev)
        self.L.check(self.lib.qc_gradnorm_fold(p.data_ptr(), rows, n_res, n_ic, stride, ncols, C.byref(self.gn), flat.data_ptr(),
                                               cls.data_ptr() if classes else None, _stream(self.dev)), "qc_gradnorm_fold")
        torch.cuda.synchronize(self.dev)
        return flat.cpu().numpy(), cls.cpu().numpy(), p.cpu().numpy()

    def read(self):
        raw = self.state.cpu().numpy()
        i = raw.view(np.int32)
        return {"lam_bc": raw[0], "lam_ic": raw[1], "n_steps": int(i[2]), "hist_base": int(i[3]), "n_updates": int(i[4]),
                "m_r": raw[5], "a_bc": raw[6], "a_ic": raw[7], "hat_bc": raw[8], "hat_ic": raw[9], "pad": raw[10:]}


def _matrix(n_res, n_ic, n_bc, ncols, stride, seed):
    """Rows of the three classes at different scales (so that the weights move far from 1), loss columns non-negative."""
    g = np.random.default_rng(seed)
    part = g.standard_normal((n_res + n_ic + n_bc, stride)).astype(np.float32)
    part[n_res:n_res + n_ic] *= 0.02
    part[n_res + n_ic:] *= 0.1
    part[:, ncols - 3:ncols] = np.abs(part[:, ncols - 3:ncols])
    return part


def _close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (rel * np.maximum(np.abs(want), 1e-30))).max())


# rows per class (residual, IC, BC) in mixed combinations of {0, 1, 31, 32, 33, 70, 300}; ncols on both sides of 3 * 1024
SHAPES = [((1, 0, 1), 67), ((31, 32, 33), 67), ((33, 1, 70), 703), ((300, 70, 31), 703), ((70, 0, 300), 3072), ((32, 33, 0), 3072),
          ((2, 1, 2), 3073), ((300, 31, 70), 3073), ((33, 300, 32), 5000), ((0, 70, 33), 67), ((1, 1, 1), 3072)]


@pytest.mark.parametrize("rows,ncols", SHAPES, ids=[f"{r[0]}_{r[1]}_{r[2]}x{c}" for r, c in SHAPES])
def test_class_sums_record_and_combination(rows, ncols, gpu_device):
    n_res, n_ic, n_bc = rows
    stride = ncols + 9
    part = _matrix(n_res, n_ic, n_bc, ncols, stride, seed=ncols + 7 * n_res + n_ic)
    f = Fold(gpu_device)
    flat, cls, after = f.run(part, n_res, n_ic, n_bc, ncols)
    # (a) the class sums
    want = GR.class_sums(part, n_res, n_ic, n_bc, ncols)
    cut = (0, n_res, n_res + n_ic, n_res + n_ic + n_bc)
    worst = 0.0
    for c in range(3):
        n_c = cut[c + 1] - cut[c]
        bound = max(n_c - 1, 0) * 2.0 ** -24 * np.abs(part[cut[c]:cut[c + 1], :ncols].astype(np.float64)).sum(0)
        err = np.abs(cls[c].astype(np.float64) - want[c])
        assert (err <= bound).all(), (c, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if n_c > 1 else 0.0)
    # (b) record and combination from the device's own class sums
    r = GR.Record(**f.cfg)
    ref = r.step(cls, n_ic, n_bc)
    st, want_st = f.read(), r.state()
    rec_err = max(_close(st[k], want_st[k], 2.0 ** -22) for k in ("lam_bc", "lam_ic", "m_r", "a_bc", "a_ic", "hat_bc", "hat_ic")
                  if want_st[k] != 0.0)
    assert all(st[k] == 0.0 for k in ("lam_bc", "lam_ic", "m_r", "a_bc", "a_ic", "hat_bc", "hat_ic") if want_st[k] == 0.0)
    NP = ncols - 3
    nz = ref[:NP] != 0
    flat_err = _close(flat[:NP][nz], ref[:NP][nz], 2.0 ** -23)
    print(rows, ncols, "class sums: largest error / bound", worst, "record error / 2^-22", rec_err, "flat error / 2^-23", flat_err,
          "lam", st["lam_bc"], st["lam_ic"])
    assert rec_err <= 1.0 and flat_err <= 1.0
    assert np.array_equal(flat[NP:ncols], (cls[0, NP:] + cls[1, NP:]) + cls[2, NP:])          # the unscaled loss columns
    assert (st["n_steps"], st["hist_base"], st["n_updates"]) == (1, 0, 1) and (st["pad"] == 0).all()
    if n_res and n_ic and n_bc:
        assert st["lam_bc"] > 2.0 and st["lam_ic"] > 2.0        # the control: unit weights are far away
    h = f.hist.cpu().numpy()
    assert np.array_equal(h[0, :5], [st["lam_bc"], st["lam_ic"], st["m_r"], st["a_bc"], st["a_ic"]]) and h[0, 6] == 1.0
    assert h[0, 5] == pytest.approx(r.history()[0, 5], rel=1e-5) and np.isnan(h[1:]).all()
    # (f) only the survivors' rows, and only the first ncols columns; flat behind ncols untouched
    assert np.isnan(flat[ncols:]).all()
    assert np.array_equal(after[:, ncols:], part[:, ncols:])
    keep = np.ones(len(part), bool)
    for c in range(3):
        keep[cut[c]:cut[c] + min(cut[c + 1] - cut[c], 32)] = False
    assert np.array_equal(after[keep], part[keep])
    # (e) a second run on a fresh record is bit-identical; class_out = NULL changes nothing
    f2 = Fold(gpu_device)
    flat2, cls2, after2 = f2.run(part, n_res, n_ic, n_bc, ncols)
    f3 = Fold(gpu_device)
    flat3, _, _ = f3.run(part, n_res, n_ic, n_bc, ncols, classes=False)
    for a, b in ((flat[:ncols], flat2[:ncols]), (cls, cls2), (after, after2), (f.state.cpu().numpy(), f2.state.cpu().numpy()),
                 (f.hist.cpu().numpy()[:1], f2.hist.cpu().numpy()[:1]), (flat[:ncols], flat3[:ncols]),
                 (f.state.cpu().numpy(), f3.state.cpu().numpy())):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_weights_move_every_second_call(gpu_device):
    """(c) five calls with every = 2: the weights move on calls 0, 2 and 4 only; history and counters are the restatement's."""
    n_res, n_ic, n_bc, ncols = 33, 2, 5, 131
    f = Fold(gpu_device, alpha=0.3, every=2)
    r = GR.Record(**f.cfg)
    lam = []
    for call in range(5):
        part = _matrix(n_res, n_ic, n_bc, ncols, ncols + 1, seed=50 + call)
        flat, cls, _ = f.run(part, n_res, n_ic, n_bc, ncols)
        ref = r.step(cls, n_ic, n_bc)
        assert _close(flat[:ncols - 3], ref[:ncols - 3], 2.0 ** -23) <= 1.0
        lam.append((f.read()["lam_bc"], f.read()["lam_ic"]))
    st, h, want = f.read(), f.hist.cpu().numpy().astype(np.float64), r.history()
    assert (st["n_steps"], st["n_updates"]) == (5, 3) == (r.n_steps, r.n_updates)
    assert h[:5, 6].tolist() == [1.0, 0.0, 1.0, 0.0, 1.0] and np.isnan(h[5:]).all()
    assert lam[0] == lam[1] and lam[2] == lam[3] and len({lam[0], lam[2], lam[4]}) == 3
    err = float((np.abs(h[:5, :6] - want[:, :6]) / (2.0 ** -22 * np.abs(want[:, :6]))).max())
    print("history error / 2^-22", err, "lam", lam)
    assert err <= 4.0          # a history entry is a float32 of a double the restatement forms from float32 inputs: 2^-22, and
    #                            the lambda-weighted loss passes through three float32 roundings more
    assert np.array_equal(h[1, 2:5], h[0, 2:5]) and not np.array_equal(h[2, 2:5], h[0, 2:5])      # statistics of the last update


def test_edge_values(gpu_device):
    """(d) alpha = 0, the clamp, an all-zero BC class, a NaN in the residual class."""
    n_res, n_ic, n_bc, ncols = 3, 2, 2, 70
    part = _matrix(n_res, n_ic, n_bc, ncols, ncols, seed=9)
    f = Fold(gpu_device, alpha=0.0)
    flat, cls, _ = f.run(part, n_res, n_ic, n_bc, ncols)
    st = f.read()
    assert (st["lam_bc"], st["lam_ic"]) == (1.0, 1.0) and st["n_updates"] == 1 and st["m_r"] > 0
    assert np.array_equal(flat[:ncols - 3], ((cls[0] + cls[2]) + cls[1])[:ncols - 3])      # fmaf with weight 1: plain sums
    f = Fold(gpu_device, alpha=1.0, lam_max=1.5)
    f.run(part, n_res, n_ic, n_bc, ncols)
    assert (f.read()["lam_bc"], f.read()["lam_ic"]) == (1.5, 1.5) and f.read()["hat_bc"] > 1.5
    zero = part.copy()
    zero[n_res + n_ic:, :ncols - 3] = 0.0
    f = Fold(gpu_device, init=(3.0, 1.0))
    flat, cls, _ = f.run(zero, n_res, n_ic, n_bc, ncols)
    st = f.read()
    assert st["lam_bc"] == 3.0 and st["a_bc"] == 0.0 and st["hat_bc"] == 0.0 and st["lam_ic"] > 2.0 and np.isfinite(flat[:ncols]).all()
    bad = part.copy()
    bad[1, 5] = NAN
    f = Fold(gpu_device, init=(3.0, 2.0))
    flat, cls, _ = f.run(bad, n_res, n_ic, n_bc, ncols)
    st = f.read()
    assert (st["lam_bc"], st["lam_ic"]) == (3.0, 2.0) and np.isnan(st["m_r"]) and st["hat_ic"] == 0.0 and st["n_updates"] == 1
    assert np.isnan(flat[5]) and np.isfinite(np.delete(flat[:ncols], 5)).all()
    # a NaN in the last wave's share of the columns is kept through the block's reduction as well
    wide = _matrix(2, 1, 1, 3072, 3072, seed=4)
    wide[0, 3068] = NAN
    f = Fold(gpu_device)
    f.run(wide, 2, 1, 1, 3072)
    assert (f.read()["lam_bc"], f.read()["lam_ic"]) == (1.0, 1.0) and np.isnan(f.read()["m_r"])
