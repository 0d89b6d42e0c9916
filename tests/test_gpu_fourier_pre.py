"""qc_pre_forward_ff / qc_pre_backward_ff (csrc/qc_mlp.hip, k_pre_ff_fwd / k_pre_ff_bwd) against the float64 reference of
tests/fourier_reference.py, at the smallest shapes that reach each boundary of the kernels:

  m      1, 3, 8, 17, 64   3: waves with no frequency of their own; 17: one past a block of 16 and of 8; 64: the maximum
  H      1, 5, 50, 65      1: waves without units; 65: past a wave
  n      2, 4, 8, 9        9: the unbatched loops
  B      1, 63, 64, 65, 130
  nch    1, 6;  angle map off and on;  scale 1, 10

Not the full product: every value of every parameter at least once, and the pairs (m = 64, H = 65, n = 8) and (m = 1, H = 1).

Memory safety: every output buffer is NaN-filled with a sentinel behind it, and the partial matrix is NaN-filled with a row
offset and a padded stride; a launch must write exactly its own rows and columns.

Tolerance, per channel and per gradient block, measured per case: 4 x the distance between the float32 torch restatement
and the float64 reference on the same fp32 inputs (a correct fp32 kernel differs from another correct fp32 evaluation by a
small multiple of their distance to the truth: the rule of tests/test_gpu_lbfgs_kernel.py), and never less than four fp32
ulps of the quantity's largest magnitude.  Control: the reference with the last frequency's two weight columns zeroed
must miss by at least 100 tolerances in every checked quantity (b2's gradient without the angle map is the sum of the value
cotangents, which no frequency reaches: it is checked but has no control).

Gradients: the partial rows summed over the tiles against the float64 gradient of sum(abar * ajets), as
tests/test_gpu_mlp_shapes.py does tile by tile."""
import numpy as np
import pytest
import torch

import fourier_reference as FR
from conftest import pkg

pytestmark = pytest.mark.gpu

ROW0, STRIDE_PAD, N_THETA = 2, 7, 3
GRAD_NAMES = ("W1", "b1", "W2", "b2")

# (m, H, n, B, scale)
CASES = [(1, 1, 2, 1, 1.0), (3, 5, 4, 63, 10.0), (8, 50, 9, 65, 1.0), (17, 50, 4, 64, 10.0), (64, 65, 8, 130, 1.0),
         (17, 5, 2, 130, 1.0)]


def _ids(c):
    return "m{}_H{}_n{}_B{}_s{:g}".format(*c)


def _inputs(case):
    m, H, n, B, scale = case
    rng = np.random.default_rng(1000 * m + 10 * H + n + B)
    Bf = (rng.standard_normal((3, m)) * scale).astype(np.float32)
    X = rng.random((B, 3)).astype(np.float32)
    lay, NP = FR.layout(H, n, N_THETA, 2 * m)
    flat = np.empty(NP, np.float32)
    for k, (o, s) in lay.items():
        fan = {"W1": 2 * m, "b1": 2 * m, "W2": H, "b2": H}.get(k, 1)
        flat[o:o + int(np.prod(s))] = rng.uniform(-1, 1, int(np.prod(s))) / np.sqrt(fan)
    flat[lay["W3"][0]:] = np.nan            # the pre stages read nothing behind b2
    return Bf, X, flat, lay, NP


def _reference(case, nch, mapped, abar, drop_freq=False, dtype=torch.float64):
    """(angle jets (nch, n, B), {block: gradient of sum(abar * ajets)}) in ``dtype`` on the fp32 inputs."""
    m, H, n, B, _ = case
    Bf, X, flat, lay, NP = _inputs(case)
    P = FR.unpack(np.nan_to_num(flat), H, n, N_THETA, m, dtype=dtype)
    a = FR.pre_jets_ff(P, torch.tensor(Bf, dtype=dtype), torch.tensor(X, dtype=dtype), nch, drop_freq, angle_map=mapped)
    g = torch.autograd.grad((torch.tensor(abar, dtype=dtype) * a).sum(), [P[k] for k in GRAD_NAMES], allow_unused=True)
    grads = {k: (torch.zeros_like(P[k]) if gi is None else gi).double().numpy().reshape(-1) for k, gi in zip(GRAD_NAMES, g)}
    return a.detach().double().numpy(), grads


@pytest.mark.parametrize("mapped", [False, True], ids=["plain", "tanh_pi"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_pre_ff_forward_and_backward(case, mapped, gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    dev = gpu_device
    st = torch.cuda.current_stream(dev).cuda_stream
    m, H, n, B, scale = case
    Bf, X, flat, lay, NP = _inputs(case)
    amap = L.QC_ANGLE_MAP_TANH_PI if mapped else L.QC_ANGLE_MAP_NONE
    Xd, prm, fq = (torch.from_numpy(a).to(dev) for a in (X, flat, Bf))
    tiles = (B + 63) // 64
    cols = np.concatenate([np.arange(lay[k][0], lay[k][0] + int(np.prod(lay[k][1]))) for k in GRAD_NAMES])
    report = {}
    for nch in (1, 6):
        aj = torch.full((nch * n * B + 64,), float("nan"), dtype=torch.float32, device=dev)
        L.check(lib.qc_pre_forward_ff(Xd.data_ptr(), prm.data_ptr(), H, n, N_THETA, amap, fq.data_ptr(), m, aj.data_ptr(), B, nch,
                                      st), "qc_pre_forward_ff")
        abar = np.random.default_rng(B + nch).standard_normal((nch, n, B)).astype(np.float32)
        abar_d = torch.from_numpy(abar).to(dev)
        part = torch.full((ROW0 + tiles + 2, NP + 3 + STRIDE_PAD), float("nan"), dtype=torch.float32, device=dev)
        L.check(lib.qc_pre_backward_ff(Xd.data_ptr(), prm.data_ptr(), H, n, N_THETA, amap, fq.data_ptr(), m, aj.data_ptr(),
                                       abar_d.data_ptr(), part.data_ptr(), part.shape[1], ROW0, B, nch, st), "qc_pre_backward_ff")
        torch.cuda.synchronize(dev)
        # memory safety
        a_host = aj.cpu().numpy()
        assert np.isnan(a_host[nch * n * B:]).all(), "the forward stage wrote past its output"
        assert np.isfinite(a_host[:nch * n * B]).all(), "the forward stage left part of its output unwritten"
        p_host = part.cpu().numpy()
        own = np.zeros(p_host.shape, bool)
        own[ROW0:ROW0 + tiles, cols] = True
        assert np.isnan(p_host[~own]).all(), "the reverse stage wrote outside its rows / columns"
        assert np.isfinite(p_host[own]).all(), "the reverse stage left part of its rows / columns unwritten"
        got_a = a_host[:nch * n * B].reshape(nch, n, B).astype(np.float64)
        got_g = p_host[ROW0:ROW0 + tiles].astype(np.float64).sum(0)

        a64, g64 = _reference(case, nch, mapped, abar)
        a32, g32 = _reference(case, nch, mapped, abar, dtype=torch.float32)
        abad, gbad = _reference(case, nch, mapped, abar, drop_freq=True)
        checks = [(f"nch{nch} ch{c}", got_a[c], a64[c], a32[c], abad[c], True) for c in range(nch)]
        for k in GRAD_NAMES:
            o, s = lay[k]
            sl = slice(o, o + int(np.prod(s)))
            checks.append((f"nch{nch} d{k}", got_g[sl], g64[k], g32[k], gbad[k], not (k == "b2" and not mapped)))
        for name, got, want, f32, bad, has_control in checks:
            tol, gap = FR.gap_tolerance(f32, want)
            err = float(np.abs(got - want).max())
            miss = float(np.abs(got - bad).max())
            report[name] = (err / tol, gap, tol, miss / tol if has_control else float("inf"))
            print(f"{_ids(case)} map={int(mapped)} {name}: err {err:.3e} gap {gap:.3e} tol {tol:.3e} ratio {err / tol:.3f} "
                  f"control {miss / tol:.1f}")
    bad = {k: v for k, v in report.items() if not v[0] <= 1.0}
    assert not bad, bad
    weak = {k: v for k, v in report.items() if v[3] < 100.0}
    assert not weak, f"a lost frequency is not told apart by 100 tolerances: {weak}"


def test_out_of_range_arguments_write_nothing(gpu_device):
    """m outside 1 .. QC_FF_MAX, and the shape limits of the _map forms, are refused before any launch."""
    L = pkg("hip.lib")
    lib = L.load()
    dev = gpu_device
    st = torch.cuda.current_stream(dev).cuda_stream
    X, prm, fq = torch.rand(64, 3, device=dev), torch.zeros(20000, device=dev), torch.zeros(3 * 70, device=dev)
    aj = torch.full((6 * 4 * 64,), float("nan"), device=dev)
    for H, n, m in ((8, 4, 0), (8, 4, 65), (8, 17, 4), (1025, 4, 4)):
        rc = lib.qc_pre_forward_ff(X.data_ptr(), prm.data_ptr(), H, n, 0, 0, fq.data_ptr(), m, aj.data_ptr(), 64, 6, st)
        torch.cuda.synchronize(dev)
        assert rc == -1, (H, n, m, rc)
        assert torch.isnan(aj).all()
