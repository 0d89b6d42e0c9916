"""The network entry points (qc_pre_forward / qc_pre_backward / qc_post / qc_post_multi, csrc/qc_mlp.hip) at hidden
widths, qubit counts and batch tails the whole-model tests never reach, against the float64 reference of
tests/mlp_reference.py.  Random <Z> jets and angle-jet cotangents stand in for the circuit.

H covers both regimes of hidden_geometry (H <= 256 packed, H > 256 rounded to 64), both sides of the fused / split post
threshold (128), the edges of the four-wave hidden split (H < 4, H mod 4 != 0) and the growth of the dynamic LDS of
k_pre_bwd / k_post_wg (the large widths run at n = 16).  Every launch writes into NaN-filled buffers with row0 > 0 and a
padded row stride, and must write exactly its own rows and columns.

Tolerances, relative to max(1, max |ref|) of each compared array:
  POINT_TOL 5e-5  per-point outputs (jets, u, residual, qbar): fp32 sums over H <= 1024 terms of O(1) products plus the
                  ~1e-7 tanh approximation stay near 1e-6; 5e-5 leaves margin and is still far below the effect of
                  one dropped hidden unit or point (checked by the negative controls);
  ROW_TOL 2e-4    tile-summed weight-gradient rows and loss sums: 64 points x H terms in fp32 (the bound the solver tests
                  use for gradients).
Each case also runs two negative controls: the same comparison against the reference without hidden unit H - 1, and
against the reference without the batch's last point, must fail."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlp_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu

POINT_TOL = 5e-5
ROW_TOL = 2e-4
ROW0, STRIDE_PAD, N_THETA = 2, 7, 3

# (H, n, B): every H of the issue once; the large widths at n = 16 (the LDS worst case); B from 1 to a batch of
# 14 value tiles (4 blocks of the four-tiles-per-block value kernels, the last one partial)
CASES = [(1, 1, 65), (3, 2, 63), (5, 5, 1), (50, 8, 200), (63, 9, 64), (64, 2, 849), (65, 5, 65), (128, 16, 200),
         (129, 9, 63), (256, 16, 65), (257, 16, 200), (300, 8, 1), (1024, 16, 130)]
SAT = (50, 4, 200)          # weights scaled so |pre-activation| > 40: tanh saturates (exp overflow / underflow)


def _ids(c):
    return "H{}_n{}_B{}".format(*c)


def _params(H, n, seed, saturate=False):
    """Flat parameters with torch's default Linear scales (activations O(1)); theta and, for the K-output kernel, the
    W4 / b4 slots are NaN: the network kernels must not read them."""
    lay, NP = R.layout(H, n, N_THETA)
    rng = np.random.default_rng(seed)
    flat = np.empty(NP, np.float32)
    for k, (o, s) in lay.items():
        fan = {"W1": 3, "b1": 3, "W2": H, "b2": H, "W3": n, "b3": n, "W4": H, "b4": H}.get(k, 1)
        flat[o:o + int(np.prod(s))] = rng.uniform(-1, 1, int(np.prod(s))) / np.sqrt(fan)
    if saturate:        # |pre-activation| > 40 at every point and unit, both signs: exp(2x) overflows / underflows
        for k, b in (("W1", "b1"), ("W3", "b3")):
            o, s = lay[k]
            ob, sb = lay[b]
            flat[ob:ob + sb[0]] = np.where(rng.random(sb[0]) < 0.5, -1, 1) * (45.0 + 15 * rng.random(sb[0]))
            flat[o:o + int(np.prod(s))] *= 0.5
    flat[lay["theta"][0]:] = np.nan
    return flat


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _pde(B, problem=0):
    L = pkg("hip.lib")
    d = dict(D=0.01, vx=1.0, vy=1.0, c_t=1.3, c_x=0.7, c_y=-0.4, d_xx=0.02, d_yy=0.05, w_res=4.0 / B, inv_n_res=1.0 / B,
             w_val_a=0.3, w_val_b=0.7, inv_n_a=0.11, inv_n_b=0.13, problem=problem, n_seg_a=B // 3)
    return L.QcPde(**d), d


class Check:
    """Collects (got, want, tol) comparisons of one launch so that each reference (and its mutations) is judged by the
    same rule."""

    def __init__(self):
        self.items = []

    def add(self, name, got, want, tol):
        self.items.append((name, np.asarray(got, np.float64), np.asarray(want, np.float64), tol))

    def errors(self):
        out = []
        for name, got, want, tol in self.items:
            err = np.abs(got - want).max() if got.size else 0.0
            out.append((name, err, tol * max(1.0, np.abs(want).max() if want.size else 0.0)))
        return out


def _judge(make_check, caught):
    """make_check(mutation) -> Check; mutation in (None, 'unit', 'point').  The unmutated reference must pass; the
    mutations that fail somewhere are added to ``caught`` (each test asserts at its end that both were caught: a
    saturated network, for one, hides every hidden unit from the derivative channels, so not every launch can)."""
    errs = make_check(None).errors()
    bad = [e for e in errs if not e[1] <= e[2]]          # (NaN fails too)
    assert not bad, bad
    for mut in ("unit", "point"):
        if any(e[1] > e[2] for e in make_check(mut).errors()):
            caught.add(mut)


def _negative_controls_caught(caught):
    assert caught == {"unit", "point"}, f"the tolerance did not tell apart the mutated reference(s): {caught}"


def _mask(B, mut):
    m = torch.ones(B, dtype=torch.float64)
    if mut == "point":
        m[B - 1] = 0.0
    return m


def _rows(part, B, cols, NP):
    """Checks the NaN sentinel outside the launch's rows / columns; returns the launch's rows (tiles, len(cols))."""
    p = part.cpu().numpy()
    tiles = (B + 63) // 64
    mask = np.zeros(p.shape, bool)
    mask[ROW0:ROW0 + tiles, cols] = True
    assert np.isnan(p[~mask]).all(), "a launch wrote outside its rows / columns"
    assert np.isfinite(p[mask]).all(), "a launch left part of its rows / columns unwritten (or non-finite)"
    return p[ROW0:ROW0 + tiles][:, cols]


def _untouched(buf, n_written=0):
    a = buf.cpu().numpy().reshape(-1)
    assert np.isnan(a[n_written:]).all(), "a launch wrote past its output"
    assert np.isfinite(a[:n_written]).all(), "a launch left part of its output unwritten (or non-finite)"
    return a[:n_written]


def _setup(case, seed, saturate=False):
    H, n, B = case
    g = np.random.default_rng(seed + 1)
    X = g.random((B, 3)).astype(np.float32)
    q = np.concatenate([g.uniform(-1, 1, (1, n, B)), g.standard_normal((5, n, B))]).astype(np.float32)
    flat = _params(H, n, seed, saturate)
    return H, n, B, X, q, flat


def _layout_cols(H, n, names):
    lay, NP = R.layout(H, n, N_THETA)
    cols = []
    for k in names:
        o, s = lay[k]
        cols.extend(range(o, o + int(np.prod(s))))
    return np.array(cols), NP


def _tile_rows(obj, wrt, names, H, n, B):
    """Per-tile flat gradient rows (tiles, NP) of a per-point objective."""
    rows = []
    for gr in R.tile_grads(obj, wrt, B):
        rows.append(R.flatten(dict(zip(names, gr)), H, n, N_THETA))
    return np.stack(rows)


# ------------------------------------------------------------------ pre network
@pytest.mark.parametrize("case", CASES + [SAT], ids=[_ids(c) for c in CASES] + ["saturated"])
def test_pre_network_forward_and_backward(case, gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    H, n, B, X, _, flat = _setup(case, seed=sum(case), saturate=case is SAT)
    dev = gpu_device
    caught = set()
    Xd, prm = torch.from_numpy(X).to(dev), torch.from_numpy(flat).to(dev)
    names = ("W1", "b1", "W2", "b2")
    cols, NP = _layout_cols(H, n, names)
    for nch in (1, 6):
        aj = _nan(dev, nch * n * B + 64)
        L.check(lib.qc_pre_forward(Xd.data_ptr(), prm.data_ptr(), H, n, N_THETA, aj.data_ptr(), B, nch, st), "qc_pre_forward")
        abar = np.random.default_rng(B + nch).standard_normal((nch, n, B)).astype(np.float32)
        part = _nan(dev, ROW0 + (B + 63) // 64 + 2, NP + 3 + STRIDE_PAD)
        abar_d = torch.from_numpy(abar).to(dev)
        L.check(lib.qc_pre_backward(Xd.data_ptr(), prm.data_ptr(), H, n, N_THETA, abar_d.data_ptr(),
                                    part.data_ptr(), part.shape[1], ROW0, B, nch, st), "qc_pre_backward")
        torch.cuda.synchronize(dev)
        got_a = _untouched(aj, nch * n * B).reshape(nch, n, B)
        got_rows = _rows(part, B, cols, NP)

        def make(mut):
            P = R.unpack(flat, H, n, N_THETA)
            m = _mask(B, mut)
            a = R.pre_jets(P, X, nch, drop_unit=mut == "unit") * m
            obj = (torch.from_numpy(abar).double() * a).sum(dim=(0, 1))
            rows = _tile_rows(obj, [P[k] for k in names], names, H, n, B)[:, cols]
            c = Check()
            c.add(f"ajets nch={nch}", got_a, a.detach().numpy(), POINT_TOL)
            c.add(f"pre rows nch={nch}", got_rows, rows, ROW_TOL)
            return c
        _judge(make, caught)
    _negative_controls_caught(caught)


# ------------------------------------------------------------------ post network, single output
def _post_modes():
    return [(0, 1), (0, 6), (1, 1), (1, 6), (2, 1), (2, 6), (3, 6), (4, 6)]


@pytest.mark.parametrize("case", CASES + [SAT], ids=[_ids(c) for c in CASES] + ["saturated"])
def test_post_network_every_mode(case, gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    H, n, B, X, q6, flat = _setup(case, seed=3 * sum(case), saturate=case is SAT)
    dev = gpu_device
    caught = set()
    Xd, prm = torch.from_numpy(X).to(dev), torch.from_numpy(flat).to(dev)
    names = ("W3", "b3", "W4", "b4")
    cols, NP = _layout_cols(H, n, names)
    rng = np.random.default_rng(B)
    for mode, nch in _post_modes():
        for problem in ((0, 1) if mode == 2 else (0,)):
            qpde, pde = _pde(B, problem)
            q = q6[:nch].copy()
            qd = torch.from_numpy(q).to(dev)
            nu = 6 if mode in (3, 4) else 1
            out_u, out_res = _nan(dev, nu * B + 64), _nan(dev, B + 64)
            qbar = _nan(dev, nch * n * B + 64)
            part = _nan(dev, ROW0 + (B + 63) // 64 + 2, NP + 3 + STRIDE_PAD)
            ubar = rng.standard_normal((6 if mode == 3 else 1, B)).astype(np.float32)
            rbar = rng.standard_normal(B).astype(np.float32)
            ub_d, rb_d = torch.from_numpy(ubar).to(dev), torch.from_numpy(rbar).to(dev)
            L.check(lib.qc_post(mode, Xd.data_ptr(), prm.data_ptr(), H, n, N_THETA, C.byref(qpde), qd.data_ptr(),
                                out_u.data_ptr(), out_res.data_ptr(), ub_d.data_ptr(), rb_d.data_ptr() if nch == 6 else None,
                                qbar.data_ptr(), part.data_ptr(), part.shape[1], ROW0, B, nch, st), f"qc_post mode {mode}")
            torch.cuda.synchronize(dev)
            wcols = {0: [], 4: []}.get(mode, list(cols) + ([NP, NP + 1, NP + 2] if mode == 2 else []))
            got_rows = _rows(part, B, np.array(wcols, int), NP) if wcols else None
            if not wcols:
                assert np.isnan(part.cpu().numpy()).all()
            got_u = _untouched(out_u, {0: B, 2: B, 4: 6 * B}.get(mode, 0))
            got_r = _untouched(out_res, B if (nch == 6 and mode in (0, 2)) else 0)
            got_qb = _untouched(qbar, nch * n * B if mode in (1, 2, 3) else 0)

            def make(mut):
                P = R.unpack(flat, H, n, N_THETA)
                qt = torch.from_numpy(q).double().requires_grad_(True)
                m = _mask(B, mut)
                u = R.post_jets(P, qt, drop_unit=mut == "unit")
                c = Check()
                tag = f"mode {mode} nch {nch} problem {problem}"
                if mode in (0, 4):
                    if mode == 4:
                        c.add("u jets " + tag, got_u.reshape(6, B), (u * m).detach().numpy(), POINT_TOL)
                    else:
                        c.add("u " + tag, got_u, (u[0] * m).detach().numpy(), POINT_TOL)
                        if nch == 6:
                            res = R.residual(u, (pde["c_t"], pde["c_x"], pde["c_y"], pde["d_xx"], pde["d_yy"]))
                            c.add("residual " + tag, got_r, (res * m).detach().numpy(), POINT_TOL)
                    return c
                if mode == 1:
                    obj = torch.from_numpy(ubar[0]).double() * u[0]
                    if nch == 6:
                        obj = obj + torch.from_numpy(rbar).double() * R.residual(
                            u, (pde["c_t"], pde["c_x"], pde["c_y"], pde["d_xx"], pde["d_yy"]))
                elif mode == 3:
                    obj = (torch.from_numpy(ubar).double() * u).sum(0)
                else:   # mode 2: gradient of sum_p w_p e_p^2 / 2, loss sums per tile
                    e = R.point_errors(u, X, pde, nch) * m
                    w = R.point_weights(B, pde, nch)
                    obj = 0.5 * w * e * e
                    cot = (w * e).detach().numpy()
                    if nch == 6:
                        c.add("residual cotangent " + tag, got_r, cot, POINT_TOL)
                        c.add("u cotangent " + tag, got_u, np.zeros(B), POINT_TOL)
                    else:
                        c.add("u cotangent " + tag, got_u, cot, POINT_TOL)
                    losses = np.stack([R.loss_parts(e[k:k + 64], dict(pde, n_seg_a=pde["n_seg_a"] - k), nch).detach().numpy()
                                       for k in range(0, B, 64)])
                    c.add("loss sums " + tag, got_rows[:, -3:], losses, ROW_TOL)
                obj = obj * m
                qb = torch.autograd.grad(obj.sum(), qt, retain_graph=True)[0]
                c.add("qbar " + tag, got_qb.reshape(nch, n, B), qb.numpy(), POINT_TOL)
                rows = _tile_rows(obj, [P[k] for k in names], names, H, n, B)[:, cols]
                c.add("post rows " + tag, got_rows[:, :len(cols)], rows, ROW_TOL)
                return c
            _judge(make, caught)
    _negative_controls_caught(caught)


# ------------------------------------------------------------------ post network, K outputs
@pytest.mark.parametrize("case", [c for c in CASES if c[2] > 1][::2] + [(300, 8, 1)], ids=_ids)
def test_post_multi_modes(case, gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    H, n, B, X, q, flat = _setup(case, seed=5 * sum(case))
    lay, NP = R.layout(H, n, N_THETA)
    flat = flat.copy()
    flat[lay["W4"][0]:lay["b4"][0] + 1] = np.nan            # the single-output slots are not read
    dev = gpu_device
    caught = set()
    prm, qd = torch.from_numpy(flat).to(dev), torch.from_numpy(q).to(dev)
    cols3, _ = _layout_cols(H, n, ("W3", "b3"))
    cols4, _ = _layout_cols(H, n, ("W4", "b4"))
    rng = np.random.default_rng(H)
    for K in (1, 2, 4):
        w4k = (rng.uniform(-1, 1, (K, H + 1)) / np.sqrt(H)).astype(np.float32)
        ubar = rng.standard_normal((K, 6, B)).astype(np.float32)
        w4d, ubd = torch.from_numpy(w4k).to(dev), torch.from_numpy(ubar).to(dev)
        out = _nan(dev, K * 6 * B + 64)
        L.check(lib.qc_post_multi(4, prm.data_ptr(), H, n, N_THETA, K, w4d.data_ptr(), qd.data_ptr(), out.data_ptr(),
                                  None, None, None, 0, None, 0, 0, B, st), "qc_post_multi mode 4")
        qbar = _nan(dev, 6 * n * B + 64)
        part = _nan(dev, ROW0 + (B + 63) // 64 + 2, NP + 3 + STRIDE_PAD)
        partk = _nan(dev, ROW0 + (B + 63) // 64 + 2, K * (H + 1) + STRIDE_PAD)
        L.check(lib.qc_post_multi(3, prm.data_ptr(), H, n, N_THETA, K, w4d.data_ptr(), qd.data_ptr(), None, ubd.data_ptr(),
                                  qbar.data_ptr(), part.data_ptr(), part.shape[1], partk.data_ptr(), partk.shape[1], ROW0, B,
                                  st), "qc_post_multi mode 3")
        torch.cuda.synchronize(dev)
        got_u = _untouched(out, K * 6 * B).reshape(K, 6, B)
        got_qb = _untouched(qbar, 6 * n * B).reshape(6, n, B)
        got_rows = _rows(part, B, np.concatenate([cols3, cols4]), NP)
        assert (got_rows[:, len(cols3):] == 0).all(), "the W4 / b4 columns of the shared row must be zero"
        got_k = _rows(partk, B, np.arange(K * (H + 1)), NP)

        def make(mut):
            P = R.unpack(np.nan_to_num(flat), H, n, N_THETA)
            qt = torch.from_numpy(q).double().requires_grad_(True)
            w4 = torch.from_numpy(w4k).double().requires_grad_(True)
            m = _mask(B, mut)
            u = R.post_jets(P, qt, drop_unit=mut == "unit", w4=w4[:, :H], b4=w4[:, H]) * m
            obj = (torch.from_numpy(ubar).double() * u).sum(dim=(0, 1))
            c = Check()
            c.add(f"u jets K={K}", got_u, u.detach().numpy(), POINT_TOL)
            c.add(f"qbar K={K}", got_qb, torch.autograd.grad(obj.sum(), qt, retain_graph=True)[0].numpy(), POINT_TOL)
            rows = _tile_rows(obj, [P["W3"], P["b3"]], ("W3", "b3"), H, n, B)[:, cols3]
            c.add(f"shared rows K={K}", got_rows[:, :len(cols3)], rows, ROW_TOL)
            rk = np.stack([g[0].numpy().reshape(-1) for g in R.tile_grads(obj, [w4], B)])
            c.add(f"last-layer rows K={K}", got_k, rk, ROW_TOL)
            return c
        _judge(make, caught)
    _negative_controls_caught(caught)


def test_out_of_range_shapes_are_refused_before_launch(gpu_device):
    """n = 17 and H = 1025 lie outside every kernel instance: the entry points refuse them with QC_ERR_ARG and write
    nothing."""
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    dev = gpu_device
    for H, n in ((50, 17), (1025, 4), (0, 4)):
        NP = max(R.layout(max(H, 1), n, N_THETA)[1], 1)
        X, prm = torch.rand(64, 3, device=dev), torch.zeros(NP, device=dev)
        aj = _nan(dev, 6 * n * 64)
        rc = lib.qc_pre_forward(X.data_ptr(), prm.data_ptr(), H, n, N_THETA, aj.data_ptr(), 64, 6, st)
        torch.cuda.synchronize(dev)
        assert rc != 0, rc
        assert torch.isnan(aj).all()


# ------------------------------------------------------------------ settings read once at library load: child processes
ENV_SELECTION = "(H1_n1_B65 or H129_n9_B63 or H1024_n16_B130 or step_H65_B830 or step_H257) and not env_variants"


@pytest.mark.parametrize("env", [{"QC_POST_SPLIT": "1"}, {"QC_MLP_THREADS": "64"}, {"QC_MLP_THREADS": "1024"},
                                 {"QC_NO_MERGE": "1"}], ids=["post_split", "threads64", "threads1024", "no_merge"])
def test_env_variants_pass_the_same_checks(env):
    """QC_POST_SPLIT=1: the split point + weight-gradient post pair at H <= 128 as well; QC_MLP_THREADS=64 / 1024: the
    other block sizes of hidden_geometry; QC_NO_MERGE=1: the two-stream step.  One child at a time, each under its own
    time limit, runs the entry-point cases at H = 1, 129, 1024 and the fused step at H = 65, 257."""
    here = os.path.dirname(os.path.abspath(__file__))
    files = [os.path.join(here, "test_gpu_mlp_shapes.py"), os.path.join(here, "test_gpu_fused_widths.py")]
    r = subprocess.run([sys.executable, "-m", "pytest", *files, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", ENV_SELECTION], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "10 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
