"""The seven-channel stages on the GPU, through the C ABI: qc_pre_forward_tt / qc_pre_backward_tt, qc_forward_jets_tt /
qc_backward_jets_tt, qc_post_coef_tt and qc_post_jets_tt against the float64 reference of tests/tt_reference.py (the
six-channel reference evaluated twice, the second time with t and x exchanged), and the refusals.

Bounds are the project's: POINT_TOL / ROW_TOL of tests/test_gpu_tabulated.py for the network stages, the circuit bounds of
tests/test_gpu_reupload_circuit.py::_jets_errors.  The tt channel is the xx channel of the column-swapped model, so its
rounding is that channel's."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_reference as R
import tt_reference as TR
from conftest import pkg
from step_reference import haar_for
from test_gpu_reupload_circuit import _jets_errors
from test_gpu_tabulated import POINT_TOL, ROW_TOL

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROW0, STRIDE_PAD, N_THETA = 2, 7, 3
rel = lambda got, want, tol: float(np.abs(got - want).max() / (tol * max(1.0, np.abs(want).max())))


def _nan(dev, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _weights(H, n, names, seed):
    """A flat vector that is NaN outside the blocks ``names`` (a stage must not read another stage's weights)."""
    g = np.random.default_rng(seed)
    lay, NP = R.layout(H, n, N_THETA)
    flat = np.full(NP, np.nan, np.float32)
    scale = {"W1": np.sqrt(2.0 / (H + 3)), "b1": 0.1, "W2": np.sqrt(2.0 / (H + n)), "b2": 0.1, "W3": 1.0 / np.sqrt(n), "b3": 0.3,
             "W4": 1.0 / np.sqrt(H), "b4": 0.1}
    for k in names:
        o, s = lay[k]
        flat[o:o + int(np.prod(s))] = g.standard_normal(int(np.prod(s))) * scale[k]
    return flat, lay, NP


def _rows_check(part, lay, NP, names, tiles, extra=()):
    """The partial rows: finite in rows ROW0 .. ROW0 + tiles - 1 at the columns of ``names`` (and ``extra``), NaN elsewhere."""
    cols = np.concatenate([np.arange(lay[k][0], lay[k][0] + int(np.prod(lay[k][1]))) for k in names] + [np.asarray(extra, int)])
    p = part.cpu().numpy()
    mask = np.zeros(p.shape, bool)
    mask[ROW0:ROW0 + tiles, cols] = True
    assert np.isnan(p[~mask]).all() and np.isfinite(p[mask]).all()
    return p[ROW0:ROW0 + tiles], cols


# ---- 1. the pre network
@pytest.mark.parametrize("H,n,B", [(1, 2, 1), (50, 4, 65), (67, 5, 130)])
def test_pre_stage_forward_and_reverse(H, n, B, gpu_device):
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    st = torch.cuda.current_stream(dev).cuda_stream
    names = ("W1", "b1", "W2", "b2")
    flat, lay, NP = _weights(H, n, names, 100 + H)
    g = np.random.default_rng(B)
    X = g.uniform(0, 1, (B, 3)).astype(np.float32)
    abar = g.standard_normal((7, n, B)).astype(np.float32)
    tiles = (B + 63) // 64
    prm, Xd, ab = (torch.from_numpy(a).to(dev) for a in (flat, X, abar))
    ajets, part = _nan(dev, 7 * n * B + 64), _nan(dev, ROW0 + tiles + 2, NP + 3 + STRIDE_PAD)
    L.check(lib.qc_pre_forward_tt(Xd.data_ptr(), prm.data_ptr(), H, n, N_THETA, ajets.data_ptr(), B, st), "qc_pre_forward_tt")
    L.check(lib.qc_pre_backward_tt(Xd.data_ptr(), prm.data_ptr(), H, n, N_THETA, ab.data_ptr(), part.data_ptr(), part.shape[1],
                                   ROW0, B, st), "qc_pre_backward_tt")
    # channel 4 of the existing six-channel stage on the model with t and x exchanged
    flat_s = flat.copy()
    o, s = lay["W1"]
    flat_s[o:o + 3 * H] = flat[o:o + 3 * H].reshape(H, 3)[:, TR.SWAP].reshape(-1)
    a6 = _nan(dev, 6, n, B)
    Xs, prm_s = torch.from_numpy(np.ascontiguousarray(X[:, TR.SWAP])).to(dev), torch.from_numpy(flat_s).to(dev)
    L.check(lib.qc_pre_forward(Xs.data_ptr(), prm_s.data_ptr(), H, n, N_THETA, a6.data_ptr(), B, 6, st), "qc_pre_forward")
    torch.cuda.synchronize(dev)
    a = ajets.cpu().numpy()
    assert np.isnan(a[7 * n * B:]).all() and np.isfinite(a[:7 * n * B]).all()
    a = a[:7 * n * B].reshape(7, n, B)
    rows, cols = _rows_check(part, lay, NP, names, tiles)

    P = R.unpack(np.nan_to_num(flat.astype(np.float64)), H, n, N_THETA)
    want = TR.pre_jets7(P, torch.from_numpy(X).double())
    obj = (want * torch.from_numpy(abar).double()).sum(dim=(0, 1))
    want_rows = np.stack([R.flatten(dict(zip(names, gr)), H, n, N_THETA) for gr in R.tile_grads(obj, [P[k] for k in names], B)])
    w = want.detach().numpy()
    err = {"ajets": rel(a, w, POINT_TOL), "tt": rel(a[6], w[6], POINT_TOL), "rows": rel(rows[:, cols], want_rows[:, cols], ROW_TOL),
           "tt_vs_swapped_xx": rel(a[6], a6.cpu().numpy()[4], POINT_TOL),
           "xx_of_swapped": rel(a6.cpu().numpy()[4], w[6], POINT_TOL)}         # the six-channel kernel's own error on that channel
    print(H, n, B, "error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    # negative control: a reference whose tt channel is the xx channel is told apart
    if B > 1:
        assert rel(a[6], w[4], POINT_TOL) > 1.0


# ---- 2. the circuit
JETS_CASES = [("cascade", 4, 1, 1, 70), ("layered", 5, 2, 1, 65), ("cross_mesh", 3, 2, None, 8), ("cascade", 2, 1, None, 1),
              ("farhi", 4, 2, 1, 64)]


def _circuit(ans, n, L, seed, device, **kw):
    circuits, engine = pkg("circuits"), pkg("hip.engine")
    use_haar = seed is not None and n >= 4
    prog = circuits.build_program(ans, n, L, use_haar, **{k: v for k, v in kw.items() if k == "reupload"})
    return engine.Circuit(prog, circuits.haar_unitaries(seed, seed + 1) if use_haar else None, device,
                          **{k: v for k, v in kw.items() if k != "reupload"})


def _jets_inputs(ans, n, L, B, salt=77):
    """tests/reupload_reference.py::jets_inputs with a seventh channel."""
    g = torch.Generator().manual_seed(salt + n + B)
    P = pkg("circuits").params_per_layer(ans, n)
    return torch.randn(L, P, generator=g) * 0.8, torch.randn(7, n, B, generator=g) * 0.9, torch.randn(7, n, B, generator=g)


def _jets_reference(ans, n, seed, params, ajets, w):
    ao, po = ajets.double().requires_grad_(True), params.double().requires_grad_(True)
    qo = TR.qjets7(ao, po, ans, n, haar_for(n, seed))
    (qo * w.double()).sum().backward()
    return {"q": qo.detach().numpy(), "da": ao.grad.numpy(), "dp": po.grad.numpy()}


@pytest.mark.parametrize("ans,n,L,seed,B", JETS_CASES)
def test_jets_forward_and_vjp(ans, n, L, seed, B, gpu_device):
    params, ajets, w = _jets_inputs(ans, n, L, B)
    circ = _circuit(ans, n, L, seed, gpu_device)
    circ.prepare(params.to(gpu_device))
    aj, wd = ajets.to(gpu_device), w.to(gpu_device)
    qh = circ.forward_jets_tt(aj)
    abar, d_theta = circ.backward_jets_tt(aj, wd)
    got = (qh.cpu().double().numpy(), abar.cpu().double().numpy(), d_theta.cpu().double().numpy())
    err = _jets_errors(got, _jets_reference(ans, n, seed, params, ajets, w))
    print(ans, n, L, B, "error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    q2 = circ.forward_jets_tt(aj)
    a2, t2 = circ.backward_jets_tt(aj, wd)
    assert torch.equal(qh, q2) and torch.equal(abar, a2) and torch.equal(d_theta, t2)
    # the six channels that do not involve tt are those of the six-channel kernels
    q6 = circ.forward_jets(aj[:6].contiguous())
    assert rel(qh[:6].cpu().numpy(), q6.cpu().numpy(), 1e-5) < 1.0
    # negative control: the reference with a_tt zeroed must fail
    zeroed = ajets.clone()
    zeroed[6] = 0.0
    bad = _jets_errors(got, _jets_reference(ans, n, seed, params, zeroed, w))
    assert max(bad.values()) > 1.0, bad


# ---- 3. the post network, coefficient form
@pytest.mark.parametrize("H,n,B", [(50, 4, 130), (3, 2, 1)])
def test_post_coef_tt_alone(H, n, B, gpu_device):
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    st = torch.cuda.current_stream(dev).cuda_stream
    names = ("W3", "b3", "W4", "b4")
    flat, lay, NP = _weights(H, n, names, 200 + H)
    g = np.random.default_rng(H + B)
    q = np.concatenate([g.uniform(-1, 1, (1, n, B)), g.standard_normal((6, n, B))]).astype(np.float32)
    target = g.standard_normal(B).astype(np.float32)
    coef = TR.coef_tt_star(g.uniform(0, 1, (B, 3)))
    tiles = (B + 63) // 64
    pde = dict(D=NAN, vx=NAN, vy=NAN, c_t=NAN, c_x=NAN, c_y=NAN, d_xx=NAN, d_yy=NAN, w_res=4.0 / B, inv_n_res=1.0 / B,
               w_val_a=NAN, w_val_b=NAN, inv_n_a=NAN, inv_n_b=NAN, problem=L.QC_PROBLEM_TABULATED, n_seg_a=0)
    qpde = L.QcPde(**pde)
    cot, qbar, uj = _nan(dev, 7 * B + 64), _nan(dev, 7 * n * B + 64), _nan(dev, 7 * B + 64)
    part = _nan(dev, ROW0 + tiles + 2, NP + 3 + STRIDE_PAD)
    prm, qd, tg = (torch.from_numpy(a).to(dev) for a in (flat, q, target))
    cf = torch.from_numpy(np.ascontiguousarray(coef.T)).to(dev)
    L.check(lib.qc_post_coef_tt(prm.data_ptr(), H, n, N_THETA, C.byref(qpde), qd.data_ptr(), tg.data_ptr(), cf.data_ptr(),
                                cot.data_ptr(), qbar.data_ptr(), part.data_ptr(), part.shape[1], ROW0, B, st), "qc_post_coef_tt")
    L.check(lib.qc_post_jets_tt(4, prm.data_ptr(), H, n, N_THETA, qd.data_ptr(), uj.data_ptr(), None, None, 0, 0, B, st),
            "qc_post_jets_tt")
    torch.cuda.synchronize(dev)
    rows, cols = _rows_check(part, lay, NP, names, tiles, extra=(NP, NP + 1, NP + 2))
    for buf, m in ((cot, 7 * B), (qbar, 7 * n * B), (uj, 7 * B)):
        a = buf.cpu().numpy()
        assert np.isnan(a[m:]).all() and np.isfinite(a[:m]).all()

    def errors(table, tgt):
        P = R.unpack(np.nan_to_num(flat.astype(np.float64)), H, n, N_THETA)
        qt = torch.from_numpy(q).double().requires_grad_(True)
        u = TR.post_jets7(P, qt)
        e = TR.residual_coef_tt(u, table) - torch.from_numpy(tgt).double()
        c = torch.from_numpy(np.asarray(table)).double()
        obj = 0.5 * pde["w_res"] * e * e
        gs = (pde["w_res"] * e).detach()
        want_cot = torch.stack([(c[:, 0] + 3.0 * c[:, 6] * u[0].detach() ** 2) * gs, gs * c[:, 1], gs * c[:, 2], gs * c[:, 3],
                                -c[:, 4] * gs, -c[:, 5] * gs, -c[:, 7] * gs]).numpy()
        qb = torch.autograd.grad(obj.sum(), qt, retain_graph=True)[0].numpy()
        want_rows = np.stack([R.flatten(dict(zip(names, gr)), H, n, N_THETA) for gr in R.tile_grads(obj, [P[k] for k in names], B)])
        losses = np.stack([[(e[k:k + 64] ** 2).sum().item() / B, 0.0, 0.0] for k in range(0, B, 64)])
        b4 = lay["b4"][0]
        return {"qbar": rel(qbar.cpu().numpy()[:7 * n * B].reshape(7, n, B), qb, POINT_TOL),
                "cot": rel(cot.cpu().numpy()[:7 * B].reshape(7, B), want_cot, POINT_TOL),
                "ujets": rel(uj.cpu().numpy()[:7 * B].reshape(7, B), u.detach().numpy(), POINT_TOL),
                "rows": rel(rows[:, cols[:-3]], want_rows[:, cols[:-3]], ROW_TOL),
                "b4": rel(rows[:, b4], np.array([want_cot[0, k:k + 64].sum() for k in range(0, B, 64)]), ROW_TOL),
                "loss": rel(rows[:, cols[-3:]], losses, ROW_TOL)}
    err = errors(coef, target)
    print(H, n, B, "error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    if B > 1:
        for v in TR.CONTROLS:
            assert max(errors(TR.variant_table(v, coef), target).values()) > 1.0, v
        assert max(errors(coef, np.roll(target, 1)).values()) > 1.0
    # qc_post_jets_tt mode 3 on the cotangents the coefficient form wrote: the same qbar and weight columns
    qbar3, part3 = _nan(dev, 7 * n * B + 64), _nan(dev, ROW0 + tiles + 2, NP + 3 + STRIDE_PAD)
    L.check(lib.qc_post_jets_tt(3, prm.data_ptr(), H, n, N_THETA, qd.data_ptr(), cot.data_ptr(), qbar3.data_ptr(), part3.data_ptr(),
                                part3.shape[1], ROW0, B, st), "qc_post_jets_tt")
    torch.cuda.synchronize(dev)
    rows3, cols3 = _rows_check(part3, lay, NP, names, tiles)
    assert torch.equal(qbar3[:7 * n * B], qbar[:7 * n * B]) and np.array_equal(rows3[:, cols3], rows[:, cols3])


# ---- 4. refusals
def test_programs_outside_the_register_family_and_other_encodings_are_refused(gpu_device):
    L = pkg("hip.lib")
    lib, dev = L.load(), gpu_device
    st = torch.cuda.current_stream(dev).cuda_stream
    B = 8
    freq = np.ones((3, 2), np.float32)
    circs = {"n6": _circuit("cascade", 6, 1, 1, dev), "reupload": _circuit("cascade", 3, 2, None, dev, reupload=True),
             "amplitude": _circuit("cascade", 4, 1, 1, dev, amplitude=True), "input_map": _circuit("cascade", 4, 1, 1, dev),
             "angle_map": _circuit("cascade", 4, 1, 1, dev, angle_map=L.QC_ANGLE_MAP_TANH_PI), "ok": _circuit("cascade", 4, 1, 1, dev)}
    circs["input_map"].set_input_map(freq)
    for name, c in circs.items():
        n = c.n
        c.prepare(torch.zeros(max(c.n_params, 1), device=dev))
        aj = torch.zeros(7, n, B, device=dev)
        out, abar, part = _nan(dev, 7, n, B), _nan(dev, 7, n, B), _nan(dev, 1, max(c.n_params, 1))
        rc_f = lib.qc_forward_jets_tt(c.handle, c.trig.data_ptr(), None if c.umat is None else c.umat.data_ptr(), aj.data_ptr(),
                                      out.data_ptr(), B, st)
        rc_b = lib.qc_backward_jets_tt(c.handle, c.trig.data_ptr(), None if c.umat is None else c.umat.data_ptr(), aj.data_ptr(),
                                       aj.data_ptr(), abar.data_ptr(), part.data_ptr(), part.shape[1], 0, B, st)
        torch.cuda.synchronize(dev)
        if name == "ok":
            assert rc_f == 0 and rc_b == 0 and torch.isfinite(out).all() and torch.isfinite(abar).all()
        else:
            assert rc_f == -2 and rc_b == -2, (name, rc_f, rc_b)
            assert torch.isnan(out).all() and torch.isnan(abar).all() and torch.isnan(part).all(), name
    # NULL buffers stay argument errors on a program that is served
    c = circs["ok"]
    assert lib.qc_forward_jets_tt(c.handle, c.trig.data_ptr(), c.umat.data_ptr(), None, None, B, st) == -1
