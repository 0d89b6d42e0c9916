"""The SCALED re-uploading circuit kernels (programs with EMBEDS gates, RX(theta[slot] a_w)) through engine.Circuit against
the float64 restatement of tests/reupload_scale_reference.py: value forward + VJP, jets forward + VJP, with the tolerances
of tests/test_gpu_reupload_circuit.py, unchanged; d_theta includes the scalings' slots.  Scalings are 1 + 0.4 randn from
their own seed.  Negative control in every case: the reference with every scaling set to 1 must fail every quantity.  Two
calls give the same bits.  Special values (a scaling 0, a negative one, all 1 against the reupload=True kernels), a
hand-built program (EMBED and EMBEDS mixed in a run, twice in a row on a wire, first, last, a shared slot), the refusals,
and double backward through DVQuantumLayer(reupload_scale)."""
import ctypes as C

import numpy as np
import pytest
import torch

import reupload_reference as RR
import reupload_scale_reference as RS
from conftest import pkg
from test_gpu_fullsize import base_args
from test_gpu_reupload_circuit import _jets_errors, _vjp_errors

pytestmark = pytest.mark.gpu

UNSUPPORTED, ERR_ARG = -2, -1


def _circuit(ans, n, L, seed, device, mode):
    circuits, engine = pkg("circuits"), pkg("hip.engine")
    use_haar = seed is not None and n >= 4
    prog = circuits.build_program(ans, n, L, use_haar, reupload=True, reupload_scale=mode)
    assert sum(g.op == circuits.OP_EMBED_S for g in prog.gates) == (L - 1) * n
    return engine.Circuit(prog, circuits.haar_unitaries(seed, seed + 1) if use_haar else None, device)


def _run_value(circ, theta, x, cot, dev):
    circ.prepare(theta.to(dev))
    ang = x.t().contiguous().to(dev)
    q = circ.forward_expval(ang)
    d_ang, d_theta = circ.backward_expval(ang, cot.to(dev))
    return q, d_ang, d_theta


def _run_jets(circ, theta, ajets, w, dev):
    circ.prepare(theta.to(dev))
    aj = ajets.to(dev)
    q = circ.forward_jets(aj)
    abar, d_theta = circ.backward_jets(aj, w.to(dev))
    return q, abar, d_theta


def _np_value(out):
    q, d_ang, d_theta = out
    return q.cpu().double().numpy(), d_ang.t().cpu().double().numpy(), d_theta.cpu().double().numpy()


def _np_jets(out):
    return tuple(t.cpu().double().numpy() for t in out)


def _scale_grad_is_large(o, ns, tol):
    """the check is not vacuous: the reference's scale gradients are far above the tolerance"""
    return np.abs(o["dp"][-ns:]).max() > 50 * tol


VJP_CASES = [("cascade", 4, 2, 1, 258, "wire"), ("layered", 3, 3, 1, 65, "wire"), ("cascade", 2, 2, None, 5, "wire"),
             ("alternate", 5, 2, 1, 64, "wire"), ("farhi", 5, 3, 1, 1, "wire"), ("cascade", 3, 3, None, 70, "layer")]


@pytest.mark.parametrize("ans,n,L,seed,B,mode", VJP_CASES)
def test_expval_vjp_matches_restatement(ans, n, L, seed, B, mode, gpu_device):
    theta, x, cot = RS.vjp_inputs(ans, n, L, B, mode)
    ns = RS.n_scales(n, L, mode)
    circ = _circuit(ans, n, L, seed, gpu_device, mode)
    assert circ.n_params == theta.numel() and circ.n_scale == ns
    o = RS.vjp_reference(ans, n, L, seed, B, mode, theta, x, cot)
    out = _run_value(circ, theta, x, cot, gpu_device)
    got = _np_value(out)
    err = _vjp_errors(got, o, B)
    err["ds"] = np.abs(got[2][-ns:] - o["dp"][-ns:]).max() / (1e-5 * max(1.0, np.abs(o["dp"]).max()) * np.sqrt(B))
    print(ans, n, L, B, mode, "error / tolerance:", err, "|ds| of the reference", np.abs(o["dp"][-ns:]))
    assert max(err.values()) < 1.0, err
    assert _scale_grad_is_large(o, ns, 1e-5 * np.sqrt(B))
    # determinism: the same call twice, the same bits
    again = _run_value(circ, theta, x, cot, gpu_device)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    # negative control: every scaling 1 misses every quantity
    bad = _vjp_errors(got, RS.vjp_reference(ans, n, L, seed, B, mode, theta, x, cot, control=True), B)
    print("control:", bad)
    assert min(bad.values()) > 1.0, bad


JETS_CASES = [("cascade", 4, 2, 1, 70, "wire"), ("layered", 5, 3, 1, 9, "wire"), ("cross_mesh", 3, 2, None, 8, "wire"),
              ("cascade", 2, 2, None, 5, "wire"), ("alternate", 5, 2, 1, 65, "wire"), ("farhi", 4, 3, 1, 6, "wire"),
              ("cascade", 3, 3, None, 65, "layer")]


@pytest.mark.parametrize("ans,n,L,seed,B,mode", JETS_CASES)
def test_jets_forward_and_vjp_match_restatement(ans, n, L, seed, B, mode, gpu_device):
    theta, ajets, w = RS.jets_inputs(ans, n, L, B, mode)
    ns = RS.n_scales(n, L, mode)
    circ = _circuit(ans, n, L, seed, gpu_device, mode)
    o = RS.jets_reference(ans, n, L, seed, B, mode, theta, ajets, w)
    out = _run_jets(circ, theta, ajets, w, gpu_device)
    got = _np_jets(out)
    err = _jets_errors(got, o)
    err["ds"] = np.abs(got[2][-ns:] - o["dp"][-ns:]).max() / (2e-5 * max(1.0, np.abs(o["dp"]).max()))
    print(ans, n, L, B, mode, "error / tolerance:", err, "|ds| of the reference", np.abs(o["dp"][-ns:]))
    assert max(err.values()) < 1.0, err
    assert _scale_grad_is_large(o, ns, 2e-5)
    again = _run_jets(circ, theta, ajets, w, gpu_device)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    bad = _jets_errors(got, RS.jets_reference(ans, n, L, seed, B, mode, theta, ajets, w, control=True))
    print("control:", bad)
    assert min(bad.values()) > 1.0, bad


# ---------------------------------------------------------------- special values
def _special(scales, gpu_device):
    """(value errors, jets errors, value reference, jets reference) of cascade, n = 3, L = 2, B = 70 with these scalings."""
    ans, n, L, B = "cascade", 3, 2, 70
    theta, ajets, w = RS.jets_inputs(ans, n, L, B)
    theta = theta.clone()
    theta[-n:] = torch.tensor(scales)
    circ = _circuit(ans, n, L, None, gpu_device, "wire")
    build = RS.whole_circuit(ans, n, L, "wire")
    x, cot = ajets[0].t().contiguous(), w[0].contiguous()
    ov = RS.vjp_compute(build, n, None, theta, x, cot)
    oj = RS.jets_compute(build, n, None, theta, ajets, w)
    ev = _vjp_errors(_np_value(_run_value(circ, theta, x, cot, gpu_device)), ov, B)
    ej = _jets_errors(_np_jets(_run_jets(circ, theta, ajets, w, gpu_device)), oj)
    return ev, ej, ov, oj


def test_a_scaling_of_zero_is_the_identity_with_a_gradient(gpu_device):
    ev, ej, ov, oj = _special([0.0, 0.7, 1.3], gpu_device)
    print("s = 0 on wire 0, error / tolerance:", ev, ej, "reference ds", ov["dp"][-3:], oj["dp"][-3:])
    assert max(ev.values()) < 1.0 and max(ej.values()) < 1.0, (ev, ej)
    assert abs(ov["dp"][-3]) > 1e-2 and abs(oj["dp"][-3]) > 1e-2        # the gate is the identity, its gradient is not 0


def test_a_negative_scaling(gpu_device):
    ev, ej, ov, oj = _special([-0.8, 1.2, 0.6], gpu_device)
    print("s = -0.8 on wire 0, error / tolerance:", ev, ej)
    assert max(ev.values()) < 1.0 and max(ej.values()) < 1.0, (ev, ej)


def test_all_scalings_one_is_the_reuploaded_model(gpu_device):
    ans, n, L, B = "cascade", 3, 2, 70
    circuits, engine = pkg("circuits"), pkg("hip.engine")
    theta, ajets, w = RS.jets_inputs(ans, n, L, B)
    theta = RS.ones_control(theta, n)
    P = theta.numel() - n
    x, cot = ajets[0].t().contiguous(), w[0].contiguous()
    scaled = _circuit(ans, n, L, None, gpu_device, "wire")
    plain = engine.Circuit(circuits.build_program(ans, n, L, False, reupload=True), None, gpu_device)
    qs, dxs, dts = _np_value(_run_value(scaled, theta, x, cot, gpu_device))
    qp, dxp, dtp = _np_value(_run_value(plain, theta[:P], x, cot, gpu_device))
    err = _vjp_errors((qs, dxs, dts[:P]), {"q": qp, "dx": dxp, "dp": dtp}, B)
    print("value kernels, scaled at ones against reupload=True, error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    js, jp = _np_jets(_run_jets(scaled, theta, ajets, w, gpu_device)), _np_jets(_run_jets(plain, theta[:P], ajets, w, gpu_device))
    err = _jets_errors((js[0], js[1], js[2][:P]), {"q": jp[0], "da": jp[1], "dp": jp[2]})
    print("jet kernels, error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    # and against the float64 reference of the reupload=True circuit
    params = theta[:P].reshape(L, -1)
    ao, po = ajets.double().requires_grad_(True), params.double().requires_grad_(True)
    qo = RR.qjets(ao, po, ans, n, None, True)
    (qo * w.double()).sum().backward()
    err = _jets_errors((js[0], js[1], js[2][:P]), {"q": qo.detach().numpy(), "da": ao.grad.numpy(), "dp": po.grad.numpy()})
    assert max(err.values()) < 1.0, err


# ---------------------------------------------------------------- a hand-built program
def _placed(sim, t, x):
    """theta = (p0..p3, s4..s7).  EMBEDS first in the program; a run that mixes EMBED and EMBEDS on different wires; EMBEDS
    twice in a row on one wire (two runs); two EMBEDS gates on different wires sharing slot 7; EMBEDS last before H."""
    S = lambda w, slot: sim.RX(t[slot] * x[:, w], w)
    E = lambda w: sim.RX(x[:, w], w)
    S(2, 4)
    sim.RY(t[0], 0)
    E(0)
    S(1, 5)
    sim.CNOT(0, 1)
    S(1, 5)
    S(1, 6)
    sim.CRX(t[1], 2, 0)
    sim.RZ(t[2], 2)
    S(0, 7)
    S(2, 7)
    sim.RX(t[3], 1)
    S(0, 6)


_placed.takes_angles = True


def _placed_program():
    c = pkg("circuits")
    S = lambda w, slot: c.Gate(c.OP_EMBED_S, w, -1, slot)
    E = lambda w: c.Gate(c.OP_EMBED, w, -1, -1)
    gates = [S(2, 4), c.Gate(c.OP_RY, 0, -1, 0), E(0), S(1, 5), c.Gate(c.OP_CNOT, 0, 1, -1), S(1, 5), S(1, 6),
             c.Gate(c.OP_CRX, 2, 0, 1), c.Gate(c.OP_RZ, 2, -1, 2), S(0, 7), S(2, 7), c.Gate(c.OP_RX, 1, -1, 3), S(0, 6),
             c.Gate(c.OP_H, 2, -1, -1)]
    return c.GateProgram(3, 1, "placed", 8, False, gates)


def test_scaled_gates_anywhere(gpu_device):
    n, B = 3, 70
    g = torch.Generator().manual_seed(12)
    theta = torch.cat([torch.randn(4, generator=g) * 0.8, RS.scalings(4, 31).float()])
    ajets = torch.randn(6, n, B, generator=g) * 0.9
    w = torch.randn(6, n, B, generator=g)
    circ = pkg("hip.engine").Circuit(_placed_program(), None, gpu_device)
    assert circ.n_scale == 4
    x, cot = ajets[0].t().contiguous(), w[0].contiguous()
    ov = RS.vjp_compute(_placed, n, None, theta, x, cot)
    ev = _vjp_errors(_np_value(_run_value(circ, theta, x, cot, gpu_device)), ov, B)
    print("placed, value, error / tolerance:", ev)
    assert max(ev.values()) < 1.0, ev
    oj = RS.jets_compute(_placed, n, None, theta, ajets, w)
    ej = _jets_errors(_np_jets(_run_jets(circ, theta, ajets, w, gpu_device)), oj)
    print("placed, jets, error / tolerance:", ej)
    assert max(ej.values()) < 1.0, ej
    # the control: all four scalings 1
    ones = RS.ones_control(theta, 4)
    bad = _vjp_errors(_np_value(_run_value(circ, theta, x, cot, gpu_device)), RS.vjp_compute(_placed, n, None, ones, x, cot), B)
    assert min(bad.values()) > 1.0, bad


# ---------------------------------------------------------------- refusals
def _raw_forward(ans, n, L, device):
    """(rc of qc_program_create, rc of qc_forward_expval, rc of qc_program_set_encoding(1)) of a scaled program."""
    circuits, Lb = pkg("circuits"), pkg("hip.lib")
    lib = Lb.load()
    prog = circuits.build_program(ans, n, L, False, reupload=True, reupload_scale="wire")
    rows = np.ascontiguousarray(prog.rows())
    assert (rows[:, 0] == circuits.OP_EMBED_S).sum() == (L - 1) * n
    h = C.c_void_p()
    with torch.cuda.device(device):
        rc0 = lib.qc_program_create(rows.ctypes.data_as(C.c_void_p), prog.n_gates, n, prog.n_params, C.byref(h))
        if rc0 != 0:
            return rc0, None, None
        trig = torch.zeros(max(int(lib.qc_trig_bytes(h)) // 4, 4), dtype=torch.float32, device=device)
        theta = torch.ones(max(prog.n_params, 1), dtype=torch.float32, device=device)
        st = torch.cuda.current_stream(device).cuda_stream
        assert lib.qc_prepare_gates(h, theta.data_ptr(), trig.data_ptr(), st) == 0
        a = torch.zeros(n, 8, dtype=torch.float32, device=device)
        out = torch.full_like(a, 7.0)
        rc1 = lib.qc_forward_expval(h, trig.data_ptr(), None, a.data_ptr(), out.data_ptr(), 8, None, 0, st)
        torch.cuda.synchronize()
        if rc1 != 0:
            assert bool((out == 7.0).all())          # nothing was written
        rc2 = lib.qc_program_set_encoding(h, 1)
        lib.qc_program_destroy(h)
    return rc0, rc1, rc2


def test_refusals(gpu_device):
    assert _raw_forward("cascade", 6, 2, gpu_device)[:2] == (0, UNSUPPORTED)
    assert _raw_forward("farhi", 1, 2, gpu_device)[:2] == (0, UNSUPPORTED)
    assert _raw_forward("cascade", 3, 2, gpu_device) == (0, 0, UNSUPPORTED)
    lib = pkg("hip.lib").load()
    # a slot is required, no second wire, the wire in range, the slot below n_params (2 here)
    for bad in ((9, 0, -1, -1), (9, 0, 1, 0), (9, 3, -1, 0), (9, 0, -1, 2), (9, -1, -1, 0)):
        rows = np.array([bad, (3, 2, -1, -1)], dtype=np.int32)
        h = C.c_void_p()
        with torch.cuda.device(gpu_device):
            assert lib.qc_program_create(rows.ctypes.data_as(C.c_void_p), 2, 3, 2, C.byref(h)) == ERR_ARG, bad
    rows = np.array([(9, 0, -1, 1), (3, 2, -1, -1)], dtype=np.int32)
    h = C.c_void_p()
    with torch.cuda.device(gpu_device):
        assert lib.qc_program_create(rows.ctypes.data_as(C.c_void_p), 2, 3, 2, C.byref(h)) == 0
        lib.qc_program_destroy(h)


# ---------------------------------------------------------------- double backward
def test_double_backward_through_the_layer(gpu_device):
    """create_graph=True goes through _LayerVjpFn with the concatenated theta; the gradient of embed_scale is part of p."""
    n, L, B, ans = 3, 2, 5, "cascade"
    args = base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, reupload=True, reupload_scale="wire")
    torch.manual_seed(3)
    layer = pkg("nn.DVQuantumLayer").DVQuantumLayer(args).to(gpu_device)
    with torch.no_grad():
        layer.embed_scale.copy_(RS.scalings(n, 41).float().reshape(1, n))
    g0 = torch.Generator().manual_seed(5)
    x0 = torch.rand(B, n, dtype=torch.float64, generator=g0) * 2.0 - 0.7
    w = torch.rand(n, B, dtype=torch.float64, generator=g0)

    def run(fwd, params, x, wt):
        x = x.clone().requires_grad_(True)
        q = fwd(x)
        g, = torch.autograd.grad((q * wt.to(q.dtype)).sum(), x, create_graph=True)
        s = (g * g).sum()
        h, = torch.autograd.grad(s, x, retain_graph=True)
        p = torch.autograd.grad(s, params)
        return q.detach(), g.detach(), h.detach(), torch.cat([t.detach().reshape(-1) for t in p])

    build = RS.whole_circuit(ans, n, L, "wire")
    outs = {}
    for ones in (False, True):
        to = layer.theta().detach().cpu().double()
        if ones:
            to = RS.ones_control(to, n)
        to.requires_grad_(True)
        outs[ones] = run(lambda x: RS.expvals(x, to, build, n), [to], x0, w)
    qh, gh, hh, ph = run(layer, [layer.params, layer.embed_scale], x0.to(gpu_device, torch.float32), w.to(gpu_device, torch.float32))
    assert ph.numel() == layer.program.n_params

    def errs(ref):
        q_, g_, h_, p_ = ref
        return {"q": (qh.cpu().double() - q_).abs().max().item() / 1e-5,
                "g": (gh.cpu().double() - g_).abs().max().item() / (2e-5 * max(1.0, g_.abs().max().item())),
                "h": (hh.cpu().double() - h_).abs().max().item() / (1e-4 * max(1.0, h_.abs().max().item())),
                "p": (ph.cpu().double() - p_).abs().max().item() / (2e-4 * max(1.0, p_.abs().max().item()))}
    err = errs(outs[False])
    print("double backward, error / tolerance:", err, "reference d/d(embed_scale)", outs[False][3][-n:])
    assert max(err.values()) < 1.0, err
    assert outs[False][3][-n:].abs().max().item() > 1e-2
    assert errs(outs[True])["q"] > 1.0
