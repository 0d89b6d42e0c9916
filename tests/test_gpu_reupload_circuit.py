"""The re-uploading circuit kernels (csrc/qc_circuit_reup*.h*, programs with EMBED gates) through engine.Circuit against
the float64 restatement of tests/reupload_reference.py: value forward + VJP, jets forward + VJP, with the tolerances of
tests/test_gpu_circuit.py (relative to the largest reference magnitude).  Negative control: the plain program's reference
must fail every quantity.  Two calls give the same bits.  A hand-built program with EMBED gates anywhere (not in whole
layers) goes through the same kernels.  n = 1 and n = 6 are refused, and so is amplitude encoding.
Double backward through DVQuantumLayer(reupload) against the restatement's double backward, with the bounds
tests/test_gpu_autograd.py uses beyond the interpolant."""
import ctypes as C

import numpy as np
import pytest
import torch

import reupload_reference as RR
from conftest import pkg
from test_gpu_fullsize import base_args

pytestmark = pytest.mark.gpu

TOL_Z = 1e-5


def _circuit(ans, n, L, seed, device, reupload=True):
    circuits, engine = pkg("circuits"), pkg("hip.engine")
    use_haar = seed is not None and n >= 4
    prog = circuits.build_program(ans, n, L, use_haar, reupload=reupload)
    assert any(g.op == circuits.OP_EMBED for g in prog.gates) == reupload
    return engine.Circuit(prog, circuits.haar_unitaries(seed, seed + 1) if use_haar else None, device)


VJP_CASES = [("cascade", 4, 2, 1, 200), ("layered", 4, 3, 1, 70), ("cross_mesh", 3, 2, None, 65), ("cascade", 2, 2, None, 10),
             ("alternate", 5, 2, 1, 64), ("farhi", 5, 3, 1, 1)]


def _vjp_errors(got, o, B):
    """quantity -> error / tolerance (tests/test_gpu_circuit.py's bounds)."""
    q, dx, dp = got
    return {"q": np.abs(q - o["q"]).max() / TOL_Z,
            "dx": np.abs(dx - o["dx"]).max() / 2e-5,
            "dp": np.abs(dp - o["dp"].reshape(-1)).max() / (1e-5 * max(1.0, np.abs(o["dp"]).max()) * np.sqrt(B))}


@pytest.mark.parametrize("ans,n,L,seed,B", VJP_CASES)
def test_expval_vjp_matches_restatement(ans, n, L, seed, B, gpu_device):
    params, x, cot = RR.vjp_inputs(ans, n, L, B)
    circ = _circuit(ans, n, L, seed, gpu_device)
    o = RR.vjp_reference(ans, n, L, seed, B, params, x, cot)
    circ.prepare(params.to(gpu_device))
    ang = x.t().contiguous().to(gpu_device)
    qh = circ.forward_expval(ang)
    d_ang, d_theta = circ.backward_expval(ang, cot.to(gpu_device))
    got = (qh.cpu().double().numpy(), d_ang.t().cpu().double().numpy(), d_theta.cpu().double().numpy())
    err = _vjp_errors(got, o, B)
    print(ans, n, L, B, "error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    # determinism: the same call twice, the same bits
    q2 = circ.forward_expval(ang)
    d2, t2 = circ.backward_expval(ang, cot.to(gpu_device))
    assert torch.equal(qh, q2) and torch.equal(d_ang, d2) and torch.equal(d_theta, t2)
    # negative control: the circuit without re-uploading misses every quantity
    bad = _vjp_errors(got, RR.vjp_reference(ans, n, L, seed, B, params, x, cot, reupload=False), B)
    assert min(bad.values()) > 1.0, bad


JETS_CASES = [("cascade", 4, 2, 1, 70), ("layered", 5, 3, 1, 9), ("cross_mesh", 3, 2, None, 8), ("cascade", 2, 2, None, 5),
              ("alternate", 5, 2, 1, 65), ("farhi", 4, 3, 1, 6)]


def _jets_errors(got, o):
    q, da, dp = got
    err = np.abs(q - o["q"])
    return {"q0": err[0].max() / TOL_Z,
            "q": err.max() / (1e-5 * max(1.0, np.abs(o["q"]).max())),
            "da": np.abs(da - o["da"]).max() / (2e-5 * max(1.0, np.abs(o["da"]).max())),
            "dp": np.abs(dp - o["dp"].reshape(-1)).max() / (2e-5 * max(1.0, np.abs(o["dp"]).max()))}


@pytest.mark.parametrize("ans,n,L,seed,B", JETS_CASES)
def test_jets_forward_and_vjp_match_restatement(ans, n, L, seed, B, gpu_device):
    params, ajets, w = RR.jets_inputs(ans, n, L, B)
    circ = _circuit(ans, n, L, seed, gpu_device)
    o = RR.jets_reference(ans, n, L, seed, B, params, ajets, w)
    circ.prepare(params.to(gpu_device))
    aj = ajets.to(gpu_device)
    qh = circ.forward_jets(aj)
    abar, d_theta = circ.backward_jets(aj, w.to(gpu_device))
    got = (qh.cpu().double().numpy(), abar.cpu().double().numpy(), d_theta.cpu().double().numpy())
    err = _jets_errors(got, o)
    print(ans, n, L, B, "error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    q2 = circ.forward_jets(aj)
    a2, t2 = circ.backward_jets(aj, w.to(gpu_device))
    assert torch.equal(qh, q2) and torch.equal(abar, a2) and torch.equal(d_theta, t2)
    bad = _jets_errors(got, RR.jets_reference(ans, n, L, seed, B, params, ajets, w, reupload=False))
    assert min(bad.values()) > 1.0, bad


def _scattered(sim, p, x):
    """EMBED gates anywhere: first in the program, alone, twice in a row on one wire (the run splits), last before H."""
    sim.RX(x[:, 2], 2)
    sim.RY(p[0], 0)
    sim.RX(x[:, 1], 1)
    sim.CNOT(0, 1)
    sim.RX(x[:, 1], 1)
    sim.RX(x[:, 1], 1)
    sim.RX(x[:, 0], 0)
    sim.CRX(p[1], 2, 0)
    sim.RZ(p[2], 2)
    sim.RX(x[:, 2], 2)
    sim.RX(p[3], 1)
    sim.RX(x[:, 0], 0)
    sim.RX(x[:, 2], 2)


_scattered.takes_angles = True


def _scattered_program():
    c = pkg("circuits")
    E = lambda w: c.Gate(c.OP_EMBED, w, -1, -1)
    gates = [E(2), c.Gate(c.OP_RY, 0, -1, 0), E(1), c.Gate(c.OP_CNOT, 0, 1, -1), E(1), E(1), E(0), c.Gate(c.OP_CRX, 2, 0, 1),
             c.Gate(c.OP_RZ, 2, -1, 2), E(2), c.Gate(c.OP_RX, 1, -1, 3), E(0), E(2), c.Gate(c.OP_H, 2, -1, -1)]
    return c.GateProgram(3, 1, "scattered", 4, False, gates)


def test_embed_gates_anywhere(gpu_device):
    """Not only whole layers: every run of EMBED gates on distinct wires is one exchange, whatever its wires."""
    n, B = 3, 70
    g = torch.Generator().manual_seed(11)
    params = torch.randn(1, 4, generator=g) * 0.8
    ajets = torch.randn(6, n, B, generator=g) * 0.9
    w = torch.randn(6, n, B, generator=g)
    circ = pkg("hip.engine").Circuit(_scattered_program(), None, gpu_device)
    circ.prepare(params.to(gpu_device))
    # value kernels
    xo, po = ajets[0].t().double().requires_grad_(True), params.double().requires_grad_(True)
    q = RR.expvals(xo, po, _scattered, n)
    (q * w[0].double()).sum().backward()
    o = {"q": q.detach().numpy(), "dx": xo.grad.numpy(), "dp": po.grad.numpy()}
    ang = ajets[0].contiguous().to(gpu_device)
    qh = circ.forward_expval(ang)
    d_ang, d_theta = circ.backward_expval(ang, w[0].contiguous().to(gpu_device))
    err = _vjp_errors((qh.cpu().double().numpy(), d_ang.t().cpu().double().numpy(), d_theta.cpu().double().numpy()), o, B)
    print("scattered, value, error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    # jet kernels
    ao, po = ajets.double().requires_grad_(True), params.double().requires_grad_(True)
    qo = RR.qjets(ao, po, _scattered, n)
    (qo * w.double()).sum().backward()
    o = {"q": qo.detach().numpy(), "da": ao.grad.numpy(), "dp": po.grad.numpy()}
    aj = ajets.to(gpu_device)
    qj = circ.forward_jets(aj)
    abar, d_theta = circ.backward_jets(aj, w.to(gpu_device))
    err = _jets_errors((qj.cpu().double().numpy(), abar.cpu().double().numpy(), d_theta.cpu().double().numpy()), o)
    print("scattered, jets, error / tolerance:", err)
    assert max(err.values()) < 1.0, err


def _raw_forward(ans, n, L, device):
    """(rc of qc_program_create, rc of qc_forward_expval, rc of qc_program_set_encoding(1)) of a re-upload program."""
    circuits, Lb = pkg("circuits"), pkg("hip.lib")
    lib = Lb.load()
    prog = circuits.build_program(ans, n, L, False, reupload=True)
    rows = np.ascontiguousarray(prog.rows())
    assert (rows[:, 0] == circuits.OP_EMBED).sum() == (L - 1) * n
    h = C.c_void_p()
    with torch.cuda.device(device):
        rc0 = lib.qc_program_create(rows.ctypes.data_as(C.c_void_p), prog.n_gates, n, prog.n_params, C.byref(h))
        if rc0 != 0:
            return rc0, None, None
        trig = torch.zeros(max(int(lib.qc_trig_bytes(h)) // 4, 4), dtype=torch.float32, device=device)
        theta = torch.zeros(max(prog.n_params, 1), dtype=torch.float32, device=device)
        st = torch.cuda.current_stream(device).cuda_stream
        assert lib.qc_prepare_gates(h, theta.data_ptr(), trig.data_ptr(), st) == 0
        a = torch.zeros(n, 8, dtype=torch.float32, device=device)
        out = torch.full_like(a, 7.0)
        rc1 = lib.qc_forward_expval(h, trig.data_ptr(), None, a.data_ptr(), out.data_ptr(), 8, None, 0, st)
        torch.cuda.synchronize()
        if rc1 != 0:
            assert bool((out == 7.0).all())          # nothing ran
        rc2 = lib.qc_program_set_encoding(h, 1)
        lib.qc_program_destroy(h)
    return rc0, rc1, rc2


def test_refusals(gpu_device):
    Lb = pkg("hip.lib")
    UNSUPPORTED = -2
    assert Lb.load().qc_error_string(UNSUPPORTED).decode().startswith("unsupported")
    assert _raw_forward("cascade", 6, 2, gpu_device)[:2] == (0, UNSUPPORTED)
    assert _raw_forward("farhi", 1, 2, gpu_device)[:2] == (0, UNSUPPORTED)
    rc0, rc1, rc2 = _raw_forward("cascade", 3, 2, gpu_device)
    assert (rc0, rc1, rc2) == (0, 0, UNSUPPORTED)
    # a malformed EMBED row (a second wire, a slot) is an argument error
    lib = Lb.load()
    for bad in ((8, 0, 1, -1), (8, 0, -1, 0), (8, 3, -1, -1), (9, 0, -1, -1)):
        rows = np.array([bad, (3, 2, -1, -1)], dtype=np.int32)
        h = C.c_void_p()
        with torch.cuda.device(gpu_device):
            assert lib.qc_program_create(rows.ctypes.data_as(C.c_void_p), 2, 3, 1, C.byref(h)) == -1


def test_double_backward_through_the_layer(gpu_device):
    """create_graph=True on a re-uploaded layer takes the jet kernels (the interpolant would be wrong)."""
    n, L, B, ans = 3, 2, 5, "cascade"
    args = base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, reupload=True)
    torch.manual_seed(3)
    layer = pkg("nn.DVQuantumLayer").DVQuantumLayer(args).to(gpu_device)
    g0 = torch.Generator().manual_seed(5)
    x0 = torch.rand(B, n, dtype=torch.float64, generator=g0) * 2.0 - 0.7
    w = torch.rand(n, B, dtype=torch.float64, generator=g0)

    def run(fwd, params, x, wt):
        x = x.clone().requires_grad_(True)
        q = fwd(x)
        g, = torch.autograd.grad((q * wt.to(q.dtype)).sum(), x, create_graph=True)
        s = (g * g).sum()
        h, = torch.autograd.grad(s, x, retain_graph=True)
        p, = torch.autograd.grad(s, params)
        return q.detach(), g.detach(), h.detach(), p.detach()

    po = layer.params.detach().cpu().double().requires_grad_(True)
    outs = {}
    for re in (True, False):
        outs[re] = run(lambda x: RR.expvals(x, po, ans, n, None, re), po, x0, w)
    qo, go, ho, pg = outs[True]
    qh, gh, hh, ph = run(layer, layer.params, x0.to(gpu_device, torch.float32), w.to(gpu_device, torch.float32))

    def errs(ref):
        q_, g_, h_, p_ = ref
        return {"q": (qh.cpu().double() - q_).abs().max().item() / 1e-5,
                "g": (gh.cpu().double() - g_).abs().max().item() / (2e-5 * max(1.0, g_.abs().max().item())),
                "h": (hh.cpu().double() - h_).abs().max().item() / (1e-4 * max(1.0, h_.abs().max().item())),
                "p": (ph.cpu().double() - p_).abs().max().item() / (2e-4 * max(1.0, p_.abs().max().item()))}
    err = errs(outs[True])
    print("double backward, error / tolerance:", err)
    assert max(err.values()) < 1.0, err
    assert min(errs(outs[False]).values()) > 1.0
    with pytest.raises(ValueError):
        layer.trig_interpolant(x0.to(gpu_device, torch.float32))
