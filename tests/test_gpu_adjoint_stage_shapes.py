"""The merged step's adjoint stage (k_circ_bwd_both2: residual tiles as 3 waves x 2 channels, value tiles three waves
per block, the absorb flag a template parameter) against the stand-alone circuit calls on the same buffers.

qc_fused_step_stage runs stages 0..3 (pre forward, circuit forward, post, circuit adjoint) on a FusedStep; the adjoint
stage reads the angle jets and the cotangents of <Z> the earlier stages left in the step's workspace and writes ``abar``
of both pipelines and the theta columns of the partial rows.  The stand-alone calls

    qc_forward_jets_keep + qc_backward_jets_kept      (six-wave kernels, one channel per wave, a final-state store of their own)
    qc_forward_expval + qc_backward_expval            (four value waves per block)

then run on those same inputs into fresh outputs.  Compared: ``abar`` of the residual pipeline [6][n][B_res], ``abar`` of
the value pipeline [n][B_val], and the theta columns summed over the partial rows.

Programs: cascade at n = 2, 3, 4, 5 (the ansatz of the merged parity cases; its leading RX layer is folded into the
embedding: the ABSORB = true instantiation) and farhi at n = 4 (starts with a CNOT: ABSORB = false).  Shapes
(B_res, B_val): (1, 1); (64, 192) = one full residual tile and one full 192-point value block; (65, 193) = one point past
both; (129, 1) = three residual tiles, the last with one point.

Tolerance: the two forms add the same fp32 terms in different orders (three shares of lambda_0 against five, two
channels per wave against one), so they agree to rounding, not bitwise; this is the comparison of
tests/test_gpu_row_fold.py::two_stream_child (merged rows against the stand-alone launches' rows) and takes its
tolerance, 1e-6 x max(1, |reference|): per column for the summed theta columns, per array for ``abar``."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import pkg
from step_reference import step_inputs
from test_gpu_fullsize import Log, base_args

pytestmark = pytest.mark.gpu

H = 50
TOL = 1e-6
PROGRAMS = [("cascade", 2), ("cascade", 3), ("cascade", 4), ("cascade", 5), ("farhi", 4)]
SHAPES = [(1, 1), (64, 192), (65, 193), (129, 0 + 1)]


def _lead_rx(ansatz, n):
    """the first n gates are RX on wires 0..n-1 with distinct parameters (what the library folds into the embedding)"""
    c = pkg("circuits")
    gates = c.build_program(ansatz, n, 1, n >= 4).gates
    if len(gates) < n:
        return False
    head = gates[:n]
    return all(g.op == c.OP_RX and g.a == w for w, g in enumerate(head)) and len({g.slot for g in head}) == n


def test_programs_cover_both_absorb_forms():
    assert _lead_rx("cascade", 4) and not _lead_rx("farhi", 4)
    assert all(_lead_rx("cascade", n) for n in (2, 3, 5))


def _step(device, ansatz, n, B_res, B_val):
    engine = pkg("hip.engine")
    n_ic = (B_val + 1) // 2
    n_bc = B_val - n_ic
    n_theta = pkg("circuits").params_per_layer(ansatz, n)
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=4)
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=1, q_ansatz=ansatz), Log(), device=device)
    eng = model._engine_for(device)
    with torch.no_grad():
        eng.flat.copy_(torch.from_numpy(flat))
    eng.refresh_gates()
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, device))
    fs.X_res[:B_res] = X_res.to(device)
    fs.X_val[:n_ic] = X_ic.to(device)
    fs.X_val[n_ic:B_val] = X_bc.to(device)
    return model, eng, fs


@pytest.mark.parametrize("B_res,B_val", SHAPES, ids=[f"r{a}_v{b}" for a, b in SHAPES])
@pytest.mark.parametrize("ansatz,n", PROGRAMS, ids=[f"{a}{n}" for a, n in PROGRAMS])
def test_adjoint_stage_matches_standalone_calls(ansatz, n, B_res, B_val, gpu_device):
    L = pkg("hip.lib")
    model, eng, fs = _step(gpu_device, ansatz, n, B_res, B_val)
    lib, d = eng.lib, fs.desc
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    rows_res, rows_val = (B_res + 63) // 64, (B_val + 63) // 64
    n_theta, o_th = eng.n_theta, eng.theta_off
    f = dict(dtype=torch.float32, device=gpu_device)

    # the merged stages, on poisoned outputs
    fs.part.fill_(float("nan"))
    fs.ws_res[3].fill_(float("nan"))
    fs.ws_val[3].fill_(float("nan"))
    for stage in (L.QC_STAGE_PRE_FWD, L.QC_STAGE_CIRCUIT_FWD, L.QC_STAGE_POST, L.QC_STAGE_CIRCUIT_BWD):
        assert lib.qc_fused_step_stage(C.byref(d), stage, st) == 0, stage      # the merged form serves these sizes
    torch.cuda.synchronize()
    abar_res = fs.ws_res[3][:, :, :B_res].cpu().numpy().astype(np.float64)
    abar_val = fs.ws_val[3][0, :, :B_val].cpu().numpy().astype(np.float64)
    theta = fs.part[:, o_th:o_th + n_theta].cpu().numpy().astype(np.float64)
    assert theta.shape == (rows_res + rows_val, n_theta)
    for name, a in (("abar_res", abar_res), ("abar_val", abar_val), ("theta rows", theta)):
        assert np.isfinite(a).all(), (name, np.argwhere(~np.isfinite(a))[:4])

    # the stand-alone calls on the same inputs (angle jets, cotangents of <Z>), fresh outputs and a final-state store of
    # their own
    qj_res, ab_res = torch.full((6, n, B_res), float("nan"), **f), torch.full((6, n, B_res), float("nan"), **f)
    qj_val, ab_val = torch.full((n, B_val), float("nan"), **f), torch.full((n, B_val), float("nan"), **f)
    part2 = torch.full((rows_res + rows_val, fs.stride), float("nan"), **f)
    chi = torch.full((max(int(d.circ_ws_bytes), 4) // 4,), float("nan"), **f)
    th2 = part2.data_ptr() + 4 * o_th
    assert lib.qc_forward_jets_keep(d.prog, d.trig_dev, d.umat_dev, d.ajets_res_dev, qj_res.data_ptr(), B_res,
                                    chi.data_ptr(), st) == 0
    assert lib.qc_backward_jets_kept(d.prog, d.trig_dev, d.umat_dev, d.ajets_res_dev, d.qbar_res_dev, ab_res.data_ptr(), th2,
                                     fs.stride, 0, B_res, chi.data_ptr(), st) == 0
    assert lib.qc_forward_expval(d.prog, d.trig_dev, d.umat_dev, d.ajets_val_dev, qj_val.data_ptr(), B_val, None, 0, st) == 0
    assert lib.qc_backward_expval(d.prog, d.trig_dev, d.umat_dev, d.ajets_val_dev, d.qbar_val_dev, ab_val.data_ptr(), th2,
                                  fs.stride, rows_res, B_val, None, 0, st) == 0
    torch.cuda.synchronize()
    want_res = ab_res.cpu().numpy().astype(np.float64)
    want_val = ab_val.cpu().numpy().astype(np.float64)
    want_theta = part2[:, o_th:o_th + n_theta].cpu().numpy().astype(np.float64)
    assert np.isfinite(want_res).all() and np.isfinite(want_val).all() and np.isfinite(want_theta).all()
    # the forward outputs the merged stage left are those of the stand-alone forward kernels too
    got_qj = fs.ws_res[1][:, :, :B_res].cpu().numpy().astype(np.float64)
    want_qj = qj_res.cpu().numpy().astype(np.float64)

    s_got, s_want = theta.sum(axis=0), want_theta.sum(axis=0)
    tol_th = TOL * np.maximum(1.0, np.abs(s_want))
    e_res = np.abs(abar_res - want_res).max() / (TOL * max(1.0, np.abs(want_res).max()))
    e_val = np.abs(abar_val - want_val).max() / (TOL * max(1.0, np.abs(want_val).max()))
    e_th = (np.abs(s_got - s_want) / tol_th).max() if n_theta else 0.0
    e_qj = np.abs(got_qj - want_qj).max() / (TOL * max(1.0, np.abs(want_qj).max()))
    print(f"\nadjoint stage {ansatz}{n} r{B_res} v{B_val}: error / tolerance: abar_res {e_res:.3f}, abar_val {e_val:.3f}, "
          f"theta sums {e_th:.3f}, qjets {e_qj:.3f}; max |abar_res| {np.abs(want_res).max():.3g}, max |abar_val| "
          f"{np.abs(want_val).max():.3g}, max |theta sum| {np.abs(s_want).max() if n_theta else 0.0:.3g}")
    # the comparison is not vacuous: the references are not zero
    assert np.abs(want_res).max() > 100 * TOL and np.abs(want_val).max() > 100 * TOL
    assert n_theta == 0 or np.abs(s_want).max() > 100 * TOL
    assert e_qj < 1.0, e_qj
    assert e_res < 1.0, e_res
    assert e_val < 1.0, e_val
    assert e_th < 1.0, e_th
