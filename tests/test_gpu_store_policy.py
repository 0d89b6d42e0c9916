"""Write-through stores of stage outputs (qc_store_wt, csrc/qc_common.h): what one launch stores that way, the next
launch reads with plain loads, also from another XCD and also where a buffer is used again.

(a) tools/ubench/store_policy, the stand-alone program built next to the library: 1280 blocks write a buffer with
    qc_store_wt (4- and 8-byte forms; full waves, lane 0 alone, lanes 0..62), a separate launch reads block (b + 3)'s
    region with plain loads; then the buffer is rewritten by plain stores and read again, and rewritten by qc_store_wt
    and read again.  Integer-valued data, compared word for word.  A missing binary is a failure.

(b) The step's stage chain on re-used buffers.  A FusedStep (the construction of tests/test_gpu_adjoint_stage_shapes.py)
    runs stages 0..4 through qc_fused_step_stage on NaN-poisoned workspaces; then torch (plain stores of other kernels)
    writes other weights and points, drawn with another ``salt``, into the same FusedStep and the stages run again on
    the buffers the first run left.  After each run the stand-alone calls (qc_post mode 2 on both pipelines,
    qc_forward_jets_keep + qc_backward_jets_kept, qc_forward_expval + qc_backward_expval, qc_pre_backward on both
    pipelines) run on the inputs the stages left, into fresh outputs.  Compared: ``abar`` of both pipelines and the
    column sums of the partial rows (all columns: pre network, post network, theta, the three loss sums), with the
    tolerance of that file, 1e-6 x max(1, |reference|): per array for ``abar``, per column for the sums.  No NaN may
    survive in a live entry.
    Programs: cascade n = 2 and n = 4, H = 50.  Shapes (B_res, B_val): (1, 1), (65, 193), (129, 1)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from step_reference import step_inputs
from test_gpu_adjoint_stage_shapes import H, TOL, _step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UBENCH = os.path.join(ROOT, "tools", "ubench", "store_policy")
PROGRAMS = [("cascade", 2), ("cascade", 4)]
SHAPES = [(1, 1), (65, 193), (129, 1)]
SALT_2 = 9          # the second run's draw (the first is _step's, salt 4)


def test_store_policy_program():
    assert os.path.exists(UBENCH), f"{UBENCH} is not built (csrc/Makefile builds it next to the library)"
    r = subprocess.run([UBENCH], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("pass ")]
    assert len(lines) == 3 and all(" PASS " in ln for ln in lines), r.stdout[-3000:]
    assert [int(ln.split()[1]) for ln in lines] == [1, 2, 3]
    assert "bad=0" in r.stdout.splitlines()


def _run_and_compare(name, eng, fs, B_res, B_val, device):
    """stages 0..4 on the FusedStep as it stands, then the stand-alone calls on what they left"""
    lib, d, n = eng.lib, fs.desc, fs.n
    st = torch.cuda.current_stream(device).cuda_stream
    rows_res, rows_val = (B_res + 63) // 64, (B_val + 63) // 64
    rows = rows_res + rows_val
    for stage in range(5):
        assert lib.qc_fused_step_stage(C.byref(d), stage, st) == 0, stage      # the merged form serves these sizes
    torch.cuda.synchronize()
    P = fs.part[:rows].cpu().numpy().astype(np.float64)
    abar_res = fs.ws_res[3][:, :, :B_res].cpu().numpy().astype(np.float64)
    abar_val = fs.ws_val[3][0, :, :B_val].cpu().numpy().astype(np.float64)
    live = {"partial rows": P, "abar_res": abar_res, "abar_val": abar_val}
    for k in range(3):   # angle jets, <Z> jets, their cotangents: the hand-offs between the stages
        live[f"ws_res[{k}]"] = fs.ws_res[k][:, :, :B_res].cpu().numpy()
        live[f"ws_val[{k}]"] = fs.ws_val[k][0, :, :B_val].cpu().numpy()
    for what, a in live.items():
        assert np.isfinite(a).all(), (name, what, np.argwhere(~np.isfinite(a))[:4])

    f = dict(dtype=torch.float32, device=device)
    nan = float("nan")
    part2 = torch.full((rows, fs.stride), nan, **f)
    chi = torch.full((max(int(d.circ_ws_bytes), 4) // 4,), nan, **f)
    out_r, out_v = torch.full((2, B_res), nan, **f), torch.full((B_val,), nan, **f)
    qb_res, qb_val = torch.full((6, n, B_res), nan, **f), torch.full((n, B_val), nan, **f)
    qj_res, qj_val = torch.full((6, n, B_res), nan, **f), torch.full((n, B_val), nan, **f)
    ab_res, ab_val = torch.full((6, n, B_res), nan, **f), torch.full((n, B_val), nan, **f)
    pde, th2 = C.byref(d.pde), part2.data_ptr() + 4 * eng.theta_off
    assert lib.qc_post(2, d.X_res_dev, d.params_dev, d.H, d.n, d.n_theta, pde, d.qjets_res_dev, out_r.data_ptr(),
                       out_r.data_ptr() + 4 * B_res, None, None, qb_res.data_ptr(), part2.data_ptr(), fs.stride, 0, B_res, 6,
                       st) == 0
    assert lib.qc_post(2, d.X_val_dev, d.params_dev, d.H, d.n, d.n_theta, pde, d.qjets_val_dev, out_v.data_ptr(), None, None,
                       None, qb_val.data_ptr(), part2.data_ptr(), fs.stride, rows_res, B_val, 1, st) == 0
    assert lib.qc_forward_jets_keep(d.prog, d.trig_dev, d.umat_dev, d.ajets_res_dev, qj_res.data_ptr(), B_res, chi.data_ptr(),
                                    st) == 0
    assert lib.qc_backward_jets_kept(d.prog, d.trig_dev, d.umat_dev, d.ajets_res_dev, d.qbar_res_dev, ab_res.data_ptr(), th2,
                                     fs.stride, 0, B_res, chi.data_ptr(), st) == 0
    assert lib.qc_forward_expval(d.prog, d.trig_dev, d.umat_dev, d.ajets_val_dev, qj_val.data_ptr(), B_val, None, 0, st) == 0
    assert lib.qc_backward_expval(d.prog, d.trig_dev, d.umat_dev, d.ajets_val_dev, d.qbar_val_dev, ab_val.data_ptr(), th2,
                                  fs.stride, rows_res, B_val, None, 0, st) == 0
    assert lib.qc_pre_backward(d.X_res_dev, d.params_dev, d.H, d.n, d.n_theta, d.abar_res_dev, part2.data_ptr(), fs.stride, 0,
                               B_res, 6, st) == 0
    assert lib.qc_pre_backward(d.X_val_dev, d.params_dev, d.H, d.n, d.n_theta, d.abar_val_dev, part2.data_ptr(), fs.stride,
                               rows_res, B_val, 1, st) == 0
    torch.cuda.synchronize()
    P2 = part2.cpu().numpy().astype(np.float64)
    want_res, want_val = ab_res.cpu().numpy().astype(np.float64), ab_val.cpu().numpy().astype(np.float64)
    for what, a in (("stand-alone rows", P2), ("stand-alone abar_res", want_res), ("stand-alone abar_val", want_val)):
        assert np.isfinite(a).all(), (name, what, np.argwhere(~np.isfinite(a))[:4])

    s_got, s_want = P.sum(axis=0), P2.sum(axis=0)
    e_cols = np.abs(s_got - s_want) / (TOL * np.maximum(1.0, np.abs(s_want)))
    e_res = np.abs(abar_res - want_res).max() / (TOL * max(1.0, np.abs(want_res).max()))
    e_val = np.abs(abar_val - want_val).max() / (TOL * max(1.0, np.abs(want_val).max()))
    o_th, NP = eng.theta_off, eng.NP
    blocks = {"network columns": slice(0, o_th), "theta columns": slice(o_th, NP), "loss sums": slice(NP, NP + 3)}
    print(f"\n{name}: error / tolerance: abar_res {e_res:.3f}, abar_val {e_val:.3f}, "
          + ", ".join(f"{k} {e_cols[s].max():.3f}" for k, s in blocks.items())
          + f"; max |abar_res| {np.abs(want_res).max():.3g}, max |abar_val| {np.abs(want_val).max():.3g}, "
          + f"max |column sum| {np.abs(s_want).max():.3g}")
    # the comparison is not vacuous
    assert np.abs(want_res).max() > 100 * TOL and np.abs(want_val).max() > 100 * TOL and np.abs(s_want).max() > 100 * TOL
    assert e_res < 1.0, e_res
    assert e_val < 1.0, e_val
    assert e_cols.max() < 1.0, (int(e_cols.argmax()), float(e_cols.max()))
    return s_want


@pytest.mark.parametrize("B_res,B_val", SHAPES, ids=[f"r{a}_v{b}" for a, b in SHAPES])
@pytest.mark.parametrize("ansatz,n", PROGRAMS, ids=[f"{a}{n}" for a, n in PROGRAMS])
def test_stage_chain_on_reused_buffers(ansatz, n, B_res, B_val, gpu_device):
    model, eng, fs = _step(gpu_device, ansatz, n, B_res, B_val)
    nan = float("nan")
    for t in (fs.part, fs.ws_res, fs.ws_val):
        t.fill_(nan)
    fs.step_ws.fill_(0xFF)      # (the final-state store: NaN as float32)
    first = _run_and_compare(f"{ansatz}{n} r{B_res} v{B_val} run 1 (poisoned workspaces)", eng, fs, B_res, B_val, gpu_device)

    # other weights and points into the same step: torch's kernels write them, with plain stores
    n_ic = (B_val + 1) // 2
    n_bc = B_val - n_ic
    flat, X_ic, X_bc, X_res = step_inputs(H, n, eng.n_theta, B_res, n_ic, n_bc, salt=SALT_2)
    with torch.no_grad():
        eng.flat.copy_(torch.from_numpy(flat))
    eng.refresh_gates()
    fs.X_res[:B_res] = X_res.to(gpu_device)
    fs.X_val[:n_ic] = X_ic.to(gpu_device)
    fs.X_val[n_ic:B_val] = X_bc.to(gpu_device)
    second = _run_and_compare(f"{ansatz}{n} r{B_res} v{B_val} run 2 (buffers of run 1)", eng, fs, B_res, B_val, gpu_device)
    assert np.abs(second - first).max() > 100 * TOL      # the second run is another problem, not the first one's leftovers
