"""The fused step's own row reduction: the in-place first level (k_fold_rows) and both second levels (qc_reduce_rows
over the surviving rows; the FOLD branch of k_adam_fast, or qc_opt_reduce_rows + k_adam past 3072 columns) against the
float64 column sums of the step's own partial rows.

qc_fused_step_stage runs the five merged stages one by one and leaves the partial-row matrix ``part`` unfolded; the full
step runs the same kernels on the same inputs (no atomics), so its rows before the fold are bitwise the same.  The
host copy ``P`` of those rows is the reference: for every column c

    |flat[c] - sum_r P[r, c]|  <=  D * 2^-24 * sum_r |P[r, c]|,      D = ceil(rows / 512) + 48.

D is the longest chain of fp32 additions a term can pass through in a correct sum of these rows (csrc/qc_optim.hip):
k_fold_rows runs RS = min(rows, 32) row groups x 8 waves, each wave two chains (a0, a1) over every 2 x 8 x 32 = 512th
row, i.e. at most ceil(rows / 512) additions per chain; then a0 + a1 (1), the 8 waves (8), and the 32 surviving rows
added left to right in k_adam_fast<FOLD> (32) or through k_reduce_rows (2 per wave, 2 to join the four accumulators, 16
waves: 20).  That is ceil(rows / 512) + 41 at most; the issue fixed D with a margin of 7.  It is a rounding bound, not a
measured number: if the structure of the kernels changes, re-derive it here.

One lost or doubled row among thousands moves a column by 1/rows of its value, which the 5e-5 additivity checks of
tests/test_gpu_fullsize.py pass; here it fails, because every row has a column (its loss column: positive, about
1/rows of the column) whose entry exceeds four times that column's bound.  That detection condition is asserted on
the host for every row of every case.

The tail loop of k_fold_rows starts only beyond 8 x 32 x 8 = 2048 rows; the row counts below sit on both sides of
that, of RS = 32 and of the per-wave strides.  Model: cascade, n = 2, one layer, angle encoding (register family,
4-amplitude states), H = 13 (NP + 3 spans three 64-column blocks, the last one ragged) or H = 1024 (NP + 3 > 3072)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import pkg
from step_reference import step_inputs
from test_gpu_fullsize import Log, base_args

pytestmark = pytest.mark.gpu

QC_ERR_UNSUPPORTED = -2          # csrc/qc_types.h
ADAM_FAST_MAX = 3072             # k_adam_fast serves NP + 3 <= 3 x 1024
N_QUBITS, ANSATZ = 2, "cascade"
SALT = 3                         # seed of step_inputs; the detection condition held on this first seed for every case

TOTALS = [2, 31, 32, 33, 64, 65, 255, 256, 257, 511, 513, 2047, 2048, 2049, 2304, 2305, 2561, 4100]
# (H, rows_res, rows_val): one to three value tiles, both batches ragged
CASES = [(13, t - min(1 + i % 3, t - 1), min(1 + i % 3, t - 1)) for i, t in enumerate(TOTALS)] + [(1024, 31, 2), (1024, 2046, 3)]
TWO_STREAM = [(13, 32, 1), (13, 254, 3), (13, 2304, 1)]        # cases of CASES repeated in a QC_NO_MERGE=1 child process
_ROWS = {}                       # case of TWO_STREAM -> P of the merged run, shared by the tests below and never modified


def _sizes(rows_res, rows_val):
    B_res, B_val = 64 * rows_res - 5, 64 * rows_val - 3
    n_ic = B_val // 2 - 4
    return B_res, n_ic, B_val - n_ic


def _model(device, H, flat):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=N_QUBITS, num_quantum_layers=1, q_ansatz=ANSATZ, classic_network=[3, H, 1]), Log(),
                   device=device)
    eng = model._engine_for(device)
    with torch.no_grad():
        eng.flat.copy_(torch.from_numpy(flat))
    eng.refresh_gates()
    return model, eng


def _step(device, H, rows_res, rows_val, **opt_kw):
    """(model, engine, FusedStep with the case's seeded points loaded, merged-probe return code)."""
    engine, L = pkg("hip.engine"), pkg("hip.lib")
    B_res, n_ic, n_bc = _sizes(rows_res, rows_val)
    n_theta = pkg("circuits").params_per_layer(ANSATZ, N_QUBITS)
    flat, X_ic, X_bc, X_res = step_inputs(H, N_QUBITS, n_theta, B_res, n_ic, n_bc, salt=SALT)
    model, eng = _model(device, H, flat)
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, device, **opt_kw))
    assert fs.part.shape == (rows_res + rows_val, eng.NP + 3)
    fs.X_res[:B_res] = X_res.to(device)
    fs.X_val[:n_ic] = X_ic.to(device)
    fs.X_val[n_ic:] = X_bc.to(device)
    rc = eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_PRE_FWD, torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize()
    return model, eng, fs, rc


def _bound(P):
    rows = P.shape[0]
    D = math.ceil(rows / 512) + 48
    return D * 2.0 ** -24 * np.abs(P).sum(axis=0)


def _merged_rows(device, H, rows_res, rows_val):
    """The five merged stages one by one on a NaN-filled ``part``: (engine, FusedStep, P = the unfolded rows, float64)."""
    model, eng, fs, rc = _step(device, H, rows_res, rows_val)
    assert rc == 0                                               # the merged form: the stage entry point serves it
    st = torch.cuda.current_stream(device).cuda_stream
    fs.part.fill_(float("nan"))
    for stage in range(5):
        assert eng.lib.qc_fused_step_stage(C.byref(fs.desc), stage, st) == 0
    torch.cuda.synchronize()
    P = fs.part.cpu().numpy().astype(np.float64)
    assert P.shape == (rows_res + rows_val, eng.NP + 3)
    assert np.isfinite(P).all(), np.argwhere(~np.isfinite(P))[:4]        # the step rewrites its scratch every step
    if (H, rows_res, rows_val) in TWO_STREAM:
        _ROWS[H, rows_res, rows_val] = P
    return eng, fs, P


@pytest.mark.parametrize("H,rows_res,rows_val", CASES, ids=[f"H{h}_rows{a}+{b}" for h, a, b in CASES])
def test_fold_and_second_level_sum_the_steps_own_rows(H, rows_res, rows_val, gpu_device):
    L = pkg("hip.lib")
    rows = rows_res + rows_val
    eng, fs, P = _merged_rows(gpu_device, H, rows_res, rows_val)
    NP, ncols = eng.NP, eng.NP + 3
    assert ncols > 2 * 64 and ncols % 64, ncols                  # at least three column blocks, the last one ragged
    assert (ncols > ADAM_FAST_MAX) == (H == 1024)
    sums, bound = P.sum(axis=0), _bound(P)
    # detection condition: every row has a column where losing or doubling it exceeds the bound fourfold
    detect = (np.abs(P) > 4.0 * bound[None, :]).any(axis=1)
    assert detect.all(), np.argwhere(~detect)[:4]
    assert (P[:, NP:] >= 0).all() and (sums[NP:] > 0).all()

    # second level = qc_reduce_rows over the surviving rows (QC_PHASE_GRADS alone)
    fs.part.fill_(float("nan"))
    fs.flat_grad.fill_(float("nan"))
    fs.run(L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    flat = fs.flat_grad.cpu().numpy().astype(np.float64)
    ratio1 = np.abs(flat - sums) / np.where(bound > 0, bound, 1.0)       # (an all-zero column: error 0, ratio 0)
    assert (np.abs(flat - sums) <= bound).all(), (np.argmax(ratio1), ratio1.max())

    # second level inside the optimiser launch (GRADS | UPDATE in one call, no clipping: flat holds the unclipped sums)
    model2, eng2, fs2, rc2 = _step(gpu_device, H, rows_res, rows_val, max_norm=None)
    assert rc2 == 0
    fs2.part.fill_(float("nan"))
    fs2.flat_grad.fill_(float("nan"))
    fs2.run(L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE)
    torch.cuda.synchronize()
    flat2 = fs2.flat_grad.cpu().numpy().astype(np.float64)
    ratio2 = np.abs(flat2 - sums) / np.where(bound > 0, bound, 1.0)
    assert (np.abs(flat2 - sums) <= bound).all(), (np.argmax(ratio2), ratio2.max())
    rec = fs2.opt.read()
    w = np.array([2.0, 4.0, 2.0])                                # (residual, BC, IC) weights; columns NP.. = L_r, L_bc, L_ic
    assert abs(rec["loss"] - float(w @ sums[NP:])) <= float(w @ bound[NP:]), (rec["loss"], w @ sums[NP:])
    assert rec["step"] == 1 and np.isfinite(eng2.flat.cpu().numpy()).all()
    print(f"\nrow-fold H={H} rows={rows_res}+{rows_val}: max |flat - sum| / bound = {ratio1.max():.3f} (reduce_rows), "
          f"{ratio2.max():.3f} (update launch); min over rows of max_c |P| / bound = "
          f"{(np.abs(P) / np.where(bound > 0, bound, np.inf)[None, :]).max(axis=1).min():.1f}")


def two_stream_child(directory):
    """Runs in a fresh process with QC_NO_MERGE=1 (the switch is read once, at load): the two-stream step's flat vector
    against the column sums of the MERGED parent run's rows.  The comparison crosses two kernel forms (separate value and
    residual launches against the merged ones), whose rows agree to fp32 rounding but not bitwise, so the rounding
    bound above does not apply: the tolerance is the project's existing 1e-6 x max(1, |column sum|), as in
    test_step_after_update_matches_fresh_model, here taken per column.  Host-side control, in every case and for
    every row: the column sums with that row lost, and with it counted twice, are NOT within the tolerance of the
    step's vector, so one lost or doubled row is told apart at this tolerance too."""
    L = pkg("hip.lib")
    device = torch.device("cuda", 0)
    for H, rows_res, rows_val in TWO_STREAM:
        P = np.load(os.path.join(directory, f"P_{H}_{rows_res}_{rows_val}.npy"))
        sums = P.sum(axis=0)
        model, eng, fs, rc = _step(device, H, rows_res, rows_val)
        assert rc == QC_ERR_UNSUPPORTED, rc
        fs.part.fill_(float("nan"))
        fs.run(L.QC_PHASE_GRADS)
        torch.cuda.synchronize()
        flat = fs.flat_grad.cpu().numpy().astype(np.float64)
        tol = 1e-6 * np.maximum(1.0, np.abs(sums))                # per column
        err = np.abs(flat - sums)
        print(f"two-stream H={H} rows={rows_res}+{rows_val}: max |flat - sum| / tolerance = {np.max(err / tol):.3f}")
        assert (err < tol).all(), (H, rows_res, rows_val, np.max(err / tol))
        # one row of P lost or doubled is told apart at this tolerance: every row, every case
        lost = (np.abs((flat - sums)[None, :] + P) > tol[None, :]).any(axis=1)
        doubled = (np.abs((flat - sums)[None, :] - P) > tol[None, :]).any(axis=1)
        print(f"  control: min over rows of max_c |P| / tolerance = {(np.abs(P) / tol[None, :]).max(axis=1).min():.1f}")
        assert lost.all() and doubled.all(), (H, rows_res, rows_val, np.argwhere(~(lost & doubled))[:4])
    print("two-stream child: ok")


def test_two_stream_step_sums_the_merged_rows(gpu_device, tmp_path):
    d = str(tmp_path)
    for case in TWO_STREAM:
        P = _ROWS[case] if case in _ROWS else _merged_rows(gpu_device, *case)[2]
        np.save(os.path.join(d, "P_%d_%d_%d.npy" % case), P)
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {here!r}); import test_gpu_row_fold as t; t.two_stream_child({d!r})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, QC_NO_MERGE="1"), capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "two-stream child: ok" in r.stdout
