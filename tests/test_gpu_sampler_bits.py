"""The device sampler bit for bit: qc_sample_collocation_faces (k_sample) and the draw folded into the merged step's
pre-forward stage against tests/philox_reference.py, the numpy restatement of Philox4x32-10 and of the draw documented in
include/qcpinn_hip.h (pinned to the Random123 known-answer vectors by tests/test_philox_reference.py).

Ranges, means and shard consistency (tests/test_gpu_solver.py) cannot tell a wrong multiplier, a swapped word or a
dropped high half of the counter from the documented generator; ``np.array_equal`` on the float32 points can.  Seeds,
steps and global point indices at and beyond 2^32 exercise the high counter and key words."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import philox_reference as PR
from conftest import pkg
from test_gpu_fullsize import Log, base_args

pytestmark = pytest.mark.gpu

N_RES, N_IC, N_BC = 1000, 130, 260
FACE_PTS = 65                                   # four faces of 65 points: off_bc + n_bc <= 4 * 65
# (seed, step, off_res, off_ic, off_bc): the plain case, a 64-bit seed, a step beyond 2^32, batches that straddle the
# 2^32 boundary of the global point index
SETTINGS = {
    "plain": (77, 5, 0, 0, 0),
    "seed64": (0x0123456789ABCDEF, 5, 0, 0, 0),
    "step_hi": (77, 2 ** 32 + 7, 0, 0, 0),
    "index_straddles_2_32": (77, 5, 2 ** 32 - 500, 2 ** 32 - 65, 2 ** 32 - 130),
}
FACE_MODES = {"one_face": 0, "four_faces": FACE_PTS, "random_face": PR.QC_BC_RANDOM_FACE}


@pytest.mark.parametrize("mode", list(FACE_MODES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_sampler_entry_point_matches_philox_restatement(setting, mode, gpu_device):
    L = pkg("hip.lib")
    lib = L.load()
    seed, step, off_res, off_ic, off_bc = SETTINGS[setting]
    face_pts = FACE_MODES[mode]
    if face_pts > 0:
        off_bc = 0                               # the face index g // face_pts stays within the four faces
        assert off_bc + N_BC <= 4 * face_pts
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    Xr = torch.full((N_RES + 8, 3), -7.0, device=gpu_device)          # eight sentinel points behind each batch
    Xv = torch.full((N_IC + N_BC + 8, 3), -7.0, device=gpu_device)
    L.check(lib.qc_sample_collocation_faces(Xr.data_ptr(), N_RES, off_res, Xv.data_ptr(), N_IC, off_ic, N_BC, off_bc,
                                            face_pts, seed, step, st), "qc_sample_collocation_faces")
    torch.cuda.synchronize()
    xr, xv = Xr.cpu().numpy(), Xv.cpu().numpy()
    want_r, want_v = PR.collocation(N_RES, off_res, N_IC, off_ic, N_BC, off_bc, face_pts, seed, step)
    assert np.array_equal(xr[:N_RES], want_r), np.argwhere(xr[:N_RES] != want_r)[:4]
    assert np.array_equal(xv[:N_IC + N_BC], want_v), np.argwhere(xv[:N_IC + N_BC] != want_v)[:4]
    assert np.all(xr[N_RES:] == -7.0) and np.all(xv[N_IC + N_BC:] == -7.0)
    # the batch has what the setting is about: all four faces / both sides of the index's word boundary
    bc = want_v[N_IC:]
    if mode != "one_face":
        assert all(np.any(bc[:, c] == v) for c, v in ((1, 0.0), (1, 1.0), (2, 0.0), (2, 1.0)))
    if setting == "index_straddles_2_32":
        assert off_res < 2 ** 32 < off_res + N_RES and off_ic < 2 ** 32 < off_ic + N_IC
        if face_pts <= 0:
            assert off_bc < 2 ** 32 < off_bc + N_BC


def test_plain_entry_point_is_the_one_face_draw(gpu_device):
    """qc_sample_collocation = qc_sample_collocation_faces with bc_face_points = 0."""
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    Xr = torch.empty(N_RES, 3, device=gpu_device)
    Xv = torch.empty(N_IC + N_BC, 3, device=gpu_device)
    seed, step = 0xFEDCBA9876543210, 2 ** 33 + 1
    L.check(lib.qc_sample_collocation(Xr.data_ptr(), N_RES, 2 ** 32 - 1, Xv.data_ptr(), N_IC, 3, N_BC, 2 ** 40, seed, step, st))
    torch.cuda.synchronize()
    want_r, want_v = PR.collocation(N_RES, 2 ** 32 - 1, N_IC, 3, N_BC, 2 ** 40, 0, seed, step)
    assert np.array_equal(Xr.cpu().numpy(), want_r) and np.array_equal(Xv.cpu().numpy(), want_v)


# ---- the step's own draw (QC_PHASE_SAMPLE | QC_PHASE_GRADS): folded into the merged pre-forward stage, or k_sample
# launched by the step in the two-stream form (QC_NO_MERGE=1, read once at load: a child process)
STEP_B_RES, STEP_N_IC, STEP_N_BC = 150, 40, 70              # ragged tiles; one value tile holds IC and BC points
STEP_SEED, STEP_AT = 0x0123456789ABCDEF, 2 ** 32 + 7
STEP_DRAWS = {"random_face": (PR.QC_BC_RANDOM_FACE, 2 ** 32 - 30, 7, 2 ** 32 - 11), "four_faces_40": (40, 2 ** 32 - 30, 7, 11)}


@pytest.mark.parametrize("draw", list(STEP_DRAWS))
def test_fused_step_draw_matches_philox_restatement(draw, gpu_device):
    L = pkg("hip.lib")
    engine = pkg("hip.engine")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    face_pts, off_res, off_ic, off_bc = STEP_DRAWS[draw]
    if face_pts > 0:
        assert off_bc + STEP_N_BC <= 4 * face_pts and off_bc % face_pts     # the shard starts inside a face
    torch.manual_seed(1)
    model = Solver(base_args(), Log(), device=gpu_device)       # cascade n = 4: register family
    eng = model._engine_for(gpu_device)
    eng.refresh_gates()
    fs = engine.FusedStep(eng, STEP_B_RES, STEP_N_IC, STEP_N_BC, engine.OptimState(eng.NP, 0.005, gpu_device))
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    merged = eng.lib.qc_fused_step_stage(C.byref(fs.desc), L.QC_STAGE_PRE_FWD, st) == 0
    assert merged == (os.environ.get("QC_NO_MERGE") != "1")
    fs.set_sampler(STEP_SEED, off_res=off_res, off_ic=off_ic, off_bc=off_bc, bc_face_points=face_pts)
    fs.desc.sample_step = STEP_AT - 1                           # run() advances the step counter before it draws
    fs.X_res.fill_(-7.0)
    fs.X_val.fill_(-7.0)
    fs.run(L.QC_PHASE_SAMPLE | L.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    assert fs.desc.sample_step == STEP_AT
    want_r, want_v = PR.collocation(STEP_B_RES, off_res, STEP_N_IC, off_ic, STEP_N_BC, off_bc, face_pts, STEP_SEED, STEP_AT)
    assert np.array_equal(fs.X_res.cpu().numpy(), want_r)
    assert np.array_equal(fs.X_val.cpu().numpy(), want_v)
    assert torch.isfinite(fs.flat_grad).all() and fs.flat_grad[-3:].min().item() > 0.0     # the step ran on those points


def test_two_stream_step_draw_matches_philox_restatement():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_sampler_bits.py"), "-m", "gpu", "-q", "-x",
                        "-k", "test_fused_step_draw_matches_philox_restatement and random_face"],
                       env=dict(os.environ, QC_NO_MERGE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]
