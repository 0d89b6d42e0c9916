"""qc_dataset_scores on the GPU against the float64 residual of tests/tabulated_reference.py and tests/coef_reference.py
(tests/adaptive_scores_reference.py): every circuit family and both encodings, the data step's residual and, for cascade
n = 4, the coefficient step's with c_3 != 0; dataset sizes 1, 65, B_res + 1 and 2 B_res + 3 at B_res = 64 (chunk tails and a
one-row chunk), sub-ranges behind sentinels, and two negative controls.

Tolerance.  Not invented: the yardstick is the parent's own residual, qc_post mode 0 through SolverEngine.forward, against
the same float64 channels on the same rows.  Its largest error relative to max |res| over the five cases is MODE0_ERR
(measured on an MI355X, printed by test_mode0_yardstick, which also asserts it has not moved past what is written here);
a score is the same arithmetic plus one subtraction and an abs, so it may err by 4 x that, relative to max |res| too."""
import ctypes as C

import numpy as np
import pytest
import torch

import adaptive_scores_reference as SR
import tabulated_reference as T
from conftest import pkg
from test_gpu_tabulated import _model, _tabulated_step
from test_gpu_coef import _coef_step

pytestmark = pytest.mark.gpu

# measured: reg_cascade2 3.81e-7, reg_cascade4 6.90e-7, wave_layered7 1.27e-6, hbm_cascade9 6.06e-7, amp_cascade4 2.344e-6
MODE0_ERR = 2.344e-6
TOL = 4 * MODE0_ERR
SENTINEL = -7.0


def _engine(dev, case):
    ans, n, L, enc = SR.CASES[case]
    flat, X, r, coef = SR.case_inputs(case)
    model, eng = _model(dev, ans, n, L, enc, flat)
    return model, eng, X, r, coef


def _scores(eng, dev, X, r, coef, N, row0=0, rows=None, c_u=T.C_U):
    """score tensor (N + 2 with sentinels) after one qc_dataset_scores call on the first N rows; coef None: data step."""
    L = pkg("hip.lib")
    fs = _coef_step(eng, SR.B_RES, 3, 2) if coef is not None else _tabulated_step(eng, SR.B_RES, 3, 2, T.COEFFS, c_u)
    keep = [torch.from_numpy(np.ascontiguousarray(a[:N])).to(dev) for a in (X, r)]
    fs.data.ds_X_res, fs.data.ds_r, fs.data.ds_n_res = keep[0].data_ptr(), keep[1].data_ptr(), N
    cf = None
    if coef is not None:
        keep.append(torch.from_numpy(np.ascontiguousarray(coef[:N])).to(dev))
        fs.coef.ds_coef = keep[2].data_ptr()
        cf = C.byref(fs.coef)
    out = torch.full((N + 2,), SENTINEL, dtype=torch.float32, device=dev)
    L.check(eng.lib.qc_dataset_scores(C.byref(fs.desc), C.byref(fs.data), cf, row0, N - row0 if rows is None else rows,
                                      out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "qc_dataset_scores")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def _rel(got, res, r):
    """largest |score - |res - r|| relative to max |res|."""
    want = np.abs(res - r.astype(np.float64))
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(res).max())


def test_mode0_yardstick(gpu_device):
    worst = 0.0
    for case in SR.CASES:
        model, eng, X, r, coef = _engine(gpu_device, case)
        eng.coeffs = T.COEFFS
        _, res, _, _ = eng.forward(torch.from_numpy(X).to(gpu_device), 6)
        eng.coeffs = None
        want = SR.residuals(case)["mode0"]
        err = float(np.abs(res.cpu().numpy()[:, 0].astype(np.float64) - want).max() / np.abs(want).max())
        print(case, "qc_post mode 0: largest error relative to max |res| =", err)
        worst = max(worst, err)
    print("MODE0_ERR measured:", worst)
    assert worst <= MODE0_ERR


@pytest.mark.parametrize("case", list(SR.CASES))
def test_scores_match_fp64(case, gpu_device):
    model, eng, X, r, coef = _engine(gpu_device, case)
    ref = SR.residuals(case)
    kinds = [("data", None)] + ([("coef", coef)] if case == "reg_cascade4" else [])
    for kind, table in kinds:
        res = ref[kind]
        assert np.abs(res).max() > 0.1 and (table is None or np.abs(table[:, 6]).max() > 0.5)
        for N in SR.SIZES:
            got = _scores(eng, gpu_device, X, r, table, N)
            assert (got[N:] == SENTINEL).all() and np.isfinite(got[:N]).all() and (got[:N] >= 0).all()
            err = np.abs(got[:N].astype(np.float64) - np.abs(res[:N] - r[:N].astype(np.float64))).max() / np.abs(res).max()
            print(case, kind, N, "score error relative to max |res| =", float(err))
            assert err <= TOL
        # a sub-range leaves the other entries alone and equals the full call there
        N = SR.N_MAX
        full = _scores(eng, gpu_device, X, r, table, N)
        part = _scores(eng, gpu_device, X, r, table, N, row0=60, rows=66)
        assert (part[:60] == SENTINEL).all() and (part[126:] == SENTINEL).all()
        assert np.array_equal(part[60:126], full[60:126])
        # negative controls: targets rolled by one row; c_u = 0 (data step) or the table's c_u column zeroed
        bad = _rel(full[:N], res, np.roll(r, 1))
        print(case, kind, "rolled targets differ by", bad, "relative to max |res|")
        assert bad > TOL, bad
        if table is None:
            no_cu = _scores(eng, gpu_device, X, r, None, N, c_u=0.0)
        else:
            t0 = table.copy()
            t0[:, 0] = 0.0
            no_cu = _scores(eng, gpu_device, X, r, t0, N)
        bad = _rel(no_cu[:N], res, r)
        print(case, kind, "c_u = 0 differs by", bad, "relative to max |res|")
        assert bad > TOL, bad


def test_refusals_with_a_real_descriptor(gpu_device):
    """A descriptor and a dataset that are accepted (rc 0, scores written), then ONE fault each: -1 and nothing written.
    The same for qc_fused_pinn_adaptive_step."""
    L = pkg("hip.lib")
    model, eng, X, r, coef = _engine(gpu_device, "reg_cascade4")
    N = 70
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    for table in (None, coef):
        fs = _coef_step(eng, SR.B_RES, 3, 2) if table is not None else _tabulated_step(eng, SR.B_RES, 3, 2, T.COEFFS, T.C_U)
        keep = [torch.from_numpy(np.ascontiguousarray(a[:N])).to(gpu_device) for a in (X, r, coef)]
        fs.data.ds_X_res, fs.data.ds_r, fs.data.ds_n_res = keep[0].data_ptr(), keep[1].data_ptr(), N
        if table is not None:
            fs.coef.ds_coef = keep[2].data_ptr()
        out = torch.full((N,), SENTINEL, dtype=torch.float32, device=gpu_device)
        ref = lambda v: None if v is None else C.byref(v)
        cf = fs.coef if table is not None else None

        def call(desc=fs.desc, data=fs.data, coef_=cf, row0=0, rows=N, score=out.data_ptr()):
            return eng.lib.qc_dataset_scores(ref(desc), ref(data), ref(coef_), row0, rows, score, st)

        def broken(src, **kw):
            t = type(src).from_buffer_copy(src)
            for k_, v in kw.items():
                setattr(t, k_, v)
            return t
        assert call() == 0
        torch.cuda.synchronize()
        assert (out.cpu().numpy() >= 0).all()
        out.fill_(SENTINEL)
        assert call(desc=None) == -1 and call(data=None) == -1 and call(score=None) == -1
        for kw in (dict(row0=-1), dict(rows=0), dict(rows=N + 1), dict(row0=N, rows=1), dict(row0=5, rows=N - 4)):
            assert call(**kw) == -1, kw
        for kw in (dict(B_res=0), dict(ajets_res_dev=None), dict(qjets_res_dev=None), dict(qbar_res_dev=None), dict(params_dev=None),
                   dict(trig_dev=None), dict(prog=None)):
            assert call(desc=broken(fs.desc, **kw)) == -1, kw
        for pb in (0, 1, 2, 4):
            d = broken(fs.desc)
            d.pde.problem = pb
            assert call(desc=d) == -1
        for kw in (dict(ds_X_res=None), dict(ds_r=None), dict(ds_n_res=0), dict(ds_n_res=2 ** 31)):
            assert call(data=broken(fs.data, **kw)) == -1, kw
        if table is not None:
            assert call(coef_=broken(fs.coef, ds_coef=None)) == -1
        torch.cuda.synchronize()
        assert (out == SENTINEL).all()
        # the step: accepted with a buffer over the dataset's rows, refused with one fault
        fs.set_adaptive(2, 0.25)
        fs.set_dataset([(keep[0], keep[1]), (keep[0][:9], keep[1][:9]), (keep[0][:5], keep[1][:5])], keep[2] if table is not None else None)
        assert fs.adapt is not None and fs.adapt.n_rows == N          # re-armed for the new rows
        both = L.QC_PHASE_SAMPLE | L.QC_PHASE_GRADS
        step = lambda ad, desc=fs.desc, data=fs.data: eng.lib.qc_fused_pinn_adaptive_step(ref(desc), ref(data), ref(cf), ref(ad), both, st)
        assert step(fs.adapt) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(fs.flat_grad).all()
        fs.flat_grad.fill_(float("nan"))
        fs.X_res.fill_(float("nan"))
        assert step(None) == -1 and step(fs.adapt, data=None) == -1
        for kw in (dict(adapt_dev=None), dict(adapt_dev=fs.adapt_buf.data_ptr() + 4), dict(n_rows=N - 1), dict(n_rows=N + 1)):
            assert step(broken(fs.adapt, **kw)) == -1, kw
        assert step(fs.adapt, desc=broken(fs.desc, B_res=0)) == -1
        assert step(fs.adapt, data=broken(fs.data, target_res_dev=None)) == -1          # what the data step refuses
        torch.cuda.synchronize()
        assert torch.isnan(fs.flat_grad).all() and torch.isnan(fs.X_res).all()
        fs.clear_adaptive()
        assert fs.adapt is None
