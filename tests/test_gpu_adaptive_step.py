"""FusedTrainer(dataset=, adaptive=) on the GPU: cascade n = 4 (merged form) and layered n = 7 (two-stream form), on a
dataset with a scalar operator and on one with a coefficient table.  After every step the residual batch must be the
restatement's gather (tests/adaptive_reference.py) from the CDF read back from the device, the value batch the uniform
step's, and the flat [grad | losses] vector bit-equal to that of a non-adaptive trainer fed the same batches: the
adaptive step runs the same kernels behind another gather, so nothing else may differ."""
import inspect

import numpy as np
import pytest
import torch

import adaptive_reference as AR
import coef_reference as CR
import tabulated_reference as T
import tabulated_training as TT
from conftest import pkg
from test_gpu_fullsize import Log

pytestmark = pytest.mark.gpu

DS_SIZES = (301, 40, 50)
B_RES, STEPS, EVERY = 70, 5, 2
N_VAL = B_RES // 3


def _dataset(table):
    from oracle import solver as osol
    TP = pkg("data.tabulated").TabulatedProblem
    g = torch.Generator().manual_seed(99)
    Xr, Xi, Xb = [(torch.tensor(b[0]) + (torch.tensor(b[1]) - torch.tensor(b[0])) * torch.rand(m, 3, generator=g)).float()
                  for b, m in zip((osol.BOX_DOM, osol.BOX_IC, osol.BOX_BC1), DS_SIZES)]
    f = lambda fn, X: torch.from_numpy(fn(X.numpy()))
    if table:
        return TP(Xr, f(T.r_star, Xr), Xi, f(T.u_star, Xi), Xb, f(T.u_star, Xb), coef_res=f(CR.coef_star, Xr))
    co = dict(zip(("c_t", "c_x", "c_y", "d_xx", "d_yy"), T.COEFFS), c_u=T.C_U)
    return TP(Xr, f(T.r_star, Xr), Xi, f(T.u_star, Xi), Xb, f(T.u_star, Xb), **co)


def _trainer(dev, ans, n, ds, tmp_path, adaptive=None):
    trainer = pkg("trainer.diffusion_train")
    Solver = pkg("nn.DVPDESolver").DVPDESolver

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(TT.base_args(ans, n), TmpLog(), device=dev)
    torch.manual_seed(TT.TRAINER_SEED_AT)
    tr = trainer.FusedTrainer(model, B_RES, capacity=STEPS, dataset=ds, adaptive=adaptive)
    assert tr.fs.desc.sample_seed == TT.trainer_seed()
    return tr


def _batches(tr):
    fs = tr.fs
    torch.cuda.synchronize()
    out = {"X_res": fs.X_res[:B_RES], "t_res": fs.target_res[:B_RES], "X_val": fs.X_val[:2 * N_VAL], "t_val": fs.target_val[:2 * N_VAL],
           "flat": fs.flat_grad}
    if fs.coef_mode:
        out["coef"] = fs.coef_res[:, :B_RES].t()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


@pytest.mark.parametrize("table", [False, True], ids=["scalar", "coef_table"])
@pytest.mark.parametrize("family", [("cascade", 4), ("layered", 7)], ids=["merged_n4", "two_stream_n7"])
def test_adaptive_step(family, table, gpu_device, tmp_path):
    AS = pkg("data.tabulated").AdaptiveSampling
    ans, n = family
    ds = _dataset(table)
    N = DS_SIZES[0]
    tr = _trainer(gpu_device, ans, n, ds, tmp_path, AS(power=2, floor=0.25, every=EVERY))
    uni = _trainer(gpu_device, ans, n, ds, tmp_path)          # the uniform step on the same seed
    fed = _trainer(gpu_device, ans, n, ds, tmp_path)          # a non-adaptive trainer fed the adaptive one's batches
    assert tr.fs.adapt is not None and uni.fs.adapt is None and tr.fs.coef_mode == table
    seed = tr.fs.desc.sample_seed
    Xr, r = ds.X_res.numpy(), ds.r.numpy()
    cdfs = []
    for k in range(STEPS):
        for t in (tr, uni):
            t.sample()
            t.step()
        got, plain = _batches(tr), _batches(uni)
        assert tr.fs.desc.sample_step == k + 1
        rec, cdf, coarse = AR.unpack(tr.fs.adapt_buf.cpu().numpy().view(np.uint8), N)
        cdfs.append(cdf)
        # the CDF is the rule's on the scores that are on the device, and the record is readable through the trainer
        scores = tr.dataset_scores().cpu().numpy()
        want = AR.build(scores, 2, 0.25)
        assert rec == want[0] and np.array_equal(cdf, want[1]) and np.array_equal(coarse, want[2])
        assert tr.adaptive_state() == {key: (float(v) if key == "max_p" else v) for key, v in rec.items()}
        assert np.isfinite(scores).all() and scores.max() > 0
        # the residual batch is the restatement's gather from that CDF; the value batch is the uniform step's
        idx = AR.indices(cdf, 0, B_RES, seed, k + 1)
        assert np.array_equal(got["X_res"], Xr[idx]) and np.array_equal(got["t_res"], r[idx])
        if table:
            assert np.array_equal(got["coef"], ds.coef_res.numpy()[idx])
        assert np.array_equal(got["X_val"], plain["X_val"]) and np.array_equal(got["t_val"], plain["t_val"])
        assert not np.array_equal(got["X_res"], plain["X_res"])          # the adaptive path was taken
        assert np.array_equal(plain["X_res"], Xr[T.dataset_indices(0, 0, B_RES, N, seed, k + 1)])
        # same batches through load_batches on a non-adaptive trainer: the same kernels, the same bits
        fed.load_batches(torch.from_numpy(got["X_val"][:N_VAL]), torch.from_numpy(got["X_val"][N_VAL:]), torch.from_numpy(got["X_res"]),
                         targets=(got["t_val"][:N_VAL], got["t_val"][N_VAL:], got["t_res"]),
                         coef=torch.from_numpy(np.ascontiguousarray(got["coef"])) if table else None)
        fed.step()
        again = _batches(fed)
        assert np.array_equal(got["flat"].view(np.uint32), again["flat"].view(np.uint32))
        assert np.isfinite(got["flat"]).all() and np.abs(got["flat"]).max() > 0
    # rescored ahead of steps 0, 2 and 4 only
    same = [np.array_equal(a, b) for a, b in zip(cdfs, cdfs[1:])]
    assert same == [True, False, True, False], same
    hist = np.array(tr.opt.loss_history(STEPS))
    assert hist.shape == (STEPS,) and np.isfinite(hist).all()
    assert np.array_equal(hist, np.array(fed.opt.loss_history(STEPS)))
    assert torch.equal(tr.eng.flat, fed.eng.flat)


def test_step_enqueues_without_reading_back():
    """No host synchronisation inside step(): by inspection of the code it runs."""
    trainer, engine = pkg("trainer.diffusion_train"), pkg("hip.engine")
    src = "".join(inspect.getsource(f) for f in (trainer.FusedTrainer.step, engine.FusedStep.run, engine.FusedStep.rescore,
                                                 engine.FusedStep._build_cdf))
    assert "rescore" in src and "qc_adapt_build" in src and "qc_dataset_scores" in src
    for word in (".cpu(", ".item(", ".tolist(", ".numpy(", "synchronize", "float(", "int("):
        assert word not in src, word
