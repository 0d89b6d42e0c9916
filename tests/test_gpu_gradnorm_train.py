"""Training under gradient-norm weights on the GPU: six steps of GradNormTrainer (every = 2, cascade n = 4, H = 16,
128 + 64 + 64 points) against the float64 replay of tests/gradnorm_reference.py on the device's own batches, and
train(model, dataset=, gradnorm=) / train(model, gradnorm=) end to end.

Tolerance: the project's 1e-4 x max(1, |want|) on the loss history and on the history of the weights; the unit-weight
control must miss one of them."""
import numpy as np
import pytest
import torch

import gradnorm_reference as GR
import tabulated_reference as T
import tabulated_training as TT
from conftest import pkg
from test_gpu_fullsize import Log

pytestmark = pytest.mark.gpu


def _dataset():
    TP = pkg("data.tabulated").TabulatedProblem
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in TT.dataset_arrays())
    c_t, c_x, c_y, d_xx, d_yy = T.COEFFS
    return TP(Xr, rr, Xi, ui, Xb, ub, c_t=c_t, c_x=c_x, c_y=c_y, d_xx=d_xx, d_yy=d_yy, c_u=T.C_U)


def _logger(tmp_path, lines=None):
    class TmpLog(Log):
        def print(self, *a):
            if lines is not None:
                lines.append(" ".join(str(x) for x in a))

        def get_output_dir(self):
            return str(tmp_path)
    return TmpLog()


def test_six_steps_match_the_fp64_replay_loss_and_weights(gpu_device, tmp_path):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    GT, LB = pkg("trainer.gradnorm_train"), pkg("nn.loss_balance")
    c, steps = GR.TRAIN, GR.TRAIN["steps"]
    torch.manual_seed(1)
    model = Solver(GR.base_args(), _logger(tmp_path), device=gpu_device)
    torch.manual_seed(TT.TRAINER_SEED_AT)
    tr = GT.GradNormTrainer(model, c["B_res"], LB.GradNormWeighting(**GR.TRAIN_CFG), _dataset(), capacity=steps,
                            n_ic=c["n_ic"], n_bc=c["n_bc"])
    assert tr.fs.desc.sample_seed == TT.trainer_seed()
    batches = []
    for _ in range(steps):
        tr.sample()
        tr.step()
        fs = tr.fs
        Xv, tv = fs.X_val.cpu().numpy(), fs.target_val.cpu().numpy()
        batches.append((Xv[:c["n_ic"]], Xv[c["n_ic"]:c["n_ic"] + c["n_bc"]], fs.X_res.cpu().numpy()[:c["B_res"]], tv[:c["n_ic"]],
                        tv[c["n_ic"]:c["n_ic"] + c["n_bc"]], fs.target_res.cpu().numpy()[:c["B_res"]]))
    for got, want in zip(batches, GR.expected_batches()):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    ref, unit = GR.training_reference(batches), GR.training_reference(batches, unit=True)
    got_l, hist = np.array(tr.opt.loss_history()), tr.gradnorm_history().astype(np.float64)
    assert got_l.shape == (steps,) and hist.shape == (steps, 7)
    rel = lambda got, want: float((np.abs(got - want) / (1e-4 * np.maximum(1.0, np.abs(want)))).max())
    err_l, err_lam, err_stat = rel(got_l, ref["loss"]), rel(hist[:, :2], ref["hist"][:, :2]), rel(hist[:, 2:6], ref["hist"][:, 2:6])
    miss_l, miss_lam = rel(got_l, unit["loss"]), rel(hist[:, :2], unit["hist"][:, :2])
    print("loss", got_l, ref["loss"], "error / tolerance", err_l, "| lam", hist[:, :2].T, "error / tolerance", err_lam,
          "| statistics and weighted loss error / tolerance", err_stat, "| unit weights miss loss by", miss_l, "lam by", miss_lam,
          "| mean |G_c| (res, ic, bc)", ref["g_abs"][0])
    assert err_l < 1.0 and err_lam < 1.0 and err_stat < 1.0
    assert max(miss_l, miss_lam) > 1.0 and miss_lam > 1000.0
    assert hist[:, 6].tolist() == ref["hist"][:, 6].tolist() == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    assert np.array_equal(hist[1, :5], hist[0, :5]) and (hist[2, :2] != hist[0, :2]).all()
    st = tr.gradient_stats()
    assert st["n_updates"] == 3 and tr.weights() == (np.float32(hist[-1, 0]), np.float32(hist[-1, 1]))
    # the logged loss is the unweighted sum of the three parts
    (loss, l_r, l_bc, l_ic), _ = tr.losses()
    assert loss == pytest.approx(2.0 * l_r + 4.0 * l_bc + 2.0 * l_ic, rel=1e-6)


def test_train_routes_to_the_gradnorm_trainer_and_fills_the_histories(gpu_device, tmp_path):
    trainer, LB = pkg("trainer.diffusion_train"), pkg("nn.loss_balance")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    lines = []
    torch.manual_seed(1)
    model = Solver(dict(GR.base_args(), print_every=2, batch_size=192), _logger(tmp_path, lines), device=gpu_device)
    before = [p.detach().clone() for p in model.parameters()]
    trainer.train(model, batch_size=192, dataset=_dataset(), gradnorm=LB.GradNormWeighting(alpha=0.5, every=2), update_lam=True)
    steps = GR.TRAIN["steps"]
    assert len(model.loss_history) == steps and np.isfinite(model.loss_history).all()
    h = model.gradnorm_history
    assert h.shape == (steps, 7) and np.isfinite(h).all() and (h[:, :2] != 1.0).all() and (h[:, 2:5] > 0).all()
    assert h[:, 6].tolist() == [1.0, 0.0] * (steps // 2)
    assert any("gradient-norm weights: lam_bc" in s for s in lines) and any("gradient-norm loss weights" in s for s in lines)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))


def test_train_on_the_analytic_problem_trains_and_refuses_a_split_off_the_tile_boundary(gpu_device, tmp_path):
    trainer, LB = pkg("trainer.diffusion_train"), pkg("nn.loss_balance")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(dict(GR.base_args(), batch_size=128), _logger(tmp_path), device=gpu_device)
    with pytest.raises(ValueError, match="n_ic = 42"):
        trainer.train(model, batch_size=128, gradnorm=LB.GradNormWeighting())
    assert model.loss_history == []
    trainer.train(model, batch_size=192, gradnorm=LB.GradNormWeighting(alpha=0.5, every=1))
    h = model.gradnorm_history
    assert len(model.loss_history) == GR.TRAIN["steps"] and np.isfinite(model.loss_history).all()
    assert h.shape == (GR.TRAIN["steps"], 7) and np.isfinite(h).all() and (h[:, 6] == 1.0).all() and (h[:, :2] != 1.0).all()
