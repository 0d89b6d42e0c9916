"""BalancedTrainer on the GPU against the float64 replays of tests/balanced_training.py: six steps on
tabulated_training's dataset, seed and sizes (the batches bit for bit, the histories of F and of the effective weights,
the held control), the first weight row to the bit, the balancer's parameters as views of the trained buffer, a saved and
reloaded run, and train(model, dataset=, balance=)."""
import os

import numpy as np
import pytest
import torch

import balanced_reference as BR
import balanced_training as BT
import tabulated_training as TT
from conftest import pkg
from test_gpu_balanced import device_weights
from test_gpu_fullsize import Log

pytestmark = pytest.mark.gpu


def _balancer():
    bal = pkg("nn.loss_balance").AdaptiveMultiLoss(scale=BR.SCALE)
    with torch.no_grad():
        for name, p in zip(BR.TERMS, BR.P0):
            bal.log_vars[name].fill_(p)
    return bal


def _dataset():
    TP = pkg("data.tabulated").TabulatedProblem
    import tabulated_reference as T
    Xr, rr, Xi, ui, Xb, ub = (torch.from_numpy(a) for a in BT.dataset_arrays())
    c_t, c_x, c_y, d_xx, d_yy = T.COEFFS
    return TP(Xr, rr, Xi, ui, Xb, ub, c_t=c_t, c_x=c_x, c_y=c_y, d_xx=d_xx, d_yy=d_yy, c_u=T.C_U)


def _trainer(gpu_device, tmp_path, ans, n, capacity=BT.STEPS):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    BalancedTrainer = pkg("trainer.balanced_train").BalancedTrainer

    class TmpLog(Log):
        def get_output_dir(self):
            return str(tmp_path)
    torch.manual_seed(1)
    model = Solver(TT.base_args(ans, n), TmpLog(), device=gpu_device)
    bal = _balancer()
    torch.manual_seed(TT.TRAINER_SEED_AT)
    tr = BalancedTrainer(model, BT.BATCH, _dataset(), bal, capacity=capacity)
    assert tr.fs.desc.sample_seed == TT.trainer_seed()
    return model, bal, tr


@pytest.mark.parametrize("case", list(BT.TRAIN_CASES))
def test_training_matches_the_fp64_replay_loss_and_weights(case, gpu_device, tmp_path):
    ans, n = BT.TRAIN_CASES[case]
    model, bal, tr = _trainer(gpu_device, tmp_path, ans, n)
    batches = []
    for _ in range(BT.STEPS):
        tr.sample()
        tr.step()
        fs = tr.fs
        Xv, tv = fs.X_val.cpu().numpy(), fs.target_val.cpu().numpy()
        batches.append((Xv[:BT.N_IC], Xv[BT.N_IC:BT.N_IC + BT.N_BC], fs.X_res.cpu().numpy()[:BT.BATCH], tv[:BT.N_IC],
                        tv[BT.N_IC:BT.N_IC + BT.N_BC], fs.target_res.cpu().numpy()[:BT.BATCH]))
    for got, want in zip(batches, BT.expected_batches()):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    ref, held = BT.training_reference(case, batches), BT.training_reference(case, batches, hold=True)
    got_l, got_w = np.array(tr.loss_history()), tr.weight_history().numpy().astype(np.float64)
    assert got_l.shape == (BT.STEPS,) and got_w.shape == (BT.STEPS, 3)
    err_l = np.abs(got_l - ref["loss"]).max() / (1e-4 * max(1.0, np.abs(ref["loss"]).max()))
    rel_w = lambda want: (np.abs(got_w - want) / (1e-4 * np.maximum(1.0, np.abs(want)))).max()
    print(case, "F", got_l, ref["loss"], "error / tolerance", err_l)
    print(case, "weights moved by", got_w[-1] - got_w[0], "reference", ref["weights"][-1] - ref["weights"][0])
    print(case, "largest weight error / tolerance", rel_w(ref["weights"]), "against the held balancer", rel_w(held["weights"]))
    assert err_l < 1.0 and rel_w(ref["weights"]) < 1.0
    assert rel_w(held["weights"]) > 1.0
    want0 = device_weights(gpu_device)
    assert np.array_equal(tr.weight_history().numpy()[0].view(np.uint32), want0.view(np.uint32))
    # the trained values are where the objects look for them: no copy
    own = [bal.log_vars[k] for k in BR.TERMS]
    assert all(p.data_ptr() == tr.flat.data_ptr() + 4 * (tr.NP + k) for k, p in enumerate(own)) and model._packed_ok()
    assert tr.flat.numel() == tr.NP + 3
    now = np.array([tr.weights()[k] for k in BR.TERMS])
    # the weights the NEXT step would use: one more Adam step (at most lr per p_k) behind the last row of the replay
    step = np.abs(np.asarray(BR.SCALE)) * 0.005 * 1.001
    assert (np.abs(np.log(now / ref["weights"][-1])) <= step + 1e-4).all()
    e = bal.weights()
    assert [e[k] * w for k, w in zip(BR.TERMS, BR.W)] == pytest.approx(list(now), rel=1e-6)


def test_a_saved_and_reloaded_run_continues_bit_for_bit(gpu_device, tmp_path):
    ans, n = BT.TRAIN_CASES["cascade4"]
    BalancedTrainer = pkg("trainer.balanced_train").BalancedTrainer
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    _, _, straight = _trainer(gpu_device, tmp_path, ans, n)
    for _ in range(BT.STEPS):
        straight.sample()
        straight.step()
    want_l, want_w = straight.loss_history(), straight.weight_history()

    model, bal, first = _trainer(gpu_device, tmp_path, ans, n)
    for _ in range(3):
        first.sample()
        first.step()
    path = os.path.join(str(tmp_path), "half.pth")
    model.save_state(path)
    bal_state = {k: v.cpu().clone() for k, v in bal.state_dict().items()}
    seed, sample_step = first.fs.desc.sample_seed, first.fs.desc.sample_step
    got_l, got_w = first.loss_history(), first.weight_history()

    state = Solver.load_state(path)
    torch.manual_seed(5)
    model2 = Solver(TT.base_args(ans, n), Log(), device=gpu_device)
    bal2 = pkg("nn.loss_balance").AdaptiveMultiLoss(scale=BR.SCALE)
    bal2.load_state_dict(bal_state)
    for name in ("preprocessor", "quantum_layer", "postprocessor"):
        getattr(model2, name).load_state_dict(state[name])
    BalancedTrainer.attach(model2, bal2)
    model2.optimizer.load_state_dict(state["optimizer"])          # the Adam moments of all NP + 3 entries
    model2.scheduler.load_state_dict(state["scheduler"])
    second = BalancedTrainer(model2, BT.BATCH, _dataset(), bal2, capacity=3)
    second.fs.set_sampler(seed)
    second.fs.desc.sample_step = sample_step
    for _ in range(3):
        second.sample()
        second.step()
    assert second.opt.read()["step"] == BT.STEPS
    got_l, got_w = got_l + second.loss_history(), torch.cat([got_w, second.weight_history()])
    assert np.array_equal(np.array(got_l, np.float32).view(np.uint32), np.array(want_l, np.float32).view(np.uint32))
    assert torch.equal(got_w, want_w)


def test_train_routes_to_the_balanced_trainer_and_logs(gpu_device, tmp_path):
    trainer = pkg("trainer.diffusion_train")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    lines = []

    class TmpLog(Log):
        def print(self, *a):
            lines.append(" ".join(str(x) for x in a))

        def get_output_dir(self):
            return str(tmp_path)
    ans, n = BT.TRAIN_CASES["cascade4"]
    torch.manual_seed(1)
    model = Solver(dict(TT.base_args(ans, n), print_every=2), TmpLog(), device=gpu_device)
    bal = _balancer()
    trainer.train(model, batch_size=BT.BATCH, dataset=_dataset(), balance=bal, update_lam=True)
    assert len(model.loss_history) == BT.STEPS and np.isfinite(model.loss_history).all()
    assert any("loss weights" in s for s in lines) and any("learned loss weights" in s for s in lines)
    p = np.array([float(bal.log_vars[k].detach()) for k in BR.TERMS])
    assert (p != np.asarray(BR.P0, np.float32)).all() and bal.log_vars["bc"].device.type == "cuda"
    # the balancer's moments went back to the torch optimiser with the model's
    st = model.optimizer.state[bal.log_vars["ic"]]
    assert float(st["step"]) == BT.STEPS and float(st["exp_avg_sq"]) > 0.0
