"""Training M = 4 models of the reference's configuration (cascade, 4 qubits, H = 50, batch_size 64: 64 + 21 + 21 points
drawn on the device) as one ensemble: distinct initialisations, learning rates (0.005, 0.002, 0.01, 0.005), one member
with loss weights (1, 10, 1) and one with D = 0.05 (both through the device tables), 20 steps.

Every member must train as the single-model fused step trains it alone with the sampler key seed + m: loss history within
1e-4 x max(1, max |loss|) and final parameters within 2e-3, the bounds tests/test_gpu_hybrid_pinn.py uses for such a
comparison; ``train_ensemble`` must leave every model as ``train`` leaves it (loss_history, optimiser and scheduler state);
``predict`` is the mean and standard deviation of the members' forward."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from test_gpu_fullsize import Log, base_args

pytestmark = pytest.mark.gpu

M, B, STEPS = 4, 64, 20
LRS = (0.005, 0.002, 0.01, 0.005)
WEIGHTS = [None, (1.0, 10.0, 1.0), None, None]
PDES = [None, None, dict(D=0.05, vx=1.0, vy=1.0, problem=0), None]
TOL_LOSS, TOL_PARAM = 1e-4, 2e-3


def _model(dev, m):
    torch.manual_seed(100 + m)
    return pkg("nn.DVPDESolver").DVPDESolver(base_args(lr=LRS[m], epochs=STEPS - 1), Log(), device=dev)


def _single_trainer(model, m, seed):
    """The single-model trainer of member m: its own weights and operator, the sampler key seed + m."""
    kw = {} if WEIGHTS[m] is None else {"loss_weights": WEIGHTS[m]}
    tr = pkg("trainer.diffusion_train").FusedTrainer(model, B, capacity=STEPS, pde=PDES[m], **kw)
    tr.fs.set_sampler(seed + m)
    return tr


@functools.lru_cache(maxsize=None)
def _trained_alone(dev, seed):
    """Every member trained by the single-model loop (what ``train`` runs), with its trainer."""
    T = pkg("trainer.diffusion_train")
    out = []
    for m in range(M):
        model = _model(dev, m)
        tr = T.run_fused_loop(model, _single_trainer(model, m, seed), "single", B)
        out.append((model, tr))
    return out


def _close_history(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == (STEPS,)
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    assert err < TOL_LOSS, (err, got, want)
    return err


def test_members_train_as_single_models(gpu_device):
    ET = pkg("trainer.ensemble_train")
    models = [_model(gpu_device, m) for m in range(M)]
    torch.manual_seed(5)
    tr = ET.EnsembleTrainer(models, B, capacity=STEPS, pde=PDES, loss_weights=WEIGHTS)
    assert tr.fs.pde_table is not None and tr.fs.hyper_table is not None
    for _ in range(STEPS):
        tr.sample()
        tr.step()
    torch.cuda.synchronize()
    alone = _trained_alone(gpu_device, tr.seed)
    NP = tr.fs.NP
    hists = [np.array(tr.loss_history(m, STEPS)) for m in range(M)]
    for m, (model, single) in enumerate(alone):
        err = _close_history(hists[m], single.loss_history(STEPS))
        diff = (tr.fs.params[m, :NP] - model._flat).abs().max().item()
        print(f"member {m}: loss history error {err:.2e} of {TOL_LOSS}, parameters differ by {diff:.2e} of {TOL_PARAM}")
        assert diff < TOL_PARAM
        rec = tr.fs.read(m)
        assert rec["step"] == STEPS and rec["hist_base"] == 0
        assert rec["lr"] == np.float32(LRS[m])                  # patience 1000: the scheduler has not moved it
        assert rec["loss"] == pytest.approx(hists[m][-1])
    # the members are different trainings: no history equals another's
    assert all(np.abs(hists[a] - hists[b]).max() > 10 * TOL_LOSS for a in range(M) for b in range(a))


def test_train_ensemble_writes_every_model_back(gpu_device):
    ET = pkg("trainer.ensemble_train")
    models = [_model(gpu_device, m) for m in range(M)]
    torch.manual_seed(5)
    tr = ET.train_ensemble(models, B, pde=PDES, loss_weights=WEIGHTS)
    alone = _trained_alone(gpu_device, tr.seed)
    for m, (ref, _) in enumerate(alone):
        model = models[m]
        _close_history(model.loss_history, ref.loss_history)
        got, want = model.optimizer.state_dict(), ref.optimizer.state_dict()
        assert got["param_groups"][0]["lr"] == want["param_groups"][0]["lr"] == float(np.float32(LRS[m]))
        assert got["state"].keys() == want["state"].keys() and len(got["state"]) == 9
        for k in want["state"]:
            assert float(got["state"][k]["step"]) == float(want["state"][k]["step"]) == STEPS
            for name in ("exp_avg", "exp_avg_sq"):
                assert (got["state"][k][name] - want["state"][k][name]).abs().max().item() < TOL_PARAM, (m, k, name)
        assert model.scheduler.num_bad_epochs == ref.scheduler.num_bad_epochs
        assert model.scheduler.last_epoch == ref.scheduler.last_epoch == STEPS
        assert model.scheduler.best == pytest.approx(ref.scheduler.best, rel=TOL_LOSS, abs=TOL_LOSS)
        for (k, p), q in zip(model.state_dict().items(), ref.state_dict().values()):
            assert (p - q).abs().max().item() < TOL_PARAM, (m, k)
        assert model._packed_ok()                                # still a normal DVPDESolver over one flat buffer
    # predict: mean and standard deviation of the members' own forward
    g = torch.Generator().manual_seed(3)
    X = torch.rand(37, 3, generator=g).to(gpu_device)
    mean, std = tr.predict(X)
    with torch.no_grad():
        u = torch.stack([model(X) for model in models])
    assert mean.shape == std.shape == (37, 1)
    assert torch.allclose(mean, u.mean(0), rtol=0, atol=1e-6) and torch.allclose(std, u.std(0, unbiased=False), rtol=0, atol=1e-6)
    assert std.max().item() > 1e-3                               # four different models
