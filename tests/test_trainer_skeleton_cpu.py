"""The trainers' shared skeleton (trainer/diffusion_train.py: StepTrainer, DatasetTrainer, fill_batches) on stub steps:
no GPU and no library call.  A trainer is made without its constructor, its ``fs`` is a namespace of CPU tensors at a
sentinel with a recording ``run``.  EXPECTED holds what the methods of the commit before the skeleton was shared left in
those buffers for the same stubs and inputs (each trainer's own ``load_batches`` / ``sample`` / ``step`` called on the same
stub); the shared code must leave the same, raise the same texts for the same faults, and run the same phases."""
import re
import types

import pytest
import torch

from conftest import pkg

N_IC, N_BC, B_RES, K, N_EQ, COLS = 2, 3, 5, 2, 3, 7
SENTINEL = -1.0
GRADS, UPDATE, SAMPLE = 1, 2, 4

# recorded at the parent commit; every element the parent did not write stays at the sentinel
_X_VAL = [[100, 101, 102], [103, 104, 105], [200, 201, 202], [203, 204, 205], [206, 207, 208], [-1, -1, -1]]
_X_RES = [[300, 301, 302], [303, 304, 305], [306, 307, 308], [309, 310, 311], [312, 313, 314], [-1, -1, -1]]
_U_VAL = [[1000, 1002, 2000, 2002, 2004, -1], [1001, 1003, 2001, 2003, 2005, -1]]
_X_VAL_DRAWN = [[100, 101, 102], [109, 110, 111], [209, 210, 211], [200, 201, 202], [209, 210, 211], [-1, -1, -1]]
_X_RES_DRAWN = [[306, 307, 308], [318, 319, 320], [309, 310, 311], [312, 313, 314], [315, 316, 317], [-1, -1, -1]]
EXPECTED = {
    "load_inverse": {"X_val": _X_VAL, "X_res": _X_RES, "target_val": [10, 11, 20, 21, 22, -1],
                     "target_res": [30, 31, 32, 33, 34, -1]},
    "load_system_True": {"X_val": _X_VAL, "X_res": _X_RES, "target_val": _U_VAL,
                         "target_res": [[3000, 3003, 3006, 3009, 3012, -1], [3001, 3004, 3007, 3010, 3013, -1],
                                        [3002, 3005, 3008, 3011, 3014, -1]]},
    "load_system_False": {"X_val": _X_VAL, "X_res": _X_RES, "target_val": _U_VAL},
    "load_fused_0": {"X_val": _X_VAL, "X_res": _X_RES, "target_val": [10, 11, 20, 21, 22, -1],
                     "target_res": [30, 31, 32, 33, 34, -1],
                     "coef_res": [[5000, 5007, 5014, 5021, 5028, -1], [5001, 5008, 5015, 5022, 5029, -1],
                                  [5002, 5009, 5016, 5023, 5030, -1], [5003, 5010, 5017, 5024, 5031, -1],
                                  [5004, 5011, 5018, 5025, 5032, -1], [5005, 5012, 5019, 5026, 5033, -1],
                                  [5006, 5013, 5020, 5027, 5034, -1]]},
    "load_fused_1": {"X_val": [[106, 107, 108], [209, 210, 211], [212, 213, 214], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]],
                     "X_res": [[315, 316, 317], [318, 319, 320], [321, 322, 323], [324, 325, 326], [-1, -1, -1], [-1, -1, -1]],
                     "target_val": [12, 23, 24, -1, -1, -1], "target_res": [35, 36, 37, 38, -1, -1],
                     "coef_res": [[5035, 5042, 5049, 5056, -1, -1], [5036, 5043, 5050, 5057, -1, -1],
                                  [5037, 5044, 5051, 5058, -1, -1], [5038, 5045, 5052, 5059, -1, -1],
                                  [5039, 5046, 5053, 5060, -1, -1], [5040, 5047, 5054, 5061, -1, -1],
                                  [5041, 5048, 5055, 5062, -1, -1]]},
    "sample_scalar": {"X_val": _X_VAL_DRAWN, "X_res": _X_RES_DRAWN, "target_val": [10, 13, 23, 20, 23, -1],
                      "target_res": [32, 36, 33, 34, 35, -1], "next_draw": 101},
    "sample_rows": {"X_val": _X_VAL_DRAWN, "X_res": _X_RES_DRAWN,
                    "target_val": [[1000, 1006, 2006, 2000, 2006, -1], [1001, 1007, 2007, 2001, 2007, -1]],
                    "target_res": [[3006, 3018, 3009, 3012, 3015, -1], [3007, 3019, 3010, 3013, 3016, -1],
                                   [3008, 3020, 3011, 3014, 3017, -1]], "next_draw": 101},
    "sample_coef": {"X_val": _X_VAL_DRAWN, "X_res": _X_RES_DRAWN, "target_val": [10, 13, 23, 20, 23, -1],
                    "target_res": [32, 36, 33, 34, 35, -1],
                    "coef_res": [[5014, 5042, 5021, 5028, 5035, -1], [5015, 5043, 5022, 5029, 5036, -1],
                                 [5016, 5044, 5023, 5030, 5037, -1], [5017, 5045, 5024, 5031, 5038, -1],
                                 [5018, 5046, 5025, 5032, 5039, -1], [5019, 5047, 5026, 5033, 5040, -1],
                                 [5020, 5048, 5027, 5034, 5041, -1]], "next_draw": 101},
    "adaptive_cadence": (["rescore", 7, 7, 3, 7, "rescore", 7, 3, 7, 7, "rescore", 7, 3], 7),
}


def fs_stub(widths=None, coef=False, res_targets=True):
    """Buffers one longer than the batch, all at the sentinel; ``run`` and ``rescore`` record into ``calls``."""
    full = lambda *shape: torch.full(shape, SENTINEL)
    fs = types.SimpleNamespace(X_val=full(N_IC + N_BC + 1, 3), X_res=full(B_RES + 1, 3), flat_grad=torch.zeros(4), calls=[])
    if widths is None:
        fs.target_val, fs.target_res = full(N_IC + N_BC + 1), full(B_RES + 1)
    else:
        fs.target_val, fs.target_res = full(widths[0], N_IC + N_BC + 1), (full(widths[1], B_RES + 1) if res_targets else None)
    if coef:
        fs.coef_res = full(COLS, B_RES + 1)
    fs.run = fs.calls.append
    fs.rescore = lambda: fs.calls.append("rescore")
    return fs


def stub_trainer(cls, fs, **attrs):
    """A trainer of class ``cls`` without its constructor: the attributes its batch and step methods read."""
    tr = object.__new__(cls)
    tr.__dict__.update(dict(dict(fs=fs, device=torch.device("cpu"), n_ic=N_IC, n_bc=N_BC, B_res=B_RES, _explicit=False,
                                 adaptive=None, world=1, rank=0, _comm=None, sampler="torch", _sampled=True), **attrs))
    return tr


def buffers(fs):
    """The step's batch buffers as nested lists of ints (every value written here is a whole number)."""
    out = {}
    for name in ("X_val", "X_res", "target_val", "target_res", "coef_res"):
        t = getattr(fs, name, None)
        if t is not None:
            out[name] = t.to(torch.int64).tolist()
    return out


def points(n, base):
    return base + torch.arange(3.0 * n).reshape(n, 3)


def rows(n, width, base):
    return base + torch.arange(float(n * width)).reshape(n, width)


def scalar_batch(n_ic=N_IC, n_bc=N_BC, B=B_RES):
    return (points(n_ic, 100), points(n_bc, 200), points(B, 300)), \
        (10 + torch.arange(float(n_ic)), 20 + torch.arange(float(n_bc)), 30 + torch.arange(float(B)))


def system_batch(with_r):
    X, _ = scalar_batch()
    return X, (rows(N_IC, K, 1000), rows(N_BC, K, 2000), rows(B_RES, N_EQ, 3000) if with_r else None)


def inverse_trainer(**attrs):
    return stub_trainer(pkg("trainer.inverse_train").InverseTrainer, fs_stub(), **attrs)


def system_trainer(with_r=True, **attrs):
    attrs.setdefault("dataset", types.SimpleNamespace(n_eq=N_EQ))
    return stub_trainer(pkg("trainer.system_train").SystemTrainer, fs_stub((K, N_EQ), res_targets=with_r), K=K, has_r=with_r,
                        **attrs)


def fused_trainer(rank=0, world=2, coef=True, **attrs):
    """Rank ``rank`` of ``world`` over the GLOBAL batch (3, 5, 9): odd counts, rank 0 takes (2, 3, 5), rank 1 (1, 2, 4)."""
    dt = pkg("trainer.diffusion_train")
    n_ic, n_bc, B = (dt.shard_count(n, world, rank) for n in (3, 5, 9))
    return stub_trainer(dt.FusedTrainer, fs_stub(coef=coef), **dict(dict(world=world, rank=rank, n_ic=n_ic, n_bc=n_bc, B_res=B,
                                                                         tabulated=True, coef_mode=coef), **attrs))


TRAINERS = [inverse_trainer, system_trainer, lambda **attrs: fused_trainer(world=1, **attrs)]


# ------------------------------------------------------------------------------------------------- load_batches
def load_inverse():
    tr = inverse_trainer()
    X, y = scalar_batch()
    tr.load_batches(*X, y)
    assert tr._explicit
    return buffers(tr.fs)


def load_system(with_r):
    tr = system_trainer(with_r)
    X, y = system_batch(with_r)
    tr.load_batches(*X, y)
    assert tr._explicit
    return buffers(tr.fs)


def load_fused(rank):
    tr = fused_trainer(rank)
    X, y = scalar_batch(3, 5, 9)
    tr.load_batches(*X, targets=y, coef=rows(9, COLS, 5000))
    assert tr._explicit
    return buffers(tr.fs)


def test_load_batches_scalar_layout():
    assert load_inverse() == EXPECTED["load_inverse"]


@pytest.mark.parametrize("with_r", [True, False])
def test_load_batches_batch_minor_layout(with_r):
    assert load_system(with_r) == EXPECTED[f"load_system_{with_r}"]


@pytest.mark.parametrize("rank", [0, 1])
def test_load_batches_takes_this_ranks_shard_with_targets_and_coefficient_rows(rank):
    assert load_fused(rank) == EXPECTED[f"load_fused_{rank}"]


def raises(text):
    return pytest.raises(ValueError, match=re.escape(text))


def test_load_batches_errors_of_the_inverse_trainer():
    X, y = scalar_batch()
    with raises("batches must hold (2, 3, 5) points"):
        inverse_trainer().load_batches(X[0], X[1], points(4, 0), y)
    for k, name in enumerate(("u_ic", "u_bc", "r_res")):
        bad = list(y)
        bad[k] = torch.zeros(7)
        with raises(f"{name} must hold {(N_IC, N_BC, B_RES)[k]} values: one per point"):
            inverse_trainer().load_batches(*X, tuple(bad))


def test_load_batches_errors_of_the_system_trainer():
    X, y = system_batch(True)
    with raises("batches must hold (2, 3, 5) points"):
        system_trainer().load_batches(points(3, 0), X[1], X[2], y)
    with raises("residual targets are given exactly when the dataset has them (R is None: zero targets)"):
        system_trainer(True).load_batches(*X, (y[0], y[1], None))
    with raises("residual targets are given exactly when the dataset has them (R is None: zero targets)"):
        system_trainer(False).load_batches(*X, y)
    with raises("U_ic must be (2, 2): one value per point and output"):
        system_trainer().load_batches(*X, (rows(N_IC, 3, 0), y[1], y[2]))
    with raises("U_bc must be (3, 2): one value per point and output"):
        system_trainer().load_batches(*X, (y[0], rows(2, K, 0), y[2]))
    with raises("R_res must be (5, 3): one value per point and equation"):
        system_trainer().load_batches(*X, (y[0], y[1], rows(B_RES, 2, 0)))


def test_load_batches_errors_of_the_fused_trainer():
    X, y = scalar_batch(3, 5, 9)
    coef = rows(9, COLS, 0)
    with raises("coef needs a coefficient step: a dataset with coef_res, or pde={'problem': 3, 'coef': True, ...}"):
        fused_trainer(coef=False).load_batches(*X, targets=y, coef=coef)
    with raises("a coefficient step needs coef=(B_res, 7) operator rows with its batches"):
        fused_trainer().load_batches(*X, targets=y)
    with raises("targets need a tabulated step: construct the trainer with dataset= or pde={'problem': 3, ...}"):
        fused_trainer(coef=False, tabulated=False).load_batches(*X, targets=y)
    with raises("a tabulated step needs targets=(u_ic, u_bc, r_res) with its batches"):
        fused_trainer(coef=False).load_batches(*X)
    with raises("targets=(u_ic, u_bc, r_res) must hold one value per point of (X_ic, X_bc, X_res)"):
        fused_trainer().load_batches(*X, targets=(y[0], y[1], torch.zeros(8)), coef=coef)
    with raises("coef must be (9, 7): one operator row per point of X_res"):
        fused_trainer().load_batches(*X, targets=y, coef=rows(8, COLS, 0))


# ------------------------------------------------------------------------------------------------- sample()
def dataset_stub(layout):
    """Segments of 7 residual, 4 initial and 5 boundary rows; ``layout``: "scalar", "rows" (batch-minor targets) or
    "coef" (scalar targets and a coefficient table)."""
    Xr, Xi, Xb = points(7, 300), points(4, 100), points(5, 200)
    if layout == "rows":
        seg = ((Xr, rows(7, N_EQ, 3000)), (Xi, rows(4, K, 1000)), (Xb, rows(5, K, 2000)))
    else:
        seg = ((Xr, 30 + torch.arange(7.0)), (Xi, 10 + torch.arange(4.0)), (Xb, 20 + torch.arange(5.0)))
    return types.SimpleNamespace(segments=lambda: seg, coef_res=rows(7, COLS, 5000) if layout == "coef" else None, n_eq=N_EQ)


def sample_with_torch(layout):
    if layout == "scalar":
        tr = inverse_trainer(dataset=dataset_stub(layout))
    elif layout == "rows":
        tr = system_trainer(dataset=dataset_stub(layout))
    else:
        tr = fused_trainer(world=1, dataset=dataset_stub(layout), n_ic=N_IC, n_bc=N_BC, B_res=B_RES)
    torch.manual_seed(0)
    tr.sample()
    assert tr._explicit
    after = int(torch.randint(0, 1000, (1,)))       # where the generator stands: one randint per non-empty segment
    return dict(buffers(tr.fs), next_draw=after)


@pytest.mark.parametrize("layout", ["scalar", "rows", "coef"])
def test_torch_sampler_fills_the_rows_the_parent_filled(layout):
    assert sample_with_torch(layout) == EXPECTED[f"sample_{layout}"]


def test_torch_sampler_draws_nothing_for_an_empty_batch():
    tr = inverse_trainer(dataset=dataset_stub("scalar"), n_ic=0)
    torch.manual_seed(0)
    tr.sample()
    torch.manual_seed(0)
    want_bc = torch.randint(0, 5, (N_BC,))
    assert tr.fs.X_val[:N_BC].tolist() == points(5, 200)[want_bc].tolist()        # BC rows first: no IC draw ahead of them


@pytest.mark.parametrize("make", TRAINERS[:2])
def test_device_sampler_only_arms_the_next_step(make):
    tr = make(sampler="device", _explicit=True)
    tr.sample()
    assert not tr._explicit and tr.fs.calls == [] and buffers(tr.fs)["X_val"][0] == [-1, -1, -1]


@pytest.mark.parametrize("make", TRAINERS[:2])
def test_sample_refuses_an_empty_segment_behind_a_non_empty_batch(make):
    with raises("the dataset has an empty segment behind a non-empty batch: use load_batches(...)"):
        make(_sampled=False, sampler="device").sample()


# ------------------------------------------------------------------------------------------------- step()
@pytest.mark.parametrize("make", TRAINERS)
def test_step_phases(make):
    tr = make(_explicit=True)
    tr.step()
    tr._explicit = False
    tr.step()
    assert tr.fs.calls == [GRADS | UPDATE, SAMPLE | GRADS | UPDATE] == [3, 7]


def test_step_of_two_ranks_without_a_communicator_all_reduces_between_the_phases(monkeypatch):
    import torch.distributed as dist
    tr = fused_trainer(world=2)
    monkeypatch.setattr(dist, "all_reduce", lambda t: tr.fs.calls.append(("all_reduce", t is tr.fs.flat_grad)))
    tr.step()
    tr._explicit = True
    tr.step()
    assert tr.fs.calls == [SAMPLE | GRADS, ("all_reduce", True), UPDATE, GRADS, ("all_reduce", True), UPDATE]
    tr = fused_trainer(world=2, _comm=object())         # a library communicator: one call, the all-reduce inside it
    tr.step()
    assert tr.fs.calls == [SAMPLE | GRADS | UPDATE]


def adaptive_cadence():
    tr = fused_trainer(world=1, adaptive=types.SimpleNamespace(every=3), _steps=0)
    for kind in "SSESSESSSE":           # seven sampled steps (0..6) with explicit ones between them
        tr._explicit = kind == "E"
        tr.step()
    return tr.fs.calls, tr._steps


def test_adaptive_rescoring_counts_sampled_steps_only():
    assert adaptive_cadence() == EXPECTED["adaptive_cadence"]


# ------------------------------------------------------------------------------------------------- readers
def opt_stub(step=9, hist_base=4, hist_cap=4):
    rec = {"loss": 1.0, "loss_res": 0.5, "loss_bc": 0.25, "loss_ic": 0.125, "lr": 0.005, "step": step, "hist_base": hist_base}
    return types.SimpleNamespace(read=lambda: rec, hist_cap=hist_cap, loss_history=lambda steps=None: ("history", steps))


@pytest.mark.parametrize("make", TRAINERS)
def test_losses_and_loss_history_are_the_optimiser_records(make):
    tr = make(opt=opt_stub())
    assert tr.losses() == ((1.0, 0.5, 0.25, 0.125), 0.005)
    assert tr.loss_history() == ("history", None) and tr.loss_history(3) == ("history", 3)


def own_history(which, steps, **opt):
    """First column of the rows an own-entry history reader returns: row i of the 8-row buffer starts with 10 i."""
    if which == "coefficient":
        tr = inverse_trainer(opt=opt_stub(**opt))
        tr.fs.coef_hist = rows(8, COLS, 0) * 10.0 / COLS
        out = tr.coefficient_history(steps)
    else:
        tr = stub_trainer(pkg("trainer.balanced_train").BalancedTrainer, fs_stub(), opt=opt_stub(**opt))
        tr.fs.weight_hist = rows(8, 3, 0) * 10.0 / 3
        out = tr.weight_history(steps)
    return [round(float(r[0])) for r in out]


@pytest.mark.parametrize("which", ["coefficient", "weight"])
def test_own_entry_histories_default_to_the_steps_taken_and_clamp_to_the_buffer(which):
    assert own_history(which, None) == [0, 10, 20, 30]                         # step - hist_base = 5, capacity 4
    assert own_history(which, None, hist_cap=8) == [0, 10, 20, 30, 40]         # 9 - 4 steps of THIS buffer
    assert own_history(which, None, step=3, hist_base=5, hist_cap=8) == []     # never negative
    assert own_history(which, 2) == [0, 10] and own_history(which, -3) == [] and own_history(which, 100) == [0, 10, 20, 30]
