"""The one training loop of trainer/diffusion_train.py (run_fused_loop) on a stub trainer and a stub model: no GPU and
no library call.  EXPECTED holds the lines that ``_train_fused`` of the commit before the loops were merged printed for
the same stubs (its FusedTrainer replaced by StubTrainer), with the timing fields masked; the loop must print the same
lines in the same order, save at iterations 2 and 4 and leave the same loss history, on sampled and on explicit batches,
and the variants' extra line and closing hook must land where their own loops had them."""
import re

import pytest

from conftest import pkg

EPOCHS, PRINT_EVERY = 5, 2
EXPECTED = [
    "Starting training for 5 epochs...",
    "Batch size: 64",
    "Epoch: 0/5 [0.0%] | Loss: 1.00e+00 | Loss_res: 5.00e-01 | Loss_bcs: 2.50e-01 | loss_ics: 1.25e-01 | lr: 5.00e-03 | "
    "Epoch_time: #s | Total: #s | ETA: #s",
    "Epoch: 2/5 [40.0%] | Loss: 3.33e-01 | Loss_res: 1.67e-01 | Loss_bcs: 8.33e-02 | loss_ics: 4.17e-02 | lr: 5.00e-03 | "
    "Epoch_time: #s | Total: #s | ETA: #s",
    "Epoch: 4/5 [80.0%] | Loss: 2.00e-01 | Loss_res: 1.00e-01 | Loss_bcs: 5.00e-02 | loss_ics: 2.50e-02 | lr: 5.00e-03 | "
    "Epoch_time: #s | Total: #s | ETA: #s",
    "Training completed in # seconds (# minutes)",
]
EXPECTED_HISTORY = [1.0 / (k + 1) for k in range(EPOCHS + 1)]


def mask(line):
    line = re.sub(r"(Epoch_time|Total|ETA): [0-9.]+s", r"\1: #s", line)
    return re.sub(r"completed in [0-9.]+ seconds \([0-9.]+ minutes\)", "completed in # seconds (# minutes)", line)


class StubTrainer:
    """What the loop needs of a trainer; step k (0-based) has the loss 1 / (k + 1).  ``opt`` is the stub itself, so the
    history is reachable as ``tr.opt.loss_history`` too."""

    def __init__(self):
        self.calls, self.n, self.opt = [], 0, self

    def sample(self):
        self.calls.append("sample")

    def load_batches(self, *X, targets=None, coef=None):
        self.calls.append(("load", X, targets, coef))

    def step(self):
        self.calls.append("step")
        self.n += 1

    def losses(self):
        f = 1.0 / self.n
        return (f, f / 2, f / 4, f / 8), 0.005

    def loss_history(self, steps=None):
        return [1.0 / (k + 1) for k in range(self.n if steps is None else min(steps, self.n))]

    def sync_to_torch(self):
        self.calls.append("sync")


class StubLogger:
    def __init__(self):
        self.lines = []

    def print(self, *a):
        self.lines.append(" ".join(str(x) for x in a))


class StubModel:
    def __init__(self):
        self.logger, self.args, self.epochs = StubLogger(), {"print_every": PRINT_EVERY}, EPOCHS
        self.loss_history, self.total_training_time, self.saved_at = [], 0.0, []

    def save_state(self):
        self.saved_at.append(len(self.loss_history) - 1)      # the iteration whose history was just stored


@pytest.mark.parametrize("explicit", [False, True])
def test_loop_prints_saves_and_records_what_the_fused_loop_did(explicit):
    dt = pkg("trainer.diffusion_train")
    model, tr = StubModel(), StubTrainer()
    batches = [(("ic", k), ("bc", k), ("res", k), ("targets", k)) for k in range(EPOCHS + 1)] if explicit else None
    out = dt.run_fused_loop(model, tr, f"Starting training for {model.epochs} epochs...", 64, batches)
    assert out is tr
    assert [mask(l) for l in model.logger.lines] == EXPECTED
    assert model.saved_at == [2, 4]
    assert model.loss_history == EXPECTED_HISTORY
    assert model.total_training_time > 0.0
    feed = [("load", b[:3], b[3], None) for b in batches] if explicit else ["sample"] * (EPOCHS + 1)
    assert tr.calls == [c for f in feed for c in (f, "step")] + ["sync"]


def test_extra_line_follows_each_log_line_and_finish_runs_ahead_of_the_copy_back():
    dt = pkg("trainer.diffusion_train")
    model, tr = StubModel(), StubTrainer()

    def finish(tr, steps):
        model.finished = (steps, list(model.loss_history), "sync" in tr.calls)
        model.logger.print("closing hook")
    dt.run_fused_loop(model, tr, "banner", 64, extra_line=lambda tr: f"  extra after step {tr.n}", finish=finish)
    lines = [mask(l) for l in model.logger.lines]
    assert lines[0] == "banner"
    assert lines[2:8] == [EXPECTED[2], "  extra after step 1", EXPECTED[3], "  extra after step 3", EXPECTED[4],
                          "  extra after step 5"]
    assert lines[8:] == ["closing hook", EXPECTED[5]]
    assert model.finished == (EPOCHS + 1, EXPECTED_HISTORY, False)
    assert model.saved_at == [2, 4] and model.loss_history == EXPECTED_HISTORY


def test_loaders_hand_over_what_the_variants_loops_did():
    dt = pkg("trainer.diffusion_train")
    tr = StubTrainer()
    dt.load_explicit(tr, ("i", "b", "r"))
    dt.load_explicit(tr, ("i", "b", "r", "t", "c"))
    dt.load_with_targets(tr, ("i", "b", "r", "t"))
    assert tr.calls == [("load", ("i", "b", "r"), None, None), ("load", ("i", "b", "r"), "t", "c"),
                        ("load", ("i", "b", "r"), "t", None)]
