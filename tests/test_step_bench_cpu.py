"""The harness of the step benchmarks (tools/step_bench.py) on two recording stub trainers, a fake clock and a recording
synchronise: no GPU.  The order of the calls, the windows and the report are the ones every tools/bench_*.py wrote out
for itself before the harness was shared."""
import importlib.util
import json
import os
import sys

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("step_bench", os.path.join(ROOT, "tools", "step_bench.py"))
step_bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(step_bench)


class Recorder:
    """Two stub trainers, the clock and the synchronise, all writing into one list of events.  The clock advances by
    1 second per ``step()`` of trainer "A" and by 3 seconds per ``step()`` of trainer "B", and by 0.5 in a synchronise."""

    COST = {"A": 1.0, "B": 3.0}

    def __init__(self):
        self.events, self.now = [], 0.0
        self.trs = {k: self.Trainer(self, k) for k in ("A", "B")}

    class Trainer:
        def __init__(self, rec, name):
            self.rec, self.name = rec, name

        def sample(self):
            self.rec.events.append(self.name + ".sample")

        def step(self):
            self.rec.events.append(self.name + ".step")
            self.rec.now += self.rec.COST[self.name]

    def clock(self):
        return self.now

    def sync(self):
        self.events.append("sync")
        self.now += 0.5


def window(name, n):
    return [name + ".sample", name + ".step"] * n + ["sync"]


def test_warm_up_then_alternate_window_by_window():
    rec = Recorder()
    windows = step_bench.warm_up_and_alternate(rec.trs, steps=3, warmup=2, repeats=2, clock=rec.clock, sync=rec.sync)
    warm = ["A.sample", "A.step"] * 2 + ["B.sample", "B.step"] * 2 + ["sync"]
    assert rec.events == warm + (window("A", 3) + window("B", 3)) * 2
    # elapsed / steps, the closing synchronise inside the window: (3 x 1 + 0.5) / 3 and (3 x 3 + 0.5) / 3
    assert windows == {"A": [3.5 / 3] * 2, "B": [9.5 / 3] * 2}


def test_steps_per_window_of_one_trainer():
    rec = Recorder()
    windows = step_bench.warm_up_and_alternate(rec.trs, steps=4, warmup=3, repeats=1, n_steps={"A": 4, "B": 2},
                                               clock=rec.clock, sync=rec.sync)
    # the warm-up never exceeds a trainer's own window
    assert rec.events == ["A.sample", "A.step"] * 3 + ["B.sample", "B.step"] * 2 + ["sync"] + window("A", 4) + window("B", 2)
    assert windows == {"A": [4.5 / 4], "B": [6.5 / 2]}


def test_report_keys_order_and_figures():
    windows = {"A": [0.0030004, 0.001, 0.0020006], "B": [0.004, 0.0050000049]}
    out = step_bench.report("a_vs_b", windows, label="change", B_res=64, dataset_rows=[4096, 1365, 1365])
    assert list(out) == ["config", "label", "B_res", "dataset_rows", "ms_per_step", "ms_per_step_median", "ms_per_step_windows"]
    assert (out["config"], out["label"], out["B_res"], out["dataset_rows"]) == ("a_vs_b", "change", 64, [4096, 1365, 1365])
    assert out["ms_per_step"] == {"A": 1.0, "B": 4.0}                                  # the min
    assert out["ms_per_step_median"] == {"A": 0.0020006 * 1e3, "B": 0.0050000049 * 1e3}        # sorted(w)[len(w) // 2]
    assert out["ms_per_step_windows"] == {"A": [3.0004, 1.0, 2.0006], "B": [4.0, 5.0]}         # 5 places, in run order
    assert json.loads(json.dumps(out)) == out


def test_common_arguments(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench_x.py", "--steps", "3"])
    monkeypatch.setattr(sys, "path", list(sys.path))
    a = step_bench.parse(step_bench.arguments(modes=("x", "y")))
    assert (a.steps, a.warmup, a.repeats, a.rows, a.modes, a.label) == (3, 50, 5, 1 << 20, "x,y", "")
    assert a.root == ROOT == sys.path[0]
    monkeypatch.setattr(sys, "argv", ["bench_x.py"])
    a = step_bench.parse(step_bench.arguments(rows=None))
    assert sorted(vars(a)) == ["repeats", "steps", "warmup"] and sys.path[0] == ROOT
