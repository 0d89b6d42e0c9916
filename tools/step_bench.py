"""The harness of the step benchmarks tools/bench_*.py: the silent logger and the common model, the warm-up and the
window-by-window alternation between trainers, the min / median / windows report, and the common arguments.

The method: every trainer is warmed up in turn, then `repeats` times each trainer in turn runs one window of `steps` x
(``sample()``, ``step()``) that ends in a device synchronise; a trainer's number is the min over its windows, so that a
disturbance of the shared host hits all of them alike and the best window of each is compared.  A script keeps its trainer
builders, its ``config`` string and its own JSON fields."""
import argparse
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "qcpinn-convection-diffusion-qiskit_amd"


def pkg(sub):
    """A submodule of the package, from the checkout ``parse`` put on the path."""
    return importlib.import_module(PKG + "." + sub)


class Log:
    def print(self, *a):
        pass

    def get_output_dir(self):
        return "/tmp"


def model(dev, **overrides):
    """The DVPDESolver every step benchmark times (cascade, 4 qubits, one layer, H = 50, one output), seeded."""
    args = {"batch_size": 64, "epochs": 0, "lr": 0.005, "seed": 1, "print_every": 10 ** 9, "num_qubits": 4,
            "num_quantum_layers": 1, "classic_network": [3, 50, 1], "q_ansatz": "cascade", "shots": 1024,
            "problem": "diffusion", "solver": "DV", "encoding": "None", "use_ibm_hardware": False}
    args.update(overrides)
    torch.manual_seed(1)
    return pkg("nn.DVPDESolver").DVPDESolver(args, Log(), device=dev)


def dataset(rows, coef=False):
    """The analytic problem's own targets, tabulated (``rows`` residual rows, a third per value segment), so that every
    step trains towards the same functions; ``coef``: with its operator as one table row per residual point."""
    data, tab = pkg("data.diffusion_dataset"), pkg("data.tabulated")
    rows_of = (lambda X: tab.coef_table(X, c_t=1.0, c_x=1.0, c_y=1.0, d_xx=0.01, d_yy=0.01)) if coef else None
    return tab.TabulatedProblem.from_functions(data.u, data.u, data.r, rows, rows // 3, rows // 3,
                                               generator=torch.Generator().manual_seed(0), coef=rows_of)


def warm_up_and_alternate(trs, steps, warmup, repeats, n_steps=None, clock=time.perf_counter, sync=None):
    """Seconds per step of every window, {name: [repeats values]}, of the trainers ``trs`` = {name: object with
    ``sample()`` and ``step()``}.  ``n_steps`` = {name: steps per window} overrides ``steps`` (and bounds the warm-up)
    per trainer; ``clock`` and ``sync`` (default ``torch.cuda.synchronize``) can be replaced to run without a GPU."""
    sync = torch.cuda.synchronize if sync is None else sync

    def run(tr, n):
        for _ in range(n):
            tr.sample()
            tr.step()
    for k, tr in trs.items():
        run(tr, warmup if n_steps is None else min(warmup, n_steps[k]))
    sync()
    windows = {k: [] for k in trs}
    for _ in range(repeats):
        for k, tr in trs.items():
            n = steps if n_steps is None else n_steps[k]
            t0 = clock()
            run(tr, n)
            sync()
            windows[k].append((clock() - t0) / n)
    return windows


def report(config, windows, **fields):
    """The JSON object of one shape: ``config``, the script's ``fields``, then per trainer the min, the median (by index)
    and all windows in ms per step."""
    return {"config": config, **fields,
            "ms_per_step": {k: min(w) * 1e3 for k, w in windows.items()},
            "ms_per_step_median": {k: sorted(w)[len(w) // 2] * 1e3 for k, w in windows.items()},
            "ms_per_step_windows": {k: [round(x * 1e3, 5) for x in w] for k, w in windows.items()}}


def losses(trs):
    """The last step's loss of every trainer (a host read each)."""
    return {k: tr.opt.read()["loss"] for k, tr in trs.items()}


def arguments(rows=1 << 20, modes=None):
    """The parser with --steps, --warmup, --repeats; with ``rows``, --rows; with ``modes``, --modes, --root and --label
    (an A/B run against another checkout: ``--root ../parent --modes <what the parent has> --label parent``)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    if rows:
        ap.add_argument("--rows", type=int, default=rows, help="residual rows of the resident dataset (a third per value segment)")
    if modes:
        ap.add_argument("--modes", default=",".join(modes))
        ap.add_argument("--root", default=ROOT, help="checkout to import the package (and its built library) from")
        ap.add_argument("--label", default="")
    return ap


def parse(ap):
    """The parsed arguments, with the checkout to import the package from (``--root``, default: this one) on the path."""
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(getattr(a, "root", ROOT)))
    return a
