"""Times one fused training step under gradient-norm loss weights (GradNormTrainer: qc_fused_pinn_gradnorm_step, the class
fold and the combination launch ahead of the optimiser) beside the tabulated step (qc_fused_pinn_data_step) at the same
shapes: cascade, 4 qubits, H = 50.  Shapes are ``B:n_val`` pairs: B residual points and n_val initial and n_val boundary
points, n_val a multiple of 64; the defaults are 128 + 64 + 64 points and 65 536 + 2 x 21 888 points (BASELINE config 2
with the value batches on a tile boundary, 21 888 = 342 x 64).  The two steps alternate window by window on one device;
each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of tools/bench_causal.py.
Prints one JSON object per shape.

``--root DIR`` imports the package from another checkout of this repository (built there), and ``--modes`` selects the
steps, as in tools/bench_causal.py.

``--convergence N``: instead of timing, N steps of the tabulated step (fixed weights 2, 4, 2) and of the gradient-norm step
on the same seed at the first shape; prints the loss parts and the weights every N / 20 steps.  An illustration of what
the weights do, not a comparison of the two rules."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

PKG = "qcpinn-convection-diffusion-qiskit_amd"
MODES = ("tabulated", "gradnorm")


class _Log:
    def print(self, *a):
        pass

    def get_output_dir(self):
        return "/tmp"


def _model(dev):
    Solver = importlib.import_module(PKG + ".nn.DVPDESolver").DVPDESolver
    args = {"batch_size": 64, "epochs": 0, "lr": 0.005, "seed": 1, "print_every": 10 ** 9, "num_qubits": 4,
            "num_quantum_layers": 1, "classic_network": [3, 50, 1], "q_ansatz": "cascade", "shots": 1024,
            "problem": "diffusion", "solver": "DV", "encoding": "None", "use_ibm_hardware": False}
    torch.manual_seed(1)
    return Solver(args, _Log(), device=dev)


def _trainers(B, n_val, rows, modes, alpha, every, capacity=0):
    trainer = importlib.import_module(PKG + ".trainer.diffusion_train")
    data = importlib.import_module(PKG + ".data.diffusion_dataset")
    tab = importlib.import_module(PKG + ".data.tabulated")
    dev = torch.device("cuda", 0)
    # the analytic problem's own targets and operator, tabulated: both steps train towards the same functions
    gen = lambda: torch.Generator().manual_seed(0)
    dataset = lambda: tab.TabulatedProblem.from_functions(data.u, data.u, data.r, rows, rows // 3, rows // 3, generator=gen())
    trs = {}
    if "tabulated" in modes:
        torch.manual_seed(7)
        trs["tabulated"] = trainer.FusedTrainer(_model(dev), B, capacity=capacity, dataset=dataset(), n_ic=n_val, n_bc=n_val)
    if "gradnorm" in modes:
        gt = importlib.import_module(PKG + ".trainer.gradnorm_train")
        lb = importlib.import_module(PKG + ".nn.loss_balance")
        torch.manual_seed(7)
        trs["gradnorm"] = gt.GradNormTrainer(_model(dev), B, lb.GradNormWeighting(alpha=alpha, every=every), dataset(),
                                             capacity=capacity, n_ic=n_val, n_bc=n_val)
    return trs


def run(B, n_val, rows, steps, warmup, repeats, modes, label, alpha, every):
    trs = _trainers(B, n_val, rows, modes, alpha, every)
    for tr in trs.values():
        for _ in range(warmup):
            tr.sample()
            tr.step()
    torch.cuda.synchronize()
    windows = {k: [] for k in trs}
    for _ in range(repeats):
        for k, tr in trs.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.sample()
                tr.step()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / steps)
    out = {"config": "gradnorm_vs_tabulated", "label": label, "n_qubits": 4, "B_res": B, "B_ic": n_val, "B_bc": n_val,
           "dataset_rows": [rows, rows // 3, rows // 3],
           "ms_per_step": {k: min(w) * 1e3 for k, w in windows.items()},
           "ms_per_step_median": {k: sorted(w)[len(w) // 2] * 1e3 for k, w in windows.items()},
           "ms_per_step_windows": {k: [round(x * 1e3, 5) for x in w] for k, w in windows.items()},
           "loss": {k: tr.opt.read()["loss"] for k, tr in trs.items()}}
    if "gradnorm" in trs:
        out["gradnorm"] = dict(zip(("lam_bc", "lam_ic"), trs["gradnorm"].weights()), **trs["gradnorm"].gradient_stats())
    print(json.dumps(out), flush=True)


def convergence(B, n_val, rows, steps, alpha, every):
    trs = _trainers(B, n_val, rows, MODES, alpha, every, capacity=steps)
    mark = max(steps // 20, 1)
    print(f"# {B} + {n_val} + {n_val} points, {steps} steps, alpha {alpha}, every {every}; columns: step | fixed weights: "
          f"L_r L_bc L_ic | gradient-norm weights: L_r L_bc L_ic lam_bc lam_ic", flush=True)
    for it in range(steps):
        for tr in trs.values():
            tr.sample()
            tr.step()
        if it % mark == 0 or it == steps - 1:
            (_, *a), _ = trs["tabulated"].losses()
            (_, *b), _ = trs["gradnorm"].losses()
            lam = trs["gradnorm"].weights()
            print(f"{it:6d} | " + " ".join(f"{v:.4e}" for v in a) + " | " + " ".join(f"{v:.4e}" for v in b)
                  + f" {lam[0]:.3e} {lam[1]:.3e}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128:64,65536:21888", help="B:n_val pairs")
    ap.add_argument("--rows", type=int, default=1 << 20, help="residual rows of the resident dataset (a third per value segment)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--convergence", type=int, default=0, metavar="N", help="print loss parts and weights over N steps instead")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import the package (and its built library) from")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    if a.convergence:
        convergence(*shapes[0], a.rows, a.convergence, a.alpha, a.every)
    else:
        for B, n_val in shapes:
            run(B, n_val, a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label, a.alpha, a.every)
