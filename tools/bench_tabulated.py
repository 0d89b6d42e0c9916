"""Times one fused training step on tabulated targets (FusedTrainer(..., dataset=): device gather from a resident
dataset + qc_fused_pinn_data_step) beside the analytic problem-0 step (on-device coordinate draw +
qc_fused_pinn_residual_step) at the same shapes: cascade, 4 qubits, H = 50, B residual + B // 3 initial + B // 3 boundary
points at B = 64 and B = 65 536 (BASELINE config 2).  The two steps alternate window by window on one device; each number
is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of tools/bench_hybrid_pinn.py.  Prints
one JSON object per batch size."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "qcpinn-convection-diffusion-qiskit_amd"


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


def run(B, rows, steps, warmup, repeats):
    trainer = importlib.import_module(PKG + ".trainer.diffusion_train")
    data = importlib.import_module(PKG + ".data.diffusion_dataset")
    TP = importlib.import_module(PKG + ".data.tabulated").TabulatedProblem
    dev = torch.device("cuda", 0)
    # the analytic problem's own targets, tabulated: both steps train towards the same functions
    ds = TP.from_functions(data.u, data.u, data.r, rows, rows // 3, rows // 3, generator=torch.Generator().manual_seed(0))
    trs = {"analytic": trainer.FusedTrainer(_model(dev), B, capacity=0),
           "tabulated": trainer.FusedTrainer(_model(dev), B, capacity=0, dataset=ds)}
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
    ms = {k: min(w) * 1e3 for k, w in windows.items()}
    out = {"config": "tabulated_vs_analytic", "n_qubits": 4, "B_res": B, "B_ic": B // 3, "B_bc": B // 3,
           "dataset_rows": [rows, rows // 3, rows // 3], "ms_per_step_analytic": ms["analytic"],
           "ms_per_step_tabulated": ms["tabulated"], "difference_ms": ms["tabulated"] - ms["analytic"],
           "ms_per_step_median": {k: sorted(w)[len(w) // 2] * 1e3 for k, w in windows.items()},
           "loss": {k: tr.opt.read()["loss"] for k, tr in trs.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--rows", type=int, default=1 << 20, help="residual rows of the resident dataset (a third per value segment)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats)
