"""Times the fused training step with residual-adaptive sampling (FusedTrainer(..., dataset=, adaptive=): the gather
draws its residual rows from the CDF of qc_adapt_build, qc_fused_pinn_adaptive_step) beside the tabulated and the
coefficient step of the same build at the same shapes: cascade, 4 qubits, H = 50, B residual + B // 3 initial + B // 3
boundary points at B = 64 and B = 65 536, a resident dataset of 2^20 + 2 x 349 525 rows.  The steps alternate window by
window on one device; each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of
tools/bench_coef.py.  Prints one JSON object per batch size:

  ms_per_step            tabulated, coef, adaptive (scalar operator) and adaptive_coef (coefficient table), the adaptive
                         ones with rescoring OFF (every = 10^9, one rescoring in the warm-up): what the search costs
                         over the uniform gather
  rescore_ms             one rescoring of the whole residual segment (qc_dataset_scores + qc_adapt_build), min of
                         `repeats` timings of 5 back-to-back calls, and its cost per step at every = 100

profiles/adaptive_ab_bench_runs.txt holds the recorded runs, among them the comparison of the LDS-staged coarse search
(kept) with the search from global memory alone."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

PKG = "qcpinn-convection-diffusion-qiskit_amd"
MODES = ("tabulated", "coef", "adaptive", "adaptive_coef")


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


def run(B, rows, steps, warmup, repeats, modes, label):
    trainer = importlib.import_module(PKG + ".trainer.diffusion_train")
    data = importlib.import_module(PKG + ".data.diffusion_dataset")
    tab = importlib.import_module(PKG + ".data.tabulated")
    dev = torch.device("cuda", 0)
    gen = lambda: torch.Generator().manual_seed(0)
    rows_of = lambda X: tab.coef_table(X, c_t=1.0, c_x=1.0, c_y=1.0, d_xx=0.01, d_yy=0.01)
    make = lambda coef: tab.TabulatedProblem.from_functions(data.u, data.u, data.r, rows, rows // 3, rows // 3, generator=gen(),
                                                            coef=rows_of if coef else None)
    never = tab.AdaptiveSampling(power=1, floor=1.0, every=10 ** 9)          # one rescoring, on the first step
    trs = {}
    for k in modes:
        trs[k] = trainer.FusedTrainer(_model(dev), B, capacity=0, dataset=make(k.endswith("coef")),
                                      adaptive=never if k.startswith("adaptive") else None)
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
    rescore = {}
    for k, tr in trs.items():
        if not k.startswith("adaptive"):
            continue
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                tr.fs.rescore()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / 5)
        rescore[k] = min(ts) * 1e3
    out = {"config": "adaptive_vs_coef_vs_tabulated", "label": label, "n_qubits": 4, "B_res": B, "B_ic": B // 3, "B_bc": B // 3,
           "dataset_rows": [rows, rows // 3, rows // 3],
           "ms_per_step": {k: min(w) * 1e3 for k, w in windows.items()},
           "ms_per_step_median": {k: sorted(w)[len(w) // 2] * 1e3 for k, w in windows.items()},
           "rescore_ms": rescore, "rescore_ms_per_step_at_every_100": {k: v / 100 for k, v in rescore.items()},
           "mean_score": {k: float(tr.dataset_scores().mean()) for k, tr in trs.items() if k.startswith("adaptive")},
           "loss": {k: tr.opt.read()["loss"] for k, tr in trs.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--rows", type=int, default=1 << 20, help="residual rows of the resident dataset (a third per value segment)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import the package (and its built library) from")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label)
