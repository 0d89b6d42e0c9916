"""Times one fused training step of a re-uploaded DVPDESolver (args["reupload"]: an EMBED layer in front of every ansatz
layer after the first, the kernels of csrc/qc_circuit_reup*.h*) beside the plain model of the same depth: cascade, 4 qubits,
H = 50, L = 2 and 3 layers, B residual + B // 3 initial + B // 3 boundary points at B = 64 and B = 65 536, on-device
coordinate draw.  The plain model is the yardstick of the same process: it runs compile-time programs where one is
generated and the merged one-launch-per-stage form, the re-uploaded model the run-time interpreter in the two-stream form
(QC_NO_STATIC=1 QC_NO_MERGE=1 puts the plain model on the same footing).  The loops alternate window by window on one
device; each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of
tools/bench_tabulated.py.  Prints one JSON object per batch size and depth."""
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


def _model(dev, L, reupload):
    Solver = importlib.import_module(PKG + ".nn.DVPDESolver").DVPDESolver
    args = {"batch_size": 64, "epochs": 0, "lr": 0.005, "seed": 1, "print_every": 10 ** 9, "num_qubits": 4,
            "num_quantum_layers": L, "classic_network": [3, 50, 1], "q_ansatz": "cascade", "shots": 1024,
            "problem": "diffusion", "solver": "DV", "encoding": "None", "use_ibm_hardware": False, "reupload": reupload}
    torch.manual_seed(1)
    return Solver(args, _Log(), device=dev)


def run(B, L, steps, warmup, repeats):
    trainer = importlib.import_module(PKG + ".trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    trs = {k: trainer.FusedTrainer(_model(dev, L, k == "reupload"), B, capacity=0) for k in ("plain", "reupload")}
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
    out = {"config": "reupload_vs_plain", "q_ansatz": "cascade", "n_qubits": 4, "n_layers": L, "H": 50, "B_res": B, "B_ic": B // 3,
           "B_bc": B // 3, "n_gates": {k: int(tr.model.quantum_layer.program.n_gates) for k, tr in trs.items()},
           "ms_per_step": ms, "difference_ms": ms["reupload"] - ms["plain"],
           "ms_per_step_median": {k: sorted(w)[len(w) // 2] * 1e3 for k, w in windows.items()},
           "switches": {k: os.environ.get(k, "") for k in ("QC_NO_STATIC", "QC_NO_MERGE")},
           "loss": {k: tr.opt.read()["loss"] for k, tr in trs.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--layers", default="2,3")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for b in a.batches.split(","):
        for L in a.layers.split(","):
            run(int(b), int(L), a.steps, a.warmup, a.repeats)
