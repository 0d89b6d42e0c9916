"""Times one fused training step of a DVPDESolver behind a Fourier-feature input map (args["fourier_features"] = m: the
pre stages k_pre_ff_fwd_both / k_pre_ff_bwd_both, W1[H][2m]) beside the plain step (W1[H][3]) at the same shapes: cascade,
4 qubits, H = 50, B residual + B // 3 initial + B // 3 boundary points at B = 64 and B = 65 536 (BASELINE config 2), on-device
coordinate draw.  The loops alternate window by window in one process on one device; each number is the min of `repeats`
windows of `steps` steps after `warmup` steps, the method of tools/bench_tabulated.py.  Prints one JSON object per batch
size."""
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


def _model(dev, m, scale):
    Solver = importlib.import_module(PKG + ".nn.DVPDESolver").DVPDESolver
    args = {"batch_size": 64, "epochs": 0, "lr": 0.005, "seed": 1, "print_every": 10 ** 9, "num_qubits": 4,
            "num_quantum_layers": 1, "classic_network": [3, 50, 1], "q_ansatz": "cascade", "shots": 1024,
            "problem": "diffusion", "solver": "DV", "encoding": "None", "use_ibm_hardware": False}
    if m:
        args.update(fourier_features=m, fourier_scale=scale)
    torch.manual_seed(1)
    return Solver(args, _Log(), device=dev)


def run(B, ms_list, scale, steps, warmup, repeats):
    trainer = importlib.import_module(PKG + ".trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    trs = {("plain" if m == 0 else f"m{m}"): trainer.FusedTrainer(_model(dev, m, scale), B, capacity=0) for m in ms_list}
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
    out = {"config": "fourier_vs_plain", "n_qubits": 4, "H": 50, "B_res": B, "B_ic": B // 3, "B_bc": B // 3, "fourier_scale": scale,
           "NP": {k: int(tr.eng.NP) for k, tr in trs.items()}, "ms_per_step": ms,
           "difference_ms": {k: v - ms["plain"] for k, v in ms.items() if k != "plain"} if "plain" in ms else {},
           "ms_per_step_median": {k: sorted(w)[len(w) // 2] * 1e3 for k, w in windows.items()},
           "loss": {k: tr.opt.read()["loss"] for k, tr in trs.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--features", default="0,8,32", help="mapping sizes m to time; 0 is the plain step")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for b in a.batches.split(","):
        run(int(b), [int(m) for m in a.features.split(",")], a.scale, a.steps, a.warmup, a.repeats)
