"""Times one fused training step under causal weights (CausalTrainer: the slab-stratified gather +
qc_fused_pinn_causal_step, the slab weights formed on the device) beside the tabulated step (qc_fused_pinn_data_step) at
the same shapes: cascade, 4 qubits, H = 50.  Shapes are ``B:M:n_val`` triples: B residual points in M time slabs and n_val
initial and n_val boundary points; the defaults are the smallest causal shape, 128 + 21 + 21 points in 2 slabs (a causal
batch holds whole 64-point tiles of every slab, so 64 residual points cannot be split), and 65 536 + 2 x 21 845 points in
16 slabs (BASELINE config 2).  The two steps alternate window by window on one device; each number is the min of
`repeats` windows of `steps` steps after `warmup` steps, the method of tools/bench_balanced.py.  Prints one JSON object per
shape.

``--root DIR`` imports the package from another checkout of this repository (built there), and ``--modes`` selects the
steps: an A/B run of a parent commit that has no causal step is

    python tools/bench_causal.py --root ../parent --modes tabulated --label parent
    python tools/bench_causal.py --label change

alternated in one call (profiles/causal_step_bench_runs.txt)."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

PKG = "qcpinn-convection-diffusion-qiskit_amd"
MODES = ("tabulated", "causal")


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


def run(B, M, n_val, rows, steps, warmup, repeats, modes, label, eps):
    trainer = importlib.import_module(PKG + ".trainer.diffusion_train")
    data = importlib.import_module(PKG + ".data.diffusion_dataset")
    tab = importlib.import_module(PKG + ".data.tabulated")
    dev = torch.device("cuda", 0)
    # the analytic problem's own targets and operator, tabulated: both steps train towards the same functions
    gen = lambda: torch.Generator().manual_seed(0)
    dataset = lambda: tab.TabulatedProblem.from_functions(data.u, data.u, data.r, rows, rows // 3, rows // 3, generator=gen())
    trs = {}
    if "tabulated" in modes:
        trs["tabulated"] = trainer.FusedTrainer(_model(dev), B, capacity=0, dataset=dataset(), n_ic=n_val, n_bc=n_val)
    if "causal" in modes:
        causal = importlib.import_module(PKG + ".trainer.causal_train")
        trs["causal"] = causal.CausalTrainer(_model(dev), B, dataset(), tab.CausalWeighting(M, eps=eps), capacity=0, n_ic=n_val,
                                             n_bc=n_val)
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
    out = {"config": "causal_vs_tabulated", "label": label, "n_qubits": 4, "B_res": B, "n_slabs": M, "B_ic": n_val, "B_bc": n_val,
           "dataset_rows": [rows, rows // 3, rows // 3],
           "ms_per_step": {k: min(w) * 1e3 for k, w in windows.items()},
           "ms_per_step_median": {k: sorted(w)[len(w) // 2] * 1e3 for k, w in windows.items()},
           "ms_per_step_windows": {k: [round(x * 1e3, 5) for x in w] for k, w in windows.items()},
           "loss": {k: tr.opt.read()["loss"] for k, tr in trs.items()}}
    if "causal" in trs:
        eps_now, raised = trs["causal"].epsilon()
        out["causal"] = {"eps": eps_now, "n_raised": raised, "W_min": float(trs["causal"].causal_weights().min())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128:2:21,65536:16:21845", help="B:M:n_val triples")
    ap.add_argument("--rows", type=int, default=1 << 20, help="residual rows of the resident dataset (a third per value segment)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import the package (and its built library) from")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    for shape in a.shapes.split(","):
        B, M, n_val = (int(v) for v in shape.split(":"))
        run(B, M, n_val, a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label, a.eps)
