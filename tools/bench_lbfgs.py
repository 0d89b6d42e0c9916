"""Times one L-BFGS evaluation on the device (LbfgsTrainer: the GRADS phase of the fused step + qc_lbfgs_step, history m = 10
and m = 32) beside the Adam step of the same FusedTrainer, and compares loss against evaluation count for Adam alone and
Adam -> L-BFGS.

Time: cascade, 4 qubits, H = 50, one resident batch of B residual + B // 3 initial + B // 3 boundary points at B = 64 and
B = 65 536 (BASELINE config 2).  Four loops alternate window by window in one process: ``adam`` (one call, the fold inside
the optimiser kernel), ``adam_two_call`` (QC_PHASE_GRADS, then QC_PHASE_UPDATE: the separate row-reduction launch the
L-BFGS evaluation also pays), ``lbfgs_m10`` and ``lbfgs_m32``.  Each number is the min of ``repeats`` windows of ``steps``
evaluations after ``warmup``; adam_two_call - adam is the cost of the two-call form, lbfgs - adam_two_call that of the kernel
against k_adam_fast.

Convergence (``--convergence``): the same model on ONE fixed batch gathered from a TabulatedProblem of the analytic
problem's targets: ``--adam`` Adam steps, then ``--evals`` more Adam steps against ``--evals`` L-BFGS evaluations; the loss
every ``--every`` evaluations.  Prints one JSON object per line (profiles/lbfgs_step_bench_runs.txt)."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

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


def _fixed_batch(tr, L):
    """Draw the trainer's batches once on the device and keep them."""
    tr.sample()
    tr.fs.run(L.QC_PHASE_SAMPLE)
    tr._explicit = True


def time_steps(B, steps, warmup, repeats):
    trainer = importlib.import_module(PKG + ".trainer.diffusion_train")
    lbt = importlib.import_module(PKG + ".trainer.lbfgs_train")
    L = importlib.import_module(PKG + ".hip.lib")
    dev = torch.device("cuda", 0)
    loops, keep, lbs = {}, [], {}
    for name in ("adam", "adam_two_call", "lbfgs_m10", "lbfgs_m32"):
        tr = trainer.FusedTrainer(_model(dev), B, capacity=0)
        _fixed_batch(tr, L)
        keep.append(tr)
        if name == "adam":
            loops[name] = tr.step
        elif name == "adam_two_call":
            loops[name] = lambda fs=tr.fs: (fs.run(L.QC_PHASE_GRADS), fs.run(L.QC_PHASE_UPDATE))
        else:
            lb = lbt.LbfgsTrainer(tr, history=int(name.split("_m")[1]), capacity=0)
            lbs[name] = lb
            loops[name] = lb.step
    for fn in loops.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in loops}
    for _ in range(repeats):
        for k, fn in loops.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / steps)
    ms = {k: min(w) * 1e3 for k, w in windows.items()}
    print(json.dumps({"config": "lbfgs_vs_adam_time", "n_qubits": 4, "B_res": B, "B_ic": B // 3, "B_bc": B // 3,
                      "ms_per_evaluation": ms,
                      "two_call_form_ms": ms["adam_two_call"] - ms["adam"],
                      "kernel_vs_adam_tail_ms": {k: ms[k] - ms["adam_two_call"] for k in ("lbfgs_m10", "lbfgs_m32")},
                      "ms_per_evaluation_windows": {k: [round(x * 1e3, 5) for x in w] for k, w in windows.items()},
                      "lbfgs_records": {k: {f: v for f, v in o.state().items()
                                            if f in ("n_eval", "n_iter", "n_rejected", "n_pairs", "stalled", "f0")} for k, o in lbs.items()}}),
          flush=True)


def convergence(B, rows, n_adam, evals, every, m):
    trainer = importlib.import_module(PKG + ".trainer.diffusion_train")
    lbt = importlib.import_module(PKG + ".trainer.lbfgs_train")
    data = importlib.import_module(PKG + ".data.diffusion_dataset")
    tab = importlib.import_module(PKG + ".data.tabulated")
    L = importlib.import_module(PKG + ".hip.lib")
    dev = torch.device("cuda", 0)
    out = {"config": "lbfgs_vs_adam_convergence", "n_qubits": 4, "B_res": B, "adam_steps_first": n_adam, "history": m,
           "evaluations": list(range(every, evals + 1, every))}

    def start():
        ds = tab.TabulatedProblem.from_functions(data.u, data.u, data.r, rows, rows // 3, rows // 3,
                                                 generator=torch.Generator().manual_seed(0))
        torch.manual_seed(3)
        tr = trainer.FusedTrainer(_model(dev), B, capacity=0, dataset=ds)
        _fixed_batch(tr, L)
        for _ in range(n_adam):
            tr.step()
        return tr

    def loss_now(tr):
        tr.fs.run(L.QC_PHASE_GRADS)
        torch.cuda.synchronize()
        p = tr.fs.flat_grad[-3:].cpu().tolist()
        return 2.0 * p[0] + 4.0 * p[1] + 2.0 * p[2]

    tr = start()
    out["loss_after_adam"] = loss_now(tr)
    curve = []
    for e in range(1, evals + 1):
        tr.step()
        if e % every == 0:
            curve.append(loss_now(tr))
    out["adam_only"] = curve
    tr = start()
    lb = lbt.LbfgsTrainer(tr, history=m, capacity=evals)
    curve = []
    for e in range(1, evals + 1):
        lb.step()
        if e % every == 0:
            curve.append(lb.state()["f0"])          # the loss at the last accepted point
    out["adam_then_lbfgs"] = curve
    out["lbfgs_record"] = {k: v for k, v in lb.state().items() if k in ("n_eval", "n_iter", "n_rejected", "n_skipped_pairs",
                                                                        "n_resets", "n_pairs", "stalled")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--convergence", action="store_true")
    ap.add_argument("--rows", type=int, default=1 << 16, help="residual rows of the convergence run's dataset")
    ap.add_argument("--adam", type=int, default=1000)
    ap.add_argument("--evals", type=int, default=500)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--history", type=int, default=10)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import the package (and its built library) from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    for b in a.batches.split(","):
        if a.convergence:
            convergence(int(b), a.rows, a.adam, a.evals, a.every, a.history)
        else:
            time_steps(int(b), a.steps, a.warmup, a.repeats)
