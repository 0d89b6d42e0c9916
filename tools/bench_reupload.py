"""Times one fused training step of a re-uploaded DVPDESolver (args["reupload"]: an EMBED layer in front of every ansatz
layer after the first, the kernels of csrc/qc_circuit_reup*.h*) beside the plain model of the same depth: cascade, 4 qubits,
H = 50, L = 2 and 3 layers, B residual + B // 3 initial + B // 3 boundary points at B = 64 and B = 65 536, on-device
coordinate draw.  The plain model is the yardstick of the same process: it runs compile-time programs where one is
generated and the merged one-launch-per-stage form, the re-uploaded model the run-time interpreter in the two-stream form
(QC_NO_STATIC=1 QC_NO_MERGE=1 puts the plain model on the same footing).  The loops alternate window by window on one
device; each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of
tools/step_bench.py.  Prints one JSON object per batch size and depth."""
import json
import os

import torch

import step_bench as sb


def run(B, L, steps, warmup, repeats):
    trainer = sb.pkg("trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    trs = {k: trainer.FusedTrainer(sb.model(dev, num_quantum_layers=L, reupload=k == "reupload"), B, capacity=0)
           for k in ("plain", "reupload")}
    r = sb.report("reupload_vs_plain", sb.warm_up_and_alternate(trs, steps, warmup, repeats))
    ms = r["ms_per_step"]
    out = {"config": r["config"], "q_ansatz": "cascade", "n_qubits": 4, "n_layers": L, "H": 50, "B_res": B, "B_ic": B // 3,
           "B_bc": B // 3, "n_gates": {k: int(tr.model.quantum_layer.program.n_gates) for k, tr in trs.items()},
           "ms_per_step": ms, "difference_ms": ms["reupload"] - ms["plain"], "ms_per_step_median": r["ms_per_step_median"],
           "switches": {k: os.environ.get(k, "") for k in ("QC_NO_STATIC", "QC_NO_MERGE")}, "loss": sb.losses(trs)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(rows=None)
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--layers", default="2,3")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        for L in a.layers.split(","):
            run(int(b), int(L), a.steps, a.warmup, a.repeats)
