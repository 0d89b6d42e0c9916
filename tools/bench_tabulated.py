"""Times one fused training step on tabulated targets (FusedTrainer(..., dataset=): device gather from a resident
dataset + qc_fused_pinn_data_step) beside the analytic problem-0 step (on-device coordinate draw +
qc_fused_pinn_residual_step) at the same shapes: cascade, 4 qubits, H = 50, B residual + B // 3 initial + B // 3 boundary
points at B = 64 and B = 65 536 (BASELINE config 2).  The two steps alternate window by window on one device; each number
is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of tools/step_bench.py.  Prints
one JSON object per batch size."""
import json

import torch

import step_bench as sb


def run(B, rows, steps, warmup, repeats):
    trainer = sb.pkg("trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    trs = {"analytic": trainer.FusedTrainer(sb.model(dev), B, capacity=0),
           "tabulated": trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=sb.dataset(rows))}
    r = sb.report("tabulated_vs_analytic", sb.warm_up_and_alternate(trs, steps, warmup, repeats))
    ms = r["ms_per_step"]
    out = {"config": r["config"], "n_qubits": 4, "B_res": B, "B_ic": B // 3, "B_bc": B // 3,
           "dataset_rows": [rows, rows // 3, rows // 3], "ms_per_step_analytic": ms["analytic"],
           "ms_per_step_tabulated": ms["tabulated"], "difference_ms": ms["tabulated"] - ms["analytic"],
           "ms_per_step_median": r["ms_per_step_median"], "loss": sb.losses(trs)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments()
    ap.add_argument("--batches", default="64,65536")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats)
