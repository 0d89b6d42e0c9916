"""Times one fused training step under learned loss weights (BalancedTrainer: one gather launch +
qc_fused_pinn_balanced_step, the three log-variances trained on the device) beside the tabulated step (fixed weights,
qc_fused_pinn_data_step) at the same shapes: cascade, 4 qubits, H = 50, B residual + B // 3 initial + B // 3 boundary points
at B = 64 and B = 65 536 (BASELINE config 2).  The two steps alternate window by window on one device; each number is the
min of `repeats` windows of `steps` steps after `warmup` steps, the method of tools/step_bench.py.  Prints one JSON
object per batch size.

``--root DIR`` imports the package from another checkout of this repository (built there), and ``--modes`` selects the
steps: an A/B run of a parent commit that has no balanced step is

    python tools/bench_balanced.py --root ../parent --modes tabulated --label parent
    python tools/bench_balanced.py --label change

alternated in one call (profiles/balanced_step_bench_runs.txt)."""
import json

import torch

import step_bench as sb

MODES = ("tabulated", "balanced")


def run(B, rows, steps, warmup, repeats, modes, label):
    dev = torch.device("cuda", 0)
    trs = {}
    if "tabulated" in modes:
        trs["tabulated"] = sb.pkg("trainer.diffusion_train").FusedTrainer(sb.model(dev), B, capacity=0, dataset=sb.dataset(rows))
    if "balanced" in modes:
        bal = sb.pkg("nn.loss_balance").AdaptiveMultiLoss()
        trs["balanced"] = sb.pkg("trainer.balanced_train").BalancedTrainer(sb.model(dev), B, sb.dataset(rows), bal, capacity=0)
    out = sb.report("balanced_vs_tabulated", sb.warm_up_and_alternate(trs, steps, warmup, repeats), label=label, n_qubits=4,
                    B_res=B, B_ic=B // 3, B_bc=B // 3, dataset_rows=[rows, rows // 3, rows // 3])
    out["loss"] = sb.losses(trs)
    if "balanced" in trs:
        out["weights"] = trs["balanced"].weights()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(modes=MODES)
    ap.add_argument("--batches", default="64,65536")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label)
