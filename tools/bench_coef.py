"""Times one fused training step with per-point operator rows (FusedTrainer(..., dataset=) on a TabulatedProblem with
coef_res: one gather launch for rows, targets and coefficient rows + qc_fused_pinn_coef_step) beside the tabulated step
(scalar operator, qc_fused_pinn_data_step) and the analytic problem-0 step at the same shapes: cascade, 4 qubits, H = 50,
B residual + B // 3 initial + B // 3 boundary points at B = 64 and B = 65 536 (BASELINE config 2).  The steps alternate
window by window on one device; each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the
method of tools/step_bench.py.  Prints one JSON object per batch size.

``--root DIR`` imports the package from another checkout of this repository (built there), and ``--modes`` selects the
steps: an A/B run of a parent commit that has no coefficient step is

    python tools/bench_coef.py --root ../parent --modes analytic,tabulated --label parent
    python tools/bench_coef.py --label change

alternated in one call (profiles/coef_ab_bench_runs.txt)."""
import json

import torch

import step_bench as sb

MODES = ("analytic", "tabulated", "coef")


def run(B, rows, steps, warmup, repeats, modes, label):
    trainer = sb.pkg("trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    trs = {}
    if "analytic" in modes:
        trs["analytic"] = trainer.FusedTrainer(sb.model(dev), B, capacity=0)
    if "tabulated" in modes:
        trs["tabulated"] = trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=sb.dataset(rows))
    if "coef" in modes:
        trs["coef"] = trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=sb.dataset(rows, coef=True))
        assert trs["coef"].fs.coef_mode
    out = sb.report("coef_vs_tabulated_vs_analytic", sb.warm_up_and_alternate(trs, steps, warmup, repeats), label=label,
                    n_qubits=4, B_res=B, B_ic=B // 3, B_bc=B // 3, dataset_rows=[rows, rows // 3, rows // 3])
    del out["ms_per_step_windows"]
    out["loss"] = sb.losses(trs)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(modes=MODES)
    ap.add_argument("--batches", default="64,65536")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label)
