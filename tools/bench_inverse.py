"""Times one fused training step of an inverse problem (InverseTrainer: one gather launch + qc_fused_pinn_inverse_step,
the operator's seven coefficients trained on the device) beside the tabulated step (scalar operator,
qc_fused_pinn_data_step) and the coefficient step (per-point operator rows, qc_fused_pinn_coef_step) at the same shapes:
cascade, 4 qubits, H = 50, B residual + B // 3 initial + B // 3 boundary points at B = 64 and B = 65 536 (BASELINE config
2).  The steps alternate window by window on one device; each number is the min of `repeats` windows of `steps` steps
after `warmup` steps, the method of tools/step_bench.py.  Prints one JSON object per batch size.

``--root DIR`` imports the package from another checkout of this repository (built there), and ``--modes`` selects the
steps: an A/B run of a parent commit that has no inverse step is

    python tools/bench_inverse.py --root ../parent --modes tabulated,coef --label parent
    python tools/bench_inverse.py --label change

alternated in one call (profiles/inverse_step_bench_runs.txt)."""
import json

import torch

import step_bench as sb

MODES = ("tabulated", "coef", "inverse")


def run(B, rows, steps, warmup, repeats, modes, label):
    trainer = sb.pkg("trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    trs = {}
    if "tabulated" in modes:
        trs["tabulated"] = trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=sb.dataset(rows))
    if "coef" in modes:
        trs["coef"] = trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=sb.dataset(rows, coef=True))
        assert trs["coef"].fs.coef_mode
    if "inverse" in modes:
        op = sb.pkg("data.tabulated").LearnedOperator(fixed={"c_t": 1.0}, learn={"c_x": 0.5, "c_y": 0.5, "d_xx": 0.02, "d_yy": 0.02},
                                                      scale={"d_xx": 0.01, "d_yy": 0.01})
        trs["inverse"] = sb.pkg("trainer.inverse_train").InverseTrainer(sb.model(dev), B, sb.dataset(rows), op, capacity=0)
    out = sb.report("inverse_vs_coef_vs_tabulated", sb.warm_up_and_alternate(trs, steps, warmup, repeats), label=label,
                    n_qubits=4, B_res=B, B_ic=B // 3, B_bc=B // 3, dataset_rows=[rows, rows // 3, rows // 3])
    out["loss"] = sb.losses(trs)
    if "inverse" in trs:
        out["coefficients"] = trs["inverse"].coefficients()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(modes=MODES)
    ap.add_argument("--batches", default="64,65536")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label)
