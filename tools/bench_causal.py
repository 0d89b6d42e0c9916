"""Times one fused training step under causal weights (CausalTrainer: the slab-stratified gather +
qc_fused_pinn_causal_step, the slab weights formed on the device) beside the tabulated step (qc_fused_pinn_data_step) at
the same shapes: cascade, 4 qubits, H = 50.  Shapes are ``B:M:n_val`` triples: B residual points in M time slabs and n_val
initial and n_val boundary points; the defaults are the smallest causal shape, 128 + 21 + 21 points in 2 slabs (a causal
batch holds whole 64-point tiles of every slab, so 64 residual points cannot be split), and 65 536 + 2 x 21 845 points in
16 slabs (BASELINE config 2).  The two steps alternate window by window on one device; each number is the min of
`repeats` windows of `steps` steps after `warmup` steps, the method of tools/step_bench.py.  Prints one JSON object per
shape.

``--root DIR`` imports the package from another checkout of this repository (built there), and ``--modes`` selects the
steps: an A/B run of a parent commit that has no causal step is

    python tools/bench_causal.py --root ../parent --modes tabulated --label parent
    python tools/bench_causal.py --label change

alternated in one call (profiles/causal_step_bench_runs.txt)."""
import json

import torch

import step_bench as sb

MODES = ("tabulated", "causal")


def run(B, M, n_val, rows, steps, warmup, repeats, modes, label, eps):
    dev = torch.device("cuda", 0)
    trs = {}
    if "tabulated" in modes:
        trs["tabulated"] = sb.pkg("trainer.diffusion_train").FusedTrainer(sb.model(dev), B, capacity=0, dataset=sb.dataset(rows),
                                                                          n_ic=n_val, n_bc=n_val)
    if "causal" in modes:
        weighting = sb.pkg("data.tabulated").CausalWeighting(M, eps=eps)
        trs["causal"] = sb.pkg("trainer.causal_train").CausalTrainer(sb.model(dev), B, sb.dataset(rows), weighting, capacity=0,
                                                                     n_ic=n_val, n_bc=n_val)
    out = sb.report("causal_vs_tabulated", sb.warm_up_and_alternate(trs, steps, warmup, repeats), label=label, n_qubits=4,
                    B_res=B, n_slabs=M, B_ic=n_val, B_bc=n_val, dataset_rows=[rows, rows // 3, rows // 3])
    out["loss"] = sb.losses(trs)
    if "causal" in trs:
        eps_now, raised = trs["causal"].epsilon()
        out["causal"] = {"eps": eps_now, "n_raised": raised, "W_min": float(trs["causal"].causal_weights().min())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(modes=MODES)
    ap.add_argument("--shapes", default="128:2:21,65536:16:21845", help="B:M:n_val triples")
    ap.add_argument("--eps", type=float, default=1.0)
    a = sb.parse(ap)
    for shape in a.shapes.split(","):
        B, M, n_val = (int(v) for v in shape.split(":"))
        run(B, M, n_val, a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label, a.eps)
