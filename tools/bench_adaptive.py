"""Times the fused training step with residual-adaptive sampling (FusedTrainer(..., dataset=, adaptive=): the gather
draws its residual rows from the CDF of qc_adapt_build, qc_fused_pinn_adaptive_step) beside the tabulated and the
coefficient step of the same build at the same shapes: cascade, 4 qubits, H = 50, B residual + B // 3 initial + B // 3
boundary points at B = 64 and B = 65 536, a resident dataset of 2^20 + 2 x 349 525 rows.  The steps alternate window by
window on one device; each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of
tools/step_bench.py.  Prints one JSON object per batch size:

  ms_per_step            tabulated, coef, adaptive (scalar operator) and adaptive_coef (coefficient table), the adaptive
                         ones with rescoring OFF (every = 10^9, one rescoring in the warm-up): what the search costs
                         over the uniform gather
  rescore_ms             one rescoring of the whole residual segment (qc_dataset_scores + qc_adapt_build), min of
                         `repeats` timings of 5 back-to-back calls, and its cost per step at every = 100

profiles/adaptive_ab_bench_runs.txt holds the recorded runs, among them the comparison of the LDS-staged coarse search
(kept) with the search from global memory alone."""
import json
import time

import torch

import step_bench as sb

MODES = ("tabulated", "coef", "adaptive", "adaptive_coef")


def run(B, rows, steps, warmup, repeats, modes, label):
    trainer = sb.pkg("trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    never = sb.pkg("data.tabulated").AdaptiveSampling(power=1, floor=1.0, every=10 ** 9)     # one rescoring, on the first step
    trs = {}
    for k in modes:
        trs[k] = trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=sb.dataset(rows, coef=k.endswith("coef")),
                                      adaptive=never if k.startswith("adaptive") else None)
    windows = sb.warm_up_and_alternate(trs, steps, warmup, repeats)
    rescore = {}
    for k, tr in trs.items():
        if not k.startswith("adaptive"):
            continue
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                tr.fs.rescore()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / 5)
        rescore[k] = min(ts) * 1e3
    out = sb.report("adaptive_vs_coef_vs_tabulated", windows, label=label, n_qubits=4, B_res=B, B_ic=B // 3, B_bc=B // 3,
                    dataset_rows=[rows, rows // 3, rows // 3])
    del out["ms_per_step_windows"]
    out.update({"rescore_ms": rescore, "rescore_ms_per_step_at_every_100": {k: v / 100 for k, v in rescore.items()},
                "mean_score": {k: float(tr.dataset_scores().mean()) for k, tr in trs.items() if k.startswith("adaptive")},
                "loss": sb.losses(trs)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(modes=MODES)
    ap.add_argument("--batches", default="64,65536")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label)
