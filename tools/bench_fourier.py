"""Times one fused training step of a DVPDESolver behind a Fourier-feature input map (args["fourier_features"] = m: the
pre stages k_pre_ff_fwd_both / k_pre_ff_bwd_both, W1[H][2m]) beside the plain step (W1[H][3]) at the same shapes: cascade,
4 qubits, H = 50, B residual + B // 3 initial + B // 3 boundary points at B = 64 and B = 65 536 (BASELINE config 2), on-device
coordinate draw.  The loops alternate window by window in one process on one device; each number is the min of `repeats`
windows of `steps` steps after `warmup` steps, the method of tools/step_bench.py.  Prints one JSON object per batch
size."""
import json

import torch

import step_bench as sb


def run(B, ms_list, scale, steps, warmup, repeats):
    trainer = sb.pkg("trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    ff = lambda m: dict(fourier_features=m, fourier_scale=scale) if m else {}
    trs = {("plain" if m == 0 else f"m{m}"): trainer.FusedTrainer(sb.model(dev, **ff(m)), B, capacity=0) for m in ms_list}
    r = sb.report("fourier_vs_plain", sb.warm_up_and_alternate(trs, steps, warmup, repeats))
    ms = r["ms_per_step"]
    out = {"config": r["config"], "n_qubits": 4, "H": 50, "B_res": B, "B_ic": B // 3, "B_bc": B // 3, "fourier_scale": scale,
           "NP": {k: int(tr.eng.NP) for k, tr in trs.items()}, "ms_per_step": ms,
           "difference_ms": {k: v - ms["plain"] for k, v in ms.items() if k != "plain"} if "plain" in ms else {},
           "ms_per_step_median": r["ms_per_step_median"], "loss": sb.losses(trs)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(rows=None)
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--features", default="0,8,32", help="mapping sizes m to time; 0 is the plain step")
    ap.add_argument("--scale", type=float, default=1.0)
    a = sb.parse(ap)
    for b in a.batches.split(","):
        run(int(b), [int(m) for m in a.features.split(",")], a.scale, a.steps, a.warmup, a.repeats)
