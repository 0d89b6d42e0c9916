"""Times one fused training step under gradient-norm loss weights (GradNormTrainer: qc_fused_pinn_gradnorm_step, the class
fold and the combination launch ahead of the optimiser) beside the tabulated step (qc_fused_pinn_data_step) at the same
shapes: cascade, 4 qubits, H = 50.  Shapes are ``B:n_val`` pairs: B residual points and n_val initial and n_val boundary
points, n_val a multiple of 64; the defaults are 128 + 64 + 64 points and 65 536 + 2 x 21 888 points (BASELINE config 2
with the value batches on a tile boundary, 21 888 = 342 x 64).  The two steps alternate window by window on one device;
each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of tools/step_bench.py.
Prints one JSON object per shape.

``--root DIR`` imports the package from another checkout of this repository (built there), and ``--modes`` selects the
steps, as in tools/bench_causal.py.

``--convergence N``: instead of timing, N steps of the tabulated step (fixed weights 2, 4, 2) and of the gradient-norm step
on the same seed at the first shape; prints the loss parts and the weights every N / 20 steps.  An illustration of what
the weights do, not a comparison of the two rules."""
import json

import torch

import step_bench as sb

MODES = ("tabulated", "gradnorm")


def _trainers(B, n_val, rows, modes, alpha, every, capacity=0):
    dev = torch.device("cuda", 0)
    trs = {}
    if "tabulated" in modes:
        torch.manual_seed(7)
        trs["tabulated"] = sb.pkg("trainer.diffusion_train").FusedTrainer(sb.model(dev), B, capacity=capacity,
                                                                          dataset=sb.dataset(rows), n_ic=n_val, n_bc=n_val)
    if "gradnorm" in modes:
        weighting = sb.pkg("nn.loss_balance").GradNormWeighting(alpha=alpha, every=every)
        torch.manual_seed(7)
        trs["gradnorm"] = sb.pkg("trainer.gradnorm_train").GradNormTrainer(sb.model(dev), B, weighting, sb.dataset(rows),
                                                                           capacity=capacity, n_ic=n_val, n_bc=n_val)
    return trs


def run(B, n_val, rows, steps, warmup, repeats, modes, label, alpha, every):
    trs = _trainers(B, n_val, rows, modes, alpha, every)
    out = sb.report("gradnorm_vs_tabulated", sb.warm_up_and_alternate(trs, steps, warmup, repeats), label=label, n_qubits=4,
                    B_res=B, B_ic=n_val, B_bc=n_val, dataset_rows=[rows, rows // 3, rows // 3])
    out["loss"] = sb.losses(trs)
    if "gradnorm" in trs:
        out["gradnorm"] = dict(zip(("lam_bc", "lam_ic"), trs["gradnorm"].weights()), **trs["gradnorm"].gradient_stats())
    print(json.dumps(out), flush=True)


def convergence(B, n_val, rows, steps, alpha, every):
    trs = _trainers(B, n_val, rows, MODES, alpha, every, capacity=steps)
    mark = max(steps // 20, 1)
    print(f"# {B} + {n_val} + {n_val} points, {steps} steps, alpha {alpha}, every {every}; columns: step | fixed weights: "
          f"L_r L_bc L_ic | gradient-norm weights: L_r L_bc L_ic lam_bc lam_ic", flush=True)
    for it in range(steps):
        for tr in trs.values():
            tr.sample()
            tr.step()
        if it % mark == 0 or it == steps - 1:
            (_, *a), _ = trs["tabulated"].losses()
            (_, *b), _ = trs["gradnorm"].losses()
            lam = trs["gradnorm"].weights()
            print(f"{it:6d} | " + " ".join(f"{v:.4e}" for v in a) + " | " + " ".join(f"{v:.4e}" for v in b)
                  + f" {lam[0]:.3e} {lam[1]:.3e}", flush=True)


if __name__ == "__main__":
    ap = sb.arguments(modes=MODES)
    ap.add_argument("--shapes", default="128:64,65536:21888", help="B:n_val pairs")
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--convergence", type=int, default=0, metavar="N", help="print loss parts and weights over N steps instead")
    a = sb.parse(ap)
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    if a.convergence:
        convergence(*shapes[0], a.rows, a.convergence, a.alpha, a.every)
    else:
        for B, n_val in shapes:
            run(B, n_val, a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label, a.alpha, a.every)
