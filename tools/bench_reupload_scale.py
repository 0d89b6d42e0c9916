"""Times one fused training step of a DVPDESolver with trainable input scalings of the re-uploaded angles
(args["reupload_scale"] = "wire": RX(s a_w) in front of every ansatz layer after the first, the SCALED kernels of
csrc/qc_circuit_reup*.h*) beside the re-uploaded model without them and the plain model of the same depth: cascade,
4 qubits, H = 50, L = 2 and 3 layers, B residual + B // 3 initial + B // 3 boundary points at B = 64 and B = 65 536,
on-device coordinate draw.  The three loops alternate window by window on one device; each number is the min of `repeats`
windows of `steps` steps after `warmup` steps, the method of tools/step_bench.py.  Prints one JSON object per batch size
and depth.  ``--modes`` / ``--root`` / ``--label`` time a subset from another checkout (one that has no scalings:
``--root ../parent --modes plain,reupload --label parent``).

``--convergence N``: instead of timing, N training steps of the three models from the same seed (L = 2, B = 1024, the
analytic convection-diffusion problem, problem 0); prints the loss parts, and the scalings of the third model, every 50
steps and at the end, one JSON object per line."""
import json
import os

import torch

import step_bench as sb

KINDS = {"plain": {}, "reupload": {"reupload": True}, "scaled": {"reupload": True, "reupload_scale": "wire"}}


def trainers(B, L, modes):
    trainer = sb.pkg("trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    return {k: trainer.FusedTrainer(sb.model(dev, num_quantum_layers=L, **KINDS[k]), B, capacity=0) for k in modes}


def run(B, L, steps, warmup, repeats, modes, label):
    trs = trainers(B, L, modes)
    r = sb.report("reupload_scale_vs_reupload_vs_plain", sb.warm_up_and_alternate(trs, steps, warmup, repeats))
    ms = r["ms_per_step"]
    out = {"config": r["config"], "label": label, "q_ansatz": "cascade", "n_qubits": 4, "n_layers": L, "H": 50, "B_res": B,
           "B_ic": B // 3, "B_bc": B // 3, "n_gates": {k: int(tr.model.quantum_layer.program.n_gates) for k, tr in trs.items()},
           "n_theta": {k: int(tr.model.quantum_layer.program.n_params) for k, tr in trs.items()},
           "ms_per_step": ms, "ms_per_step_median": r["ms_per_step_median"], "ms_per_step_windows": r["ms_per_step_windows"],
           "switches": {k: os.environ.get(k, "") for k in ("QC_NO_STATIC", "QC_NO_MERGE")}, "loss": sb.losses(trs)}
    if "scaled" in ms and "reupload" in ms:
        out["scaled_minus_reupload_ms"] = ms["scaled"] - ms["reupload"]
    print(json.dumps(out), flush=True)


def convergence(n_steps, B, L, modes):
    trs = trainers(B, L, modes)

    def line(k, tr, step):
        rec = tr.opt.read()
        out = {"convergence": k, "step": step, "loss": rec["loss"], "loss_res": rec["loss_res"], "loss_bc": rec["loss_bc"],
               "loss_ic": rec["loss_ic"], "lr": rec["lr"]}
        s = tr.model.quantum_layer.embed_scale
        if s is not None:
            out["embed_scale"] = [round(float(v), 5) for v in s.detach().cpu().reshape(-1)]
        print(json.dumps(out), flush=True)
    for step in range(1, n_steps + 1):
        for k, tr in trs.items():
            tr.sample()
            tr.step()
            if step % 50 == 0 or step == n_steps:
                line(k, tr, step)


if __name__ == "__main__":
    ap = sb.arguments(rows=None, modes=tuple(KINDS))
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--layers", default="2,3")
    ap.add_argument("--convergence", type=int, default=0, metavar="N")
    a = sb.parse(ap)
    modes = a.modes.split(",")
    if a.convergence:
        convergence(a.convergence, 1024, 2, modes)
    else:
        for b in a.batches.split(","):
            for L in a.layers.split(","):
                run(int(b), int(L), a.steps, a.warmup, a.repeats, modes, a.label)
