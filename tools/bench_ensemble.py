"""Times the ensemble step (EnsembleStep: qc_fused_pinn_ensemble_step, M models per launch sequence) beside the single-model
fused step (FusedTrainer: qc_fused_pinn_residual_step) on the reference's own configuration: cascade, 4 qubits, one layer,
H = 50, B residual points and B // 3 initial and B // 3 boundary points drawn on the device, B = 64 and 128.  For every B
the single-model step and the ensemble steps of M = 1, 8, 64, 256, 1024 members alternate window by window on one device;
each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of tools/step_bench.py.

Prints one JSON object per B: ms per ensemble step and models x steps per second at every M, beside M x the single-model
step of the same run (``single_x_M_ms``), their ratio (``speedup``: M single-model steps / one ensemble step) and the spread
of the windows."""
import json

import torch

import step_bench as sb


class EnsembleRun:
    """``sample()`` / ``step()`` over one EnsembleStep of M perturbed copies of the bench model, points drawn in the step."""

    def __init__(self, model, M, B):
        engine, L = sb.pkg("hip.engine"), sb.pkg("hip.lib")
        dev = model._flat.device
        eng = model._engine_for(dev)
        g = torch.Generator(device="cpu").manual_seed(M)
        flats = [eng.flat + 0.01 * torch.randn(eng.NP, generator=g).to(dev) for _ in range(M)]
        opts = [engine.OptimState(eng.NP, 0.005, dev) for _ in range(M)]
        n3 = B // 3
        self.fs = engine.EnsembleStep(eng.circuit, eng.H, flats, opts, [eng._pde(B, n3, n3, n3)] * M, B, n3, n3)
        self.fs.refresh_gates()
        self.fs.set_sampler(1234)
        self.phases = L.QC_PHASE_SAMPLE | L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE

    def sample(self):
        pass

    def step(self):
        self.fs.run(self.phases)

    def loss(self):
        return [self.fs.read(m)["loss"] for m in (0, self.fs.M - 1)]


def run(B, members, steps, warmup, repeats):
    dev = torch.device("cuda", 0)
    model = sb.model(dev)
    torch.manual_seed(7)
    trs = {"single": sb.pkg("trainer.diffusion_train").FusedTrainer(model, B, capacity=0)}
    for M in members:
        trs[f"M{M}"] = EnsembleRun(sb.model(dev), M, B)
    windows = sb.warm_up_and_alternate(trs, steps, warmup, repeats)
    out = sb.report("ensemble_vs_single", windows, n_qubits=4, H=50, B_res=B, B_ic=B // 3, B_bc=B // 3)
    single = out["ms_per_step"]["single"]
    spread = lambda w: (max(w) - min(w)) / min(w)
    out["single_x_M_ms"] = {f"M{M}": M * single for M in members}
    out["speedup"] = {f"M{M}": M * single / out["ms_per_step"][f"M{M}"] for M in members}
    out["models_steps_per_s"] = {"single": 1e3 / single, **{f"M{M}": M * 1e3 / out["ms_per_step"][f"M{M}"] for M in members}}
    out["window_spread"] = {k: round(spread(w), 4) for k, w in windows.items()}
    out["loss_first_last_member"] = {f"M{M}": trs[f"M{M}"].loss() for M in members}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(rows=0)
    ap.add_argument("--batches", default="64,128", help="residual batch sizes B (B // 3 initial and boundary points each)")
    ap.add_argument("--members", default="1,8,64,256,1024")
    a = sb.parse(ap)
    for B in (int(b) for b in a.batches.split(",")):
        run(B, [int(m) for m in a.members.split(",")], a.steps, a.warmup, a.repeats)
