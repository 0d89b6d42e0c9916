"""Times one fused training step of a problem that is second order in time over two space dimensions (FusedTrainer(...,
dataset=) on a TabulatedProblem with ``d_tt``: seven derivative channels, operator rows of eight columns,
qc_fused_pinn_coef_tt_step) beside the coefficient step (six channels, rows of seven columns, qc_fused_pinn_coef_step) of the
same model, dataset points and batch: cascade, 4 qubits, H = 50, B residual + B // 3 initial + B // 3 boundary points at
B = 64 and B = 65 536.  The steps alternate window by window on one device, in one process; each number is the min of
`repeats` windows of `steps` steps after `warmup` steps, the method of tools/step_bench.py.  Prints one JSON object per batch
size.

The seven-channel step always runs in the two-stream form and recomputes the forward sweep in its adjoint kernel; the
coefficient step beside it is the merged form with kept final states, so the ratio is what a user pays for u_tt today, not
the cost of the seventh channel alone (by instruction count the circuit stages cost 7 / 6).

    timeout 600 python tools/bench_wave.py"""
import json

import torch

import step_bench as sb

MODES = ("coef", "wave")


def wave_dataset(rows, c=0.5):
    """The dataset of tools/step_bench.py with its operator as a table, and the same rows with the wave operator
    u_tt - c^2 (u_xx + u_yy) in eight columns (the targets stay the analytic problem's: only the step's cost is measured)."""
    tab = sb.pkg("data.tabulated")
    ds = sb.dataset(rows, coef=True)
    wave = tab.TabulatedProblem(ds.X_res, ds.r, ds.X_ic, ds.u_ic, ds.X_bc, ds.u_bc,
                                coef_res=tab.coef_table(ds.X_res, d_xx=c * c, d_yy=c * c), d_tt=-1.0)
    return ds, wave


def run(B, rows, steps, warmup, repeats, modes, label):
    trainer = sb.pkg("trainer.diffusion_train")
    dev = torch.device("cuda", 0)
    coef, wave = wave_dataset(rows)
    trs = {}
    if "coef" in modes:
        trs["coef"] = trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=coef)
        assert trs["coef"].fs.coef_mode and not trs["coef"].tt
    if "wave" in modes:
        trs["wave"] = trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=wave)
        assert trs["wave"].tt
    out = sb.report("wave_vs_coef", sb.warm_up_and_alternate(trs, steps, warmup, repeats), label=label, n_qubits=4, B_res=B,
                    B_ic=B // 3, B_bc=B // 3, dataset_rows=[rows, rows // 3, rows // 3])
    out["loss"] = sb.losses(trs)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(modes=MODES)
    ap.add_argument("--batches", default="64,65536")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats, a.modes.split(","), a.label)
