"""Times one L-BFGS evaluation on the device (LbfgsTrainer: the GRADS phase of the fused step + qc_lbfgs_step, history m = 10
and m = 32) beside the Adam step of the same FusedTrainer, and compares loss against evaluation count for Adam alone and
Adam -> L-BFGS.

Time: cascade, 4 qubits, H = 50, one resident batch of B residual + B // 3 initial + B // 3 boundary points at B = 64 and
B = 65 536 (BASELINE config 2).  Four loops alternate window by window in one process: ``adam`` (one call, the fold inside
the optimiser kernel), ``adam_two_call`` (QC_PHASE_GRADS, then QC_PHASE_UPDATE: the separate row-reduction launch the
L-BFGS evaluation also pays), ``lbfgs_m10`` and ``lbfgs_m32``.  Each number is the min of ``repeats`` windows of ``steps``
evaluations after ``warmup``; adam_two_call - adam is the cost of the two-call form, lbfgs - adam_two_call that of the kernel
against k_adam_fast.

Convergence (``--convergence``): the same model on ONE fixed batch gathered from a TabulatedProblem of the analytic
problem's targets: ``--adam`` Adam steps, then ``--evals`` more Adam steps against ``--evals`` L-BFGS evaluations; the loss
every ``--every`` evaluations.  Prints one JSON object per line (profiles/lbfgs_step_bench_runs.txt)."""
import json
import types

import torch

import step_bench as sb


def _fixed_batch(tr, L):
    """Draw the trainer's batches once on the device and keep them."""
    tr.sample()
    tr.fs.run(L.QC_PHASE_SAMPLE)
    tr._explicit = True


def time_steps(B, steps, warmup, repeats):
    trainer, lbt, L = sb.pkg("trainer.diffusion_train"), sb.pkg("trainer.lbfgs_train"), sb.pkg("hip.lib")
    dev = torch.device("cuda", 0)
    loops, keep, lbs = {}, [], {}
    for name in ("adam", "adam_two_call", "lbfgs_m10", "lbfgs_m32"):
        tr = trainer.FusedTrainer(sb.model(dev), B, capacity=0)
        _fixed_batch(tr, L)
        keep.append(tr)
        if name == "adam":
            loops[name] = tr.step
        elif name == "adam_two_call":
            loops[name] = lambda fs=tr.fs: (fs.run(L.QC_PHASE_GRADS), fs.run(L.QC_PHASE_UPDATE))
        else:
            lb = lbt.LbfgsTrainer(tr, history=int(name.split("_m")[1]), capacity=0)
            lbs[name] = lb
            loops[name] = lb.step
    # the batches are fixed: a loop's "sample" does nothing
    r = sb.report("lbfgs_vs_adam_time", sb.warm_up_and_alternate(
        {k: types.SimpleNamespace(sample=lambda: None, step=fn) for k, fn in loops.items()}, steps, warmup, repeats))
    ms = r["ms_per_step"]
    print(json.dumps({"config": r["config"], "n_qubits": 4, "B_res": B, "B_ic": B // 3, "B_bc": B // 3,
                      "ms_per_evaluation": ms,
                      "two_call_form_ms": ms["adam_two_call"] - ms["adam"],
                      "kernel_vs_adam_tail_ms": {k: ms[k] - ms["adam_two_call"] for k in ("lbfgs_m10", "lbfgs_m32")},
                      "ms_per_evaluation_windows": r["ms_per_step_windows"],
                      "lbfgs_records": {k: {f: v for f, v in o.state().items()
                                            if f in ("n_eval", "n_iter", "n_rejected", "n_pairs", "stalled", "f0")} for k, o in lbs.items()}}),
          flush=True)


def convergence(B, rows, n_adam, evals, every, m):
    trainer, lbt, L = sb.pkg("trainer.diffusion_train"), sb.pkg("trainer.lbfgs_train"), sb.pkg("hip.lib")
    dev = torch.device("cuda", 0)
    out = {"config": "lbfgs_vs_adam_convergence", "n_qubits": 4, "B_res": B, "adam_steps_first": n_adam, "history": m,
           "evaluations": list(range(every, evals + 1, every))}

    def start():
        ds = sb.dataset(rows)
        torch.manual_seed(3)
        tr = trainer.FusedTrainer(sb.model(dev), B, capacity=0, dataset=ds)
        _fixed_batch(tr, L)
        for _ in range(n_adam):
            tr.step()
        return tr

    def loss_now(tr):
        tr.fs.run(L.QC_PHASE_GRADS)
        torch.cuda.synchronize()
        p = tr.fs.flat_grad[-3:].cpu().tolist()
        return 2.0 * p[0] + 4.0 * p[1] + 2.0 * p[2]

    tr = start()
    out["loss_after_adam"] = loss_now(tr)
    curve = []
    for e in range(1, evals + 1):
        tr.step()
        if e % every == 0:
            curve.append(loss_now(tr))
    out["adam_only"] = curve
    tr = start()
    lb = lbt.LbfgsTrainer(tr, history=m, capacity=evals)
    curve = []
    for e in range(1, evals + 1):
        lb.step()
        if e % every == 0:
            curve.append(lb.state()["f0"])          # the loss at the last accepted point
    out["adam_then_lbfgs"] = curve
    out["lbfgs_record"] = {k: v for k, v in lb.state().items() if k in ("n_eval", "n_iter", "n_rejected", "n_skipped_pairs",
                                                                        "n_resets", "n_pairs", "stalled")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments(rows=None)
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--convergence", action="store_true")
    ap.add_argument("--rows", type=int, default=1 << 16, help="residual rows of the convergence run's dataset")
    ap.add_argument("--adam", type=int, default=1000)
    ap.add_argument("--evals", type=int, default=500)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--history", type=int, default=10)
    ap.add_argument("--root", default=sb.ROOT, help="checkout to import the package (and its built library) from")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        if a.convergence:
            convergence(int(b), a.rows, a.adam, a.evals, a.every, a.history)
        else:
            time_steps(int(b), a.steps, a.warmup, a.repeats)
