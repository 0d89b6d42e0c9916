"""Times one fused training step of the reference's Navier-Stokes model (cascade, 4 qubits, H = 50, three outputs u, v, p;
SystemTrainer: device gather from a resident dataset + qc_fused_pinn_system_step with navier_stokes_2D_terms()) beside
  - the K = 1 tabulated step at the same sizes (FusedTrainer(..., dataset=): qc_fused_pinn_data_step), and
  - the only way to train this model without the system step: navier_stokes_2D_operator (six channels of the three
    outputs from qc_post_multi) -> three MSEs + the value MSEs -> backward -> clip_grad_norm_ -> torch Adam -> scheduler,
    on batches drawn with torch.randint from the same dataset,
at B residual + B // 3 initial + B // 3 boundary points, B = 64 and B = 65 536.  The three alternate window by window on
one device; each number is the min of `repeats` windows of `steps` steps after `warmup` steps, the method of
tools/step_bench.py.  Prints one JSON object per batch size."""
import json

import torch

import step_bench as sb

W_EQ, W_OUT = (1.0, 1.0, 1.0), (1.0, 1.0, 0.0)       # the pressure is not prescribed on the boundary


class TorchLoop:
    """The torch training loop of a K-output DVPDESolver on a TabulatedSystem (zero residual targets)."""

    def __init__(self, model, B, ds):
        self.model, self.B, self.ds = model, B, ds
        self.pde = sb.pkg("nn.pde")
        self.w_out = torch.tensor(W_OUT, device=ds.X_ic.device)
        self.loss = None

    def sample(self):
        ds, dev = self.ds, self.ds.X_res.device
        pick = lambda X, n: torch.randint(0, X.shape[0], (n,), device=dev)
        self.ki, self.kb, self.kr = pick(ds.X_ic, self.B // 3), pick(ds.X_bc, self.B // 3), pick(ds.X_res, self.B)

    def step(self):
        m, ds = self.model, self.ds
        m.optimizer.zero_grad()
        X = ds.X_res[self.kr]
        res = self.pde.navier_stokes_2D_operator(m, X[:, 0:1].clone(), X[:, 1:2].clone(), X[:, 2:3].clone())
        l_r = sum(w * (r ** 2).mean() for w, r in zip(W_EQ, res))
        l_bc = (self.w_out * ((m(ds.X_bc[self.kb]) - ds.U_bc[self.kb]) ** 2).mean(0)).sum()
        l_ic = (self.w_out * ((m(ds.X_ic[self.ki]) - ds.U_ic[self.ki]) ** 2).mean(0)).sum()
        loss = 2.0 * l_r + 4.0 * l_bc + 2.0 * l_ic
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=1)
        m.optimizer.step()
        m.scheduler.step(loss)
        self.loss = loss


def run(B, rows, steps, warmup, repeats, torch_steps):
    tab = sb.pkg("data.tabulated")
    terms = sb.pkg("nn.pde").navier_stokes_2D_terms()
    dev = torch.device("cuda", 0)
    tp = sb.dataset(rows)
    three = lambda u: torch.stack([u, 0.5 * u, torch.zeros_like(u)], 1).contiguous()
    ts = tab.TabulatedSystem((tp.X_res, None), (tp.X_ic, three(tp.u_ic)), (tp.X_bc, three(tp.u_bc)), terms, W_EQ, W_OUT).to(dev)
    K3 = dict(classic_network=[3, 50, 3])
    trs = {"system": sb.pkg("trainer.system_train").SystemTrainer(sb.model(dev, **K3), B, dataset=ts, capacity=0),
           "tabulated_k1": sb.pkg("trainer.diffusion_train").FusedTrainer(sb.model(dev), B, capacity=0, dataset=tp),
           "torch_loop": TorchLoop(sb.model(dev, **K3), B, ts)}
    n_steps = {"system": steps, "tabulated_k1": steps, "torch_loop": torch_steps}
    r = sb.report("navier_stokes_system", sb.warm_up_and_alternate(trs, steps, warmup, repeats, n_steps))
    ms = r["ms_per_step"]
    out = {"config": r["config"], "n_qubits": 4, "hidden": 50, "outputs": 3, "B_res": B, "B_ic": B // 3, "B_bc": B // 3,
           "dataset_rows": [rows, rows // 3, rows // 3], "steps_per_window": n_steps,
           "ms_per_step_system": ms["system"], "ms_per_step_tabulated_k1": ms["tabulated_k1"],
           "ms_per_step_torch_loop": ms["torch_loop"], "ms_per_step_median": r["ms_per_step_median"],
           "loss": {"system": trs["system"].opt.read()["loss"], "tabulated_k1": trs["tabulated_k1"].opt.read()["loss"],
                    "torch_loop": float(trs["torch_loop"].loss)}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = sb.arguments()
    ap.add_argument("--batches", default="64,65536")
    ap.add_argument("--torch-steps", type=int, default=20, help="steps per window of the torch loop (milliseconds per step)")
    a = sb.parse(ap)
    for b in a.batches.split(","):
        run(int(b), a.rows, a.steps, a.warmup, a.repeats, a.torch_steps)
