"""The fused training step (qc_fused_pinn_residual_step) at hidden widths other than 50, against the float64 reference of
the network stages (tests/mlp_reference.py) composed with the float64 circuit oracle (oracle/jets.py,
oracle/statevector.py): the [grad | L_r, L_bc, L_ic] vector after QC_PHASE_GRADS, the clipped gradient and the
Adam-updated parameters after QC_PHASE_UPDATE.

H = 1 / 65 / 129 reach the packed geometry on both sides of the fused post threshold; H = 257 / 1024 the rounded
geometry, the split post pair inside a step and the reduce-rows + k_adam tail of the optimiser (NP + 3 > 3072).
Cascade n = 4 runs the register family (merged launches); layered n = 8 the wave family on two streams.  Batches are
ragged, with value-tile counts that are not multiples of 4.

Tolerances as in test_first_step_gradient_matches_reference: 2e-4 x max(1, max |ref|) on the gradient, 1e-4 on the
loss parts; the updated parameters within 2e-6 (fp32 rounding of O(1) parameters) of Adam's float64 update wherever
the gradient is clear of that tolerance: Adam's first step moves a parameter by lr g / (|g| + eps), so only the sign of
g matters there.  A second model takes the same step in ONE call (GRADS | UPDATE): the fold of the partial rows then
rides in the optimiser launch (k_adam_fast) or, past 3072 columns, runs as qc_opt_reduce_rows + k_adam."""
import numpy as np
import pytest
import torch

from conftest import pkg
from step_reference import reference_loss
from test_gpu_solver import Log, base_args

pytestmark = pytest.mark.gpu

ADAM_FAST_MAX = 3072      # k_adam_fast serves NP + 3 <= 3 x 1024 (csrc/qc_optim.hip:adam_fast_ok)


CASES = [(1, {}, 200), (65, {}, 830), (129, {}, 200), (257, {}, 200), (1024, {}, 130),
         (300, {"num_qubits": 8, "num_quantum_layers": 2, "q_ansatz": "layered"}, 200)]


@pytest.mark.parametrize("H,over,batch", CASES, ids=["step_H1", "step_H65_B830", "step_H129", "step_H257", "step_H1024", "step_layered_n8_H300"])
def test_fused_step_at_other_widths_matches_fp64(H, over, batch, gpu_device, tmp_path):
    from oracle import solver as osol
    L = pkg("hip.lib")
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    trainer = pkg("trainer.diffusion_train")
    args = base_args(classic_network=[3, H, 1], **over)
    torch.manual_seed(1)
    model = Solver(args, Log(tmp_path), device=gpu_device)
    tr = trainer.FusedTrainer(model, batch, capacity=4)
    n, ansatz = args["num_qubits"], args["q_ansatz"]
    eng = tr.eng
    NP, n_theta = eng.NP, eng.n_theta
    # the optimiser tail this case is meant to reach
    assert (NP + 3 > ADAM_FAST_MAX) == (H >= 257), NP
    assert tr.B_res % 64 and (tr.n_ic + tr.n_bc) % 64 and ((tr.n_ic + tr.n_bc + 63) // 64) % 4
    g = torch.Generator().manual_seed(H)
    X_ic, X_bc, X_res = [(torch.tensor(b[0]) + (torch.tensor(b[1]) - torch.tensor(b[0])) * torch.rand(m, 3, generator=g))
                         .to(torch.float32)
                         for b, m in ((osol.BOX_IC, tr.n_ic), (osol.BOX_BC1, tr.n_bc), (osol.BOX_DOM, tr.B_res))]
    tr.load_batches(X_ic, X_bc, X_res)
    flat0 = eng.flat.detach().cpu().numpy().copy()
    tr.fs.run(L.QC_PHASE_GRADS)
    got = tr.fs.flat_grad.cpu().numpy()
    Xs = [x.double() for x in (X_ic, X_bc, X_res)]
    theta_shape = tuple(model.quantum_layer.params.shape)
    from oracle import statevector as sv
    ql = model.quantum_layer
    haar = sv.haar_pair(ql.haar_seed1, ql.haar_seed2)     # the fixed two-wire unitaries of the seeded layer
    want_g, want_parts = reference_loss(flat0, H, n, n_theta, theta_shape, ansatz, haar, *Xs)
    gs = max(1.0, np.abs(want_g).max())
    assert np.abs(got[:NP] - want_g).max() < 2e-4 * gs, np.abs(got[:NP] - want_g).max() / gs
    assert np.abs(got[NP:] - want_parts).max() < 1e-4 * max(1.0, np.abs(want_parts).max()), (got[NP:], want_parts)
    # negative control: the reference without hidden unit H - 1 is told apart at this tolerance
    mut_g, _ = reference_loss(flat0, H, n, n_theta, theta_shape, ansatz, haar, *Xs, drop_unit=True)
    assert np.abs(got[:NP] - mut_g).max() > 2e-4 * gs

    tr.fs.run(L.QC_PHASE_UPDATE)
    clipped = tr.fs.flat_grad[:NP].cpu().numpy()
    coef = min(1.0, 1.0 / (np.linalg.norm(want_g) + 1e-6))      # torch.nn.utils.clip_grad_norm_(max_norm=1)
    assert np.abs(clipped - coef * want_g).max() < 2e-4 * max(1.0, coef * np.abs(want_g).max())
    p = torch.nn.Parameter(torch.from_numpy(flat0.astype(np.float64)))
    opt = torch.optim.Adam([p], lr=args["lr"])
    p.grad = torch.from_numpy(coef * want_g)
    opt.step()
    new, want_p = eng.flat.detach().cpu().numpy(), p.detach().numpy()
    # where the gradient is clear of the comparison's error the update is Adam's to fp32 rounding; elsewhere the
    # first step still moves a parameter by at most lr
    clear = np.abs(want_g) > 1e-2 * np.abs(want_g).max()
    assert clear.sum() > NP // 20
    assert np.abs(new - want_p)[clear].max() < 2e-6
    assert np.abs(new - flat0).max() < args["lr"] * (1 + 1e-5) + 1e-6

    # the same step in one call: fold + update tail (reduce rows + k_adam past ADAM_FAST_MAX columns)
    torch.manual_seed(1)
    model2 = Solver(args, Log(tmp_path), device=gpu_device)
    tr2 = trainer.FusedTrainer(model2, batch, capacity=4)
    assert np.array_equal(tr2.eng.flat.detach().cpu().numpy(), flat0)
    tr2.load_batches(X_ic, X_bc, X_res)
    tr2.fs.run(L.QC_PHASE_GRADS | L.QC_PHASE_UPDATE)
    got2 = tr2.fs.flat_grad.cpu().numpy()
    assert np.abs(got2[:NP] - coef * want_g).max() < 2e-4 * max(1.0, coef * np.abs(want_g).max())
    assert np.abs(got2[NP:] - want_parts).max() < 1e-4 * max(1.0, np.abs(want_parts).max())
    new2 = tr2.eng.flat.detach().cpu().numpy()
    assert np.abs(new2 - want_p)[clear].max() < 2e-6
    assert np.abs(new2 - flat0).max() < args["lr"] * (1 + 1e-5) + 1e-6
    assert abs(tr2.opt.read()["loss"] - float(np.dot([2.0, 4.0, 2.0], want_parts))) < 1e-4 * max(1.0, float(want_parts.max()))
