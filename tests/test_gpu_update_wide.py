"""The step after an in-library update on the k_adam path (NP + 3 > 3072, csrc/qc_optim.hip): there the optimiser kernel
rebuilds the per-gate trig table and the phase tables of the diagonal runs from GLOBAL memory with 1024 threads (the
k_adam_fast kernel of the narrower models hands the new theta over through LDS).  tests/test_gpu_fused_widths.py checks
the parameters after that update but never evaluates the circuit again; test_step_after_update_matches_fresh_model
(tests/test_gpu_fused_families.py) evaluates it again, at H = 50 only, which is the fast path.

As there: GRADS | UPDATE at lr 0.05, then GRADS, against a fresh model built on the updated weights, at the same
1e-6 x max(1, max |g|); theta must have moved by more than 1e-2."""
import numpy as np
import pytest
import torch

from conftest import pkg
from step_reference import step_inputs
from test_gpu_fullsize import Log, base_args, grads_for

pytestmark = pytest.mark.gpu

H = 300
ADAM_FAST_MAX = 3072      # k_adam_fast serves NP + 3 <= 3 x 1024
# (ansatz, n, layers, B_res, n_ic, n_bc, split)
CASES = [("layered", 8, 2, 40, 10, 10, False),        # wave family, diagonal runs
         ("cross_mesh", 8, 1, 40, 10, 10, False),     # wave family, 56 CRZ + 8 RZ as one phase-table run
         ("cascade", 4, 1, 70, 30, 20, False),        # register family
         ("layered", 8, 2, 40, 10, 10, True)]         # GRADS, then UPDATE through qc_adam_step


def _model(gpu_device, ans, n, L, flat):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, classic_network=[3, H, 1]), Log(),
                   device=gpu_device)
    eng = model._engine_for(gpu_device)
    with torch.no_grad():
        eng.flat.copy_(torch.from_numpy(np.asarray(flat, dtype=np.float32)))
    return model, eng


@pytest.mark.parametrize("ans,n,L,B_res,n_ic,n_bc,split", CASES, ids=[f"{c[0]}{c[1]}" + ("_split" if c[6] else "") for c in CASES])
def test_step_after_k_adam_update_matches_fresh_model(ans, n, L, B_res, n_ic, n_bc, split, gpu_device):
    Lb = pkg("hip.lib")
    engine = pkg("hip.engine")
    n_theta = L * pkg("circuits").params_per_layer(ans, n)
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=4)
    model, eng = _model(gpu_device, ans, n, L, flat)
    assert eng.NP + 3 > ADAM_FAST_MAX, eng.NP                  # the k_adam path
    eng.refresh_gates()
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.05, gpu_device))
    fs.X_res[:B_res] = X_res.to(gpu_device)
    fs.X_val[:n_ic] = X_ic.to(gpu_device)
    fs.X_val[n_ic:n_ic + n_bc] = X_bc.to(gpu_device)
    if split:
        fs.run(Lb.QC_PHASE_GRADS)
        fs.run(Lb.QC_PHASE_UPDATE)
    else:
        fs.run(Lb.QC_PHASE_GRADS | Lb.QC_PHASE_UPDATE)
    assert fs.opt.read()["step"] == 1
    fs.run(Lb.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    g1 = fs.flat_grad.cpu().numpy().astype(np.float64)
    new = eng.flat.detach().cpu().numpy()
    th = slice(eng.theta_off, eng.theta_off + n_theta)
    assert np.abs(new[th] - flat[th]).max() > 1e-2            # the update moved theta (lr 0.05)
    model2, _ = _model(gpu_device, ans, n, L, new)
    g2 = grads_for(model2, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)
    scale = max(1.0, np.abs(g2).max())
    assert np.isfinite(g1).all() and np.abs(g1 - g2).max() < 1e-6 * scale, np.abs(g1 - g2).max() / scale
