"""Generates ``hybrid_pinn_train.npz``: the third workload (the reference's ``trainer/train.py``) pinned by the reference's
own code.  Run ONCE in the build container::

    QC_REFERENCE_DIR=<checkout of the reference project> python tests/golden/make_golden_hybrid_pinn.py

The reference's ``trainer/train.py`` is imported from QC_REFERENCE_DIR (never copied) with stub modules in place of
``pennylane`` and ``qiskit_ibm_runtime``, which it imports at module level and this image lacks.  Its ``HybridPINN`` is
replaced by the float64 stand-in of ``tests/hybrid_pinn_reference.py`` (oracle circuit: RX, RY, RZ, CNOT of
``oracle/statevector.py``; created encoder, q_layer, decoder like the reference, TorchLayer's uniform [0, 2 pi) weights),
and the reference's own ``train_model`` runs for ``Config.EPOCHS = 20`` (21 iterations) on the CPU.

Recorded (all arrays):
  * ``init__<key>`` / ``final__<key>``: the stand-in's state_dict (float32 initial values; float64 after training);
  * ``res`` (21, 64, 3), ``ic`` / ``bc`` (21, 32, 3): every iteration's batches, captured by wrapping PDESampler's methods,
    and ``u_ic`` / ``u_bc``: the sampler's ``exact_u`` targets on them;
  * ``loss_history`` (21,): what train_model returns;
  * ``pde_X`` (64, 3), ``pde_u`` / ``pde_f`` (64, 1): the reference's ``get_pde_residual`` on the first residual batch
    with the initial weights.
Pinned by the reference: optimiser, scheduler, loss weights, sampling order and shapes, the operator.  Not pinned: the
circuit arithmetic and the TorchLayer initialiser (parity unpinned).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
if not os.environ.get("QC_REFERENCE_DIR"):
    sys.exit("make_golden_hybrid_pinn.py imports the reference project: set QC_REFERENCE_DIR to its checkout")

import hybrid_pinn_reference as R            # noqa: E402


def _reference_train_module():
    """The reference's trainer/train.py with its two unavailable imports stubbed."""
    qml = types.ModuleType("pennylane")
    qiskit = types.ModuleType("qiskit_ibm_runtime")
    qiskit.QiskitRuntimeService = object
    sys.modules.setdefault("pennylane", qml)
    sys.modules.setdefault("qiskit_ibm_runtime", qiskit)
    path = os.path.join(os.environ["QC_REFERENCE_DIR"], "trainer", "train.py")
    spec = importlib.util.spec_from_file_location("reference_trainer_train", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Cast(torch.nn.Module):
    """The float64 stand-in behind the reference's float32 inputs."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x.double())


def main():
    ref = _reference_train_module()
    cfg = ref.Config
    cfg.EPOCHS = 20
    init = {}

    class StandInPINN(torch.nn.Module):
        def __init__(self, device_atom):
            super().__init__()
            m = R.StandIn(cfg.N_QUBITS, cfg.N_LAYERS, cfg.CLASSICAL_HIDDEN)
            init.update({k: v.detach().numpy().copy() for k, v in m.state_dict().items()})
            self.m = m.double()
            # the reference's parameter order (encoder, q_layer, decoder) for its Adam
            self.encoder, self.q_layer, self.decoder = m.encoder, m.q_layer, m.decoder

        def forward(self, x):
            return self.m(x.double())

    ref.HybridPINN = StandInPINN
    got = {"res": [], "ic": [], "bc": [], "u_ic": [], "u_bc": []}
    S = ref.PDESampler
    dom, ini, bnd = S.sample_domain, S.sample_initial, S.sample_boundary

    def sample_domain(self, n):
        t, x, y = dom(self, n)
        got["res"].append(torch.cat([t, x, y], 1).numpy().copy())
        return t, x, y

    def sample_initial(self, n):
        t, x, y, u = ini(self, n)
        got["ic"].append(torch.cat([t, x, y], 1).numpy().copy())
        got["u_ic"].append(u.numpy().copy())
        return t, x, y, u

    def sample_boundary(self, n):
        t, x, y, u = bnd(self, n)
        got["bc"].append(torch.cat([t, x, y], 1).numpy().copy())
        got["u_bc"].append(u.numpy().copy())
        return t, x, y, u

    S.sample_domain, S.sample_initial, S.sample_boundary = sample_domain, sample_initial, sample_boundary
    model, history = ref.train_model()
    out = {"init__" + k: v for k, v in init.items()}
    out.update({"final__" + k: v.detach().numpy().copy() for k, v in model.m.state_dict().items()})
    out.update({k: np.stack(v) for k, v in got.items()})
    out["loss_history"] = np.asarray(history, dtype=np.float64)

    fresh = R.StandIn(cfg.N_QUBITS, cfg.N_LAYERS, cfg.CLASSICAL_HIDDEN)
    fresh.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    X = torch.from_numpy(out["res"][0])
    f, u = ref.get_pde_residual(_Cast(fresh.double()), X[:, 0:1].clone(), X[:, 1:2].clone(), X[:, 2:3].clone())
    out.update(pde_X=X.numpy(), pde_u=u.detach().double().numpy(), pde_f=f.detach().double().numpy())
    np.savez_compressed(os.path.join(HERE, "hybrid_pinn_train.npz"), **out)
    print("loss history", out["loss_history"])


if __name__ == "__main__":
    main()
