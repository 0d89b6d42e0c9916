"""The ensemble step (qc_fused_pinn_ensemble_step) on explicit batches, QC_PHASE_GRADS: every member's [grad | L_r, L_bc,
L_ic] against the float64 reference of tests/step_reference.py at the tolerances of tests/test_gpu_fused_families.py (the
gradient block by block at 2e-4 x max(1, max |ref block|), the loss parts at 1e-4), with member 1 against member 0's
reference as the negative control; the exact properties of the member index (a member alone, permuted members, repeated
runs: bit for bit); every member against the single-model step on its slices; and guard bands between the members' slices
of every strided buffer across SAMPLE | GRADS | UPDATE.

Bit-identity with the single-model step is printed, not asserted (DESIGN section 9 records it)."""
import numpy as np
import pytest
import torch

from conftest import pkg
from ensemble_reference import CASES, member_inputs, member_reference, n_theta_of
from test_gpu_fullsize import Log, base_args, grads_for

pytestmark = pytest.mark.gpu

TOL_G, TOL_L = 2e-4, 1e-4
THETA_MIN = 20 * TOL_G
CANARY = 12345.678


def _model(dev, case, flat=None):
    ans, n, L, H = CASES[case][:4]
    torch.manual_seed(1)
    model = pkg("nn.DVPDESolver").DVPDESolver(
        base_args(num_qubits=n, num_quantum_layers=L, q_ansatz=ans, classic_network=[3, H, 1]), Log(), device=dev)
    eng = model._engine_for(dev)
    if flat is not None:
        with torch.no_grad():
            eng.flat.copy_(torch.from_numpy(np.asarray(flat, dtype=np.float32)))
    return model, eng


def _ensemble(dev, case, members=None, pad=0, hist_cap=0):
    """An EnsembleStep over the given members of a case (default: all, in order), explicit batches loaded, gates ready;
    the final-state stores poisoned."""
    engine = pkg("hip.engine")
    ans, n, L, H, M, B_res, n_ic, n_bc = CASES[case]
    members = list(range(M)) if members is None else list(members)
    model, eng = _model(dev, case)
    flats = [torch.from_numpy(member_inputs(case, m)[0]).to(dev) for m in members]
    opts = [engine.OptimState(eng.NP, 0.005, dev, hist_cap=hist_cap) for _ in members]
    pde = eng._pde(B_res, n_ic, n_bc, n_ic)
    fs = engine.EnsembleStep(eng.circuit, H, flats, opts, [pde] * len(members), B_res, n_ic, n_bc, pad=pad)
    fs.step_ws.view(torch.float32).fill_(float("nan"))
    for k, m in enumerate(members):
        _, X_ic, X_bc, X_res = member_inputs(case, m)
        Xr, Xv = fs.points(k)
        Xr[:], Xv[:n_ic], Xv[n_ic:] = X_res.to(dev), X_ic.to(dev), X_bc.to(dev)
    fs.refresh_gates()
    fs._model = model       # the circuit belongs to the model's quantum layer: keep it alive
    return fs


def _grads(fs):
    Lb = pkg("hip.lib")
    fs.run(Lb.QC_PHASE_GRADS)
    torch.cuda.synchronize()
    return fs.flat_grad[:, : fs.NP + 3].cpu().numpy().astype(np.float64)


def _blocks(H, n, n_theta):
    lay = pkg("hip.engine").param_layout(H, n, n_theta)
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    return {"pre": slice(0, o_post), "theta": slice(o_th, NP), "post": slice(o_post, o_th)}


def _errors(got, want_g, blocks):
    """block -> error / tolerance (< 1 passes)."""
    return {name: np.abs(got[s] - want_g[s]).max() / (TOL_G * max(1.0, np.abs(want_g[s]).max())) for name, s in blocks.items()}


def _parts_error(got, parts):
    return np.abs(got - parts).max() / (TOL_L * max(1.0, np.abs(parts).max()))


@pytest.mark.parametrize("case", list(CASES))
def test_every_member_matches_fp64(case, gpu_device):
    ans, n, L, H, M, B_res, n_ic, n_bc = CASES[case]
    n_theta = n_theta_of(case)
    blocks = _blocks(H, n, n_theta)
    got = _grads(_ensemble(gpu_device, case))
    assert got.shape[0] == M and np.isfinite(got).all()
    refs = [member_reference(case, m) for m in range(M)]
    for m in range(M):
        err = _errors(got[m, :-3], refs[m]["grad"], blocks)
        perr = _parts_error(got[m, -3:], refs[m]["parts"])
        print(f"{case} member {m}: error / tolerance by block {err}, loss parts {perr:.3g}")
        assert max(err.values()) < 1.0, (m, err)
        assert perr < 1.0, (m, got[m, -3:], refs[m]["parts"])
        assert np.abs(refs[m]["grad"][blocks["theta"]]).max() > THETA_MIN
    # negative control: member 1's slices are not member 0's, in the network blocks and in the theta block
    bad = _errors(got[1, :-3], refs[0]["grad"], blocks)
    print(f"{case} control (member 1 against member 0's reference): {bad}")
    assert max(bad.values()) > 1.0 and bad["theta"] > 1.0, bad


def test_member_index_is_exact(gpu_device):
    """The same kernels on the same slices: no tolerance."""
    case = "cascade4"
    all3 = _grads(_ensemble(gpu_device, case))
    again = _grads(_ensemble(gpu_device, case))
    assert np.array_equal(all3, again)                                  # two identical runs
    alone = _grads(_ensemble(gpu_device, case, members=[0]))
    assert np.array_equal(all3[0], alone[0])                            # member 0 of M = 3 == an M = 1 run
    perm = [2, 0, 1]
    permuted = _grads(_ensemble(gpu_device, case, members=perm))
    assert np.array_equal(permuted, all3[perm])                         # permuted members permute the flat vectors
    assert not np.array_equal(all3[0], all3[1])


@pytest.mark.parametrize("case", ["cascade4", "cascade3_L2"])
def test_members_match_the_single_model_step(case, gpu_device):
    ans, n, L, H, M, B_res, n_ic, n_bc = CASES[case]
    blocks = _blocks(H, n, n_theta_of(case))
    got = _grads(_ensemble(gpu_device, case))
    for m in range(M):
        flat, X_ic, X_bc, X_res = member_inputs(case, m)
        model, _ = _model(gpu_device, case, flat)
        one = grads_for(model, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)
        print(f"{case} member {m}: bit-identical to the single-model step: {np.array_equal(one, got[m])}, "
              f"max |difference| {np.abs(one - got[m]).max():.3g}")
        err = _errors(got[m, :-3], one[:-3], blocks)
        assert max(err.values()) < 1.0, (m, err)
        assert _parts_error(got[m, -3:], one[-3:]) < 1.0


def test_guard_bands_stay_untouched(gpu_device):
    """Every strided buffer with 64 more floats per member than its slice, the gaps filled with a canary: three whole
    steps with device-drawn points change no gap."""
    Lb = pkg("hip.lib")
    case = "cascade4"
    ans, n, L, H, M, B_res, n_ic, n_bc = CASES[case]
    fs = _ensemble(gpu_device, case, pad=64, hist_cap=4)
    lib, h = fs.lib, fs.circuit.handle
    B_val = n_ic + n_bc
    sizes = {"params": fs.NP, "m": fs.NP, "v": fs.NP, "flat_grad": fs.NP + 3, "hist": 4, "X_res": 3 * B_res, "X_val": 3 * B_val,
             "trig": int(lib.qc_trig_bytes(h)) // 4}
    bufs = {k: (getattr(fs, k), s) for k, s in sizes.items()}
    for i in range(4):
        bufs[f"ws_res{i}"] = (fs.ws_res[i], 6 * n * B_res)
        bufs[f"ws_val{i}"] = (fs.ws_val[i], n * B_val)
    bufs["step_ws"] = (fs.step_ws.view(torch.float32), int(lib.qc_step_workspace_bytes(h, B_res, B_val)) // 4)
    for name, (t, size) in bufs.items():
        assert t.shape[0] == M and t.shape[1] >= size + 64, (name, tuple(t.shape), size)
        t[:, size:] = CANARY
    fs.set_sampler(11)
    for _ in range(3):
        fs.run(Lb.QC_PHASE_SAMPLE | Lb.QC_PHASE_GRADS | Lb.QC_PHASE_UPDATE)
    torch.cuda.synchronize()
    for name, (t, size) in bufs.items():
        gap = t[:, size:].cpu().numpy()
        assert np.array_equal(gap, np.full_like(gap, np.float32(CANARY))), name
    for m in range(M):
        rec = fs.read(m)
        assert rec["step"] == 3 and np.isfinite(rec["loss"])
        assert np.isfinite(fs.params[m, : fs.NP].cpu().numpy()).all()
    # the members drew different points (key seed + m) inside the unit box
    Xs = [fs.points(m)[0].cpu().numpy() for m in range(M)]
    assert all(((X >= 0) & (X <= 1)).all() for X in Xs) and not np.array_equal(Xs[0], Xs[1])
