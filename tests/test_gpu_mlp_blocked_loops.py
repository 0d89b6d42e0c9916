"""The lane = point network kernels walk a wave's hidden units in compile-time blocks (qc_unit_blocks, csrc/qc_mlp.hip:
blocks of 4, then a remainder block of 2 and of 1; the next block's weights are requested while the current one is
computed).  These cases put every shape of that walk behind the float64 reference of tests/mlp_reference.py and
tests/step_reference.py.

A wave owns hq = ceil(H / 4) hidden units.  H in {2, 6, 9, 12, 27, 44, 47} gives hq = 1, 2, 3, 3, 7, 11, 12: every
residue of hq mod 4 (and mod 2, the block size at n = 5), a last wave with fewer units than the others (H = 6: 2, 2, 2,
0; 9: 3, 3, 3, 0; 27: 7, 7, 7, 6; 47: 12, 12, 12, 11) and waves with no unit at all (H = 2, 6, 9).  n = 2, 4, 5 covers
both block sizes and the packed epilogues; batches end on a ragged tile with B mod 64 in {1, 7, 63} or on a full one.

The standalone entry points (qc_pre_forward / qc_pre_backward, their _map variants, qc_post in every mode, mode 2
included) run the checks of tests/test_gpu_mlp_shapes.py on these shapes: same comparisons, same tolerances (POINT_TOL,
ROW_TOL) and the same two mutated references (hidden unit H - 1 dropped, the batch's last point dropped), which must
fail.  The fused step runs at the same widths in merged launches against the step reference with the tolerances of
tests/test_gpu_fused_widths.py and tests/test_gpu_fused_families.py (2e-4 on the gradient, 1e-4 on the loss parts,
relative to max(1, max |ref|)), with a dropped hidden unit and, where one point weighs enough, a dropped residual point
as controls.  Inputs come from
seeded CPU generators; the step references are cached through conftest.cached_oracle (records under
tests/golden/oracle/, written by tests/golden/make_oracle_cache.py)."""
import numpy as np
import pytest
import torch

import hybrid_pinn_reference as HR
import mlp_reference as R
import test_gpu_mlp_shapes as S
from conftest import pkg
from step_reference import step_inputs, step_record

POINT_TOL, ROW_TOL = S.POINT_TOL, S.ROW_TOL      # tests/test_gpu_mlp_shapes.py
TOL_G, TOL_L = 2e-4, 1e-4                        # tests/test_gpu_fused_widths.py, tests/test_gpu_fused_families.py

WIDTHS = (2, 6, 9, 12, 27, 44, 47)
# (H, n, B): every H at every n, the four batch tails rotating over them
TAILS = (65, 71, 127, 128, 193, 7, 191, 64)
CASES = [(H, n, TAILS[(3 * i + j) % len(TAILS)]) for i, H in enumerate(WIDTHS) for j, n in enumerate((2, 4, 5))]

# fused step, register family in merged launches: (ansatz, n, H, B_res, n_ic, n_bc)
STEP_CASES = {
    "H2_n4": ("cascade", 4, 2, 71, 3, 4),
    "H6_n2": ("cascade", 2, 6, 127, 64, 64),
    "H9_n4": ("cascade", 4, 9, 128, 100, 91),
    "H12_n5": ("alternate", 5, 12, 65, 40, 31),
    "H27_n4": ("cascade", 4, 27, 129, 33, 32),
    "H44_n2": ("cascade", 2, 44, 64, 30, 33),
    "H47_n5": ("alternate", 5, 47, 199, 70, 57),
}
# the dropped residual point is a control where the reference itself moves by more than twice the tolerance without it
# (one point of 71 .. 199 carries little of the gradient in the other two cases: 0.9 and 1.4 tolerances)
POINT_CONTROL = ("H6_n2", "H9_n4", "H12_n5", "H27_n4", "H44_n2")


def _controls(tag):
    return ("drop_unit", "drop_res") if tag in POINT_CONTROL else ("drop_unit",)


def test_cases_cover_the_block_walk():
    """No GPU: the shapes reach what they are meant to reach."""
    hq = {H: (H + 3) // 4 for H in WIDTHS}
    assert {q % 4 for q in hq.values()} == {0, 1, 2, 3} and {q % 2 for q in hq.values()} == {0, 1}
    owned = {H: [max(0, min(H, (w + 1) * hq[H]) - w * hq[H]) for w in range(4)] for H in WIDTHS}
    assert any(0 in o for o in owned.values())
    assert any(0 < o[3] < o[0] for o in owned.values())
    assert all(sum(o) == H for H, o in owned.items())
    for cases in (CASES, [(c[2], c[1], c[3]) for c in STEP_CASES.values()]):
        assert {c[0] for c in cases} == set(WIDTHS)
        assert {c[1] for c in cases} == {2, 4, 5}
    assert {c[2] % 64 for c in CASES} == {0, 1, 7, 63}
    assert {c[3] % 64 for c in STEP_CASES.values()} == {0, 1, 7, 63}
    assert {(c[4] + c[5]) % 64 for c in STEP_CASES.values()} >= {0, 1, 7, 63}


# ------------------------------------------------------------------ the float64 reference alone (no GPU)
@pytest.mark.parametrize("case", CASES[::4], ids=S._ids)
def test_reference_tells_the_mutations_apart(case):
    """The mutated references differ from the reference by more than the tolerances the GPU cases compare with."""
    H, n, B, X, q6, flat = S._setup(case, seed=sum(case))
    P = R.unpack(flat, H, n, S.N_THETA)
    for nch in (1, 6):
        a = R.pre_jets(P, X, nch).detach()
        for mapped in (False, True):
            f = HR.angle_map_fwd if mapped else (lambda v: v)
            full = f(a)
            scale = POINT_TOL * max(1.0, full.abs().max().item())
            assert (f(R.pre_jets(P, X, nch, drop_unit=True).detach()) - full).abs().max().item() > scale
            assert (full * S._mask(B, "point") - full).abs().max().item() > scale
        u = R.post_jets(P, torch.from_numpy(q6[:nch]).double()).detach()
        ud = R.post_jets(P, torch.from_numpy(q6[:nch]).double(), drop_unit=True).detach()
        assert (u - ud).abs().max().item() > POINT_TOL * max(1.0, u.abs().max().item())


def _step_inputs(tag):
    ans, n, H, B_res, n_ic, n_bc = STEP_CASES[tag]
    n_theta = pkg("circuits").params_per_layer(ans, n)
    return step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=5)


def _step_job(tag, variant=""):
    ans, n, H, B_res, n_ic, n_bc = STEP_CASES[tag]
    return step_record(ans, n, 1, 1, "angle", *_step_inputs(tag), H=H, variant=variant)


def _step_reference(tag, variant=""):
    """{"grad", "parts"} of the step reference; variant "drop_unit" (hidden unit H - 1 of both networks) or "drop_res"."""
    return _step_job(tag, variant).get()


def oracle_jobs():
    return [_step_job(tag, v) for tag in STEP_CASES for v in ("",) + _controls(tag)]


def _rel(got, want, tol):
    return np.abs(got - want).max() / (tol * max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("tag", list(STEP_CASES))
def test_step_reference_tells_the_mutations_apart(tag):
    """Each control moves the reference gradient by more than twice the tolerance: a result within one tolerance of
    the reference is then more than one tolerance away from the mutated one."""
    ref = _step_reference(tag)
    assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["parts"]).all()
    for v in _controls(tag):
        assert _rel(_step_reference(tag, v)["grad"], ref["grad"], TOL_G) > 2.0, v


# ------------------------------------------------------------------ standalone entry points
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=S._ids)
def test_pre_network_blocked(case, gpu_device):
    S.test_pre_network_forward_and_backward(case, gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=S._ids)
def test_post_network_blocked(case, gpu_device):
    S.test_post_network_every_mode(case, gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=S._ids)
def test_pre_network_map_blocked(case, gpu_device):
    """qc_pre_forward_map / qc_pre_backward_map (a = pi tanh(v)) under the checks of the unmapped entry points."""
    L = pkg("hip.lib")
    lib = L.load()
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    H, n, B, X, _, flat = S._setup(case, seed=7 * sum(case))
    dev = gpu_device
    caught = set()
    Xd, prm = torch.from_numpy(X).to(dev), torch.from_numpy(flat).to(dev)
    names = ("W1", "b1", "W2", "b2")
    cols, NP = S._layout_cols(H, n, names)
    MAP = L.QC_ANGLE_MAP_TANH_PI
    for nch in (1, 6):
        aj = S._nan(dev, nch * n * B + 64)
        L.check(lib.qc_pre_forward_map(Xd.data_ptr(), prm.data_ptr(), H, n, S.N_THETA, MAP, aj.data_ptr(), B, nch, st),
                "qc_pre_forward_map")
        abar = np.random.default_rng(B + nch).standard_normal((nch, n, B)).astype(np.float32)
        part = S._nan(dev, S.ROW0 + (B + 63) // 64 + 2, NP + 3 + S.STRIDE_PAD)
        abar_d = torch.from_numpy(abar).to(dev)
        L.check(lib.qc_pre_backward_map(Xd.data_ptr(), prm.data_ptr(), H, n, S.N_THETA, MAP, aj.data_ptr(), abar_d.data_ptr(),
                                        part.data_ptr(), part.shape[1], S.ROW0, B, nch, st), "qc_pre_backward_map")
        torch.cuda.synchronize(dev)
        got_a = S._untouched(aj, nch * n * B).reshape(nch, n, B)
        got_rows = S._rows(part, B, cols, NP)

        def make(mut):
            P = R.unpack(flat, H, n, S.N_THETA)
            m = S._mask(B, mut)
            a = HR.angle_map_fwd(R.pre_jets(P, X, nch, drop_unit=mut == "unit")) * m
            obj = (torch.from_numpy(abar).double() * a).sum(dim=(0, 1))
            rows = S._tile_rows(obj, [P[k] for k in names], names, H, n, B)[:, cols]
            c = S.Check()
            c.add(f"mapped ajets nch={nch}", got_a, a.detach().numpy(), POINT_TOL)
            c.add(f"mapped pre rows nch={nch}", got_rows, rows, ROW_TOL)
            return c
        S._judge(make, caught)
    S._negative_controls_caught(caught)


# ------------------------------------------------------------------ fused step
@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(STEP_CASES))
def test_fused_step_blocked(tag, gpu_device):
    from test_gpu_fullsize import Log, base_args, grads_for
    ans, n, H, B_res, n_ic, n_bc = STEP_CASES[tag]
    flat, X_ic, X_bc, X_res = _step_inputs(tag)
    ref = _step_reference(tag)
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    torch.manual_seed(1)
    model = Solver(base_args(num_qubits=n, q_ansatz=ans, classic_network=[3, H, 1]), Log(), device=gpu_device)
    eng = model._engine_for(gpu_device)
    with torch.no_grad():
        eng.flat.copy_(torch.from_numpy(flat))
    got = grads_for(model, X_ic, X_bc, X_res).cpu().numpy().astype(np.float64)
    NP = got.size - 3
    assert np.isfinite(got).all()
    eg, el = _rel(got[:NP], ref["grad"], TOL_G), _rel(got[NP:], ref["parts"], TOL_L)
    print(f"{tag}: gradient error / tolerance {eg:.3f}, loss parts error / tolerance {el:.3f}")
    assert eg < 1.0, eg
    assert el < 1.0, (got[NP:], ref["parts"])
    for v in _controls(tag):
        assert _rel(got[:NP], _step_reference(tag, v)["grad"], TOL_G) > 1.0, v
