"""The merged wave sums of tile gradients (qc_wave_sum_merged, csrc/qc_common.h) in the kernels that use them.

(a) tools/ubench/wave_sum_merge, the stand-alone lane-exactness program built next to the library: for NV = 1..16 every
    value's total in its home lane must have the bits of qc_wave_sum_to_lane63.  A missing binary is a failure.

(b) The stages against the float64 step reference (tests/step_reference.py: reference_loss; tolerances TOL_G / TOL_L of
    tests/test_gpu_post_value_geometry.py).  Per case the fused step's five stages run one by one through
    qc_fused_step_stage on a NaN-filled ``part`` and the rows are summed on the host; then the stand-alone calls the merged
    kernels replaced (qc_post mode 2 on the residual and on the value points, qc_forward_jets_keep +
    qc_backward_jets_kept, qc_backward_expval) run on the same workspace into a second ``part``, whose post-network, theta
    and loss columns are compared with the same reference.  Shapes, the smallest at which a merged reduction can go wrong:
      cascade n = 2, 3, 4, 5          N + 2 = 4 .. 7 values per hidden unit: one merged register, or two filled unevenly
      H = 1, 3, 5, 13                 waves of a tile with no hidden unit, with one, and ragged last unit blocks
      residual points 1, 63, 65       dead lanes; a second tile
      value points 1, 65              (IC / BC split inside the tile)
      layered n = 4                   diagonal runs of another length
    Every (n, H) pair occurs once, with the six (residual, value) shapes dealt round robin over the pairs (one exception,
    SHAPE_OF).

(c) No hidden swaps: a total stored from the wrong home lane would land in another column of the same hidden unit (or in
    another slot of the same diagonal run; checked for all diagonal gates of the program as one group).  For every case
    the float64 reference entries within each such group differ pairwise by more than 100 x the tolerance of (b), so no
    such exchange can pass (b).
    The seeds (``salt`` of step_inputs) were chosen for that on the CPU, from the reference alone; the check needs no GPU.

The reference records are committed under tests/golden/oracle/ (tests/golden/make_oracle_cache.py)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import cached_oracle, pkg
from step_reference import haar_for, reference_loss, step_inputs
from test_gpu_fullsize import Log, base_args

TOL_G, TOL_L = 2e-4, 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UBENCH = os.path.join(ROOT, "tools", "ubench", "wave_sum_merge")

SHAPES = [(1, 1, 0), (63, 33, 32), (65, 1, 0), (1, 33, 32), (63, 0, 1), (65, 32, 33)]   # (B_res, n_ic, n_bc)
# (n, H) -> salt of step_inputs for which (c) holds (found on the CPU; see test_groups_are_pairwise_distinct)
SALTS = {("cascade", 2, 1): 3, ("cascade", 2, 3): 1, ("cascade", 2, 5): 2, ("cascade", 2, 13): 15,
         ("cascade", 3, 1): 5, ("cascade", 3, 3): 9, ("cascade", 3, 5): 10, ("cascade", 3, 13): 196,
         ("cascade", 4, 1): 6, ("cascade", 4, 3): 5, ("cascade", 4, 5): 9, ("cascade", 4, 13): 141,
         ("cascade", 5, 1): 9, ("cascade", 5, 3): 7, ("cascade", 5, 5): 124, ("cascade", 5, 13): 123,
         ("layered", 4, 5): 40}


# the one pair whose dealt shape (1 residual point, 65 value points) has no such seed among 800: it takes (63, 65)
SHAPE_OF = {(5, 13): 1}


def _cases():
    out = {}
    for j, (n, H) in enumerate(itertools.product((2, 3, 4, 5), (1, 3, 5, 13))):
        B_res, n_ic, n_bc = SHAPES[SHAPE_OF.get((n, H), j % len(SHAPES))]
        out[f"cascade{n}_H{H}_r{B_res}_v{n_ic + n_bc}"] = ("cascade", n, H, B_res, n_ic, n_bc, SALTS.get(("cascade", n, H), 4))
    out["layered4_H5_r65_v65"] = ("layered", 4, 5, 65, 32, 33, SALTS.get(("layered", 4, 5), 4))
    return out


CASES = _cases()


def case_inputs(case):
    """step_inputs of the case, with the output layer's weights redrawn: alternating sign, magnitude in [0.5, 1.5) / sqrt(H).
    (A hidden unit's N + 2 gradient columns all carry the factor W4[m]; with the normal draw some units' columns are
    hundreds of times smaller than the largest entry of the block, which sets the tolerance, and (c) cannot hold.)"""
    ans, n, H, B_res, n_ic, n_bc, salt = CASES[case]
    n_theta = int(pkg("circuits").params_per_layer(ans, n))
    flat, X_ic, X_bc, X_res = step_inputs(H, n, n_theta, B_res, n_ic, n_bc, salt=salt)
    oW4 = pkg("hip.engine").param_layout(H, n, n_theta)["postprocessor.2.weight"][0]
    rng = np.random.default_rng(salt)
    flat[oW4:oW4 + H] = (np.where(np.arange(H) % 2, -1.0, 1.0) * (0.5 + rng.random(H)) / np.sqrt(H)).astype(np.float32)
    return flat, X_ic, X_bc, X_res


def case_reference(case):
    """{"grad": (NP,), "parts": (3,)} float64, through the committed record of the case."""
    ans, n, H, B_res, n_ic, n_bc, salt = CASES[case]
    n_theta = int(pkg("circuits").params_per_layer(ans, n))
    flat, X_ic, X_bc, X_res = case_inputs(case)

    def compute():
        g, parts = reference_loss(flat, H, n, n_theta, (1, n_theta), ans, haar_for(n, 1),
                                  *(torch.as_tensor(x).double() for x in (X_ic, X_bc, X_res)), encoding="angle")
        return {"grad": g, "parts": parts}
    inputs = (np.asarray(flat, dtype=np.float32),) + tuple(np.asarray(x, dtype=np.float32) for x in (X_ic, X_bc, X_res))
    return cached_oracle(f"wsm_{case}_s{salt}", inputs, compute)


def _layout(case):
    ans, n, H, *_ = CASES[case]
    n_theta = int(pkg("circuits").params_per_layer(ans, n))
    lay = pkg("hip.engine").param_layout(H, n, n_theta)
    return lay, n_theta


def groups(case):
    """name -> (list of index lists, slice of the block whose maximum scales the tolerance): the columns one merged (or
    jointly reduced) wave sum writes, between which a wrong home-lane map would exchange totals."""
    ans, n, H, *_ = CASES[case]
    c = pkg("circuits")
    lay, n_theta = _layout(case)
    oW3, ob3, oW4 = (lay[k][0] for k in ("postprocessor.0.weight", "postprocessor.0.bias", "postprocessor.2.weight"))
    o_th, NP = lay["quantum_layer.params"][0], lay["__total__"][0]
    units = [[oW3 + m * n + i for i in range(n)] + [ob3 + m, oW4 + m] for m in range(H)]
    # the library forms its runs on a reordered gate list (gates on different wires commute); ALL diagonal gates of the
    # program as one group contains every run it can form
    gates = c.build_program(ans, n, 1, n >= 4).gates
    diag = sorted({o_th + g.slot for g in gates if g.op in (c.OP_RZ, c.OP_CRZ) and g.slot >= 0})
    return {"unit": (units, slice(oW3, o_th)), "diagonal run": ([diag] if len(diag) >= 2 else [], slice(o_th, NP))}


def distinct_margin(case, grad):
    """min over the groups of (smallest pairwise difference) / (100 x tolerance); > 1 is what (c) asks for"""
    worst = np.inf
    for name, (lists, block) in groups(case).items():
        tol = TOL_G * max(1.0, np.abs(grad[block]).max())
        for idx in lists:
            v = grad[idx]
            if len(v) >= 2:
                d = np.abs(v[:, None] - v[None, :])[np.triu_indices(len(v), 1)].min()
                worst = min(worst, d / (100.0 * tol))
    return worst


def test_cases_cover_the_shapes():
    ns, Hs, rs, vs = (set(x) for x in zip(*[(c[1], c[2], c[3], c[4] + c[5]) for c in CASES.values()]))
    assert ns == {2, 3, 4, 5} and Hs == {1, 3, 5, 13} and rs == {1, 63, 65} and vs == {1, 65}
    assert {(c[3], c[4] + c[5]) for c in CASES.values()} == {(r, v) for r in (1, 63, 65) for v in (1, 65)}
    assert any(c[0] == "layered" and c[1] == 4 for c in CASES.values())
    # the groups are what they are meant to be: N + 2 columns per unit; cascade has a diagonal run
    for case, c in CASES.items():
        g = groups(case)
        assert len(g["unit"][0]) == c[2] and all(len(u) == c[1] + 2 for u in g["unit"][0])
        if c[0] == "cascade":
            assert len(g["diagonal run"][0]) >= 1, case
    lens = {len(r) for c in CASES if CASES[c][1] == 4 for r in groups(c)["diagonal run"][0]}
    assert len(lens) >= 2, lens      # the layered program has another number of diagonal gates than cascade


@pytest.mark.parametrize("case", list(CASES))
def test_groups_are_pairwise_distinct(case):
    """(c), on the host from the reference alone"""
    ref = case_reference(case)
    m = distinct_margin(case, ref["grad"])
    print(f"\n{case}: smallest pairwise difference within a group = {m:.2f} x (100 x tolerance)")
    assert m > 1.0, m


@pytest.mark.gpu
def test_lane_exactness_program():
    assert os.path.exists(UBENCH), f"{UBENCH} is not built (csrc/Makefile builds it next to the library)"
    r = subprocess.run([UBENCH], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("NV=")]
    assert len(lines) == 16 and all(" PASS" in ln for ln in lines), r.stdout[-3000:]
    assert [int(ln[3:5]) for ln in lines] == list(range(1, 17))


def _check(name, got, ref, lay, n_theta, blocks):
    o_post, o_th, NP = lay["postprocessor.0.weight"][0], lay["quantum_layer.params"][0], lay["__total__"][0]
    sl = {"pre": slice(0, o_post), "post": slice(o_post, o_th), "theta": slice(o_th, NP)}
    errs = {}
    for b in blocks:
        want = ref["grad"][sl[b]]
        errs[b] = np.abs(got[sl[b]] - want).max() / (TOL_G * max(1.0, np.abs(want).max()))
    parts = ref["parts"]
    errs["losses"] = np.abs(got[NP:NP + 3] - parts).max() / (TOL_L * max(1.0, np.abs(parts).max()))
    print(f"{name}: error / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1.0, (name, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_stages_match_fp64(case, gpu_device):
    ans, n, H, B_res, n_ic, n_bc, salt = CASES[case]
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    ref = case_reference(case)
    lay, n_theta = _layout(case)
    flat, X_ic, X_bc, X_res = case_inputs(case)
    B_val = n_ic + n_bc
    torch.manual_seed(1)
    model = pkg("nn.DVPDESolver").DVPDESolver(
        base_args(num_qubits=n, num_quantum_layers=1, q_ansatz=ans, classic_network=[3, H, 1], encoding="angle"), Log(),
        device=gpu_device)
    eng = model._engine_for(gpu_device)
    with torch.no_grad():
        eng.flat.copy_(torch.from_numpy(np.asarray(flat, dtype=np.float32)))
    eng.refresh_gates()
    fs = engine.FusedStep(eng, B_res, n_ic, n_bc, engine.OptimState(eng.NP, 0.005, gpu_device))
    fs.X_res[:B_res] = X_res.to(gpu_device)
    fs.X_val[:n_ic] = X_ic.to(gpu_device)
    fs.X_val[n_ic:B_val] = X_bc.to(gpu_device)
    lib, d = eng.lib, fs.desc
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    NP, o_th = eng.NP, eng.theta_off
    assert NP == lay["__total__"][0] and o_th == lay["quantum_layer.params"][0]
    rows_res, rows_val = (B_res + 63) // 64, (B_val + 63) // 64

    # the fused step's five stages, one by one, on a poisoned row matrix
    fs.part.fill_(float("nan"))
    for stage in range(5):
        assert lib.qc_fused_step_stage(C.byref(d), stage, st) == 0, stage      # the merged form serves these sizes
    torch.cuda.synchronize()
    P = fs.part[:rows_res + rows_val].cpu().numpy().astype(np.float64)
    assert np.isfinite(P).all(), np.argwhere(~np.isfinite(P))[:4]
    print()
    _check(f"{case} merged stages", P.sum(axis=0), ref, lay, n_theta, ("pre", "post", "theta"))

    # the stand-alone post and adjoint calls on the same workspace (jets of the stages above), rows of their own
    f = dict(dtype=torch.float32, device=gpu_device)
    part2 = torch.full((rows_res + rows_val, fs.stride), float("nan"), **f)
    chi = torch.full((max(int(d.circ_ws_bytes), 4) // 4,), float("nan"), **f)
    qj = torch.full((6, n, B_res), float("nan"), **f)
    ab_res, ab_val = torch.full((6, n, B_res), float("nan"), **f), torch.full((n, max(B_val, 1)), float("nan"), **f)
    pde, th2 = C.byref(d.pde), part2.data_ptr() + 4 * o_th
    assert lib.qc_post(2, d.X_res_dev, d.params_dev, d.H, d.n, d.n_theta, pde, d.qjets_res_dev, d.abar_res_dev,
                       d.abar_res_dev + 4 * d.B_res, None, None, d.qbar_res_dev, part2.data_ptr(), fs.stride, 0, B_res, 6,
                       st) == 0
    assert lib.qc_post(2, d.X_val_dev, d.params_dev, d.H, d.n, d.n_theta, pde, d.qjets_val_dev, d.abar_val_dev, None, None,
                       None, d.qbar_val_dev, part2.data_ptr(), fs.stride, rows_res, B_val, 1, st) == 0
    assert lib.qc_forward_jets_keep(d.prog, d.trig_dev, d.umat_dev, d.ajets_res_dev, qj.data_ptr(), B_res, chi.data_ptr(),
                                    st) == 0
    assert lib.qc_backward_jets_kept(d.prog, d.trig_dev, d.umat_dev, d.ajets_res_dev, d.qbar_res_dev, ab_res.data_ptr(), th2,
                                     fs.stride, 0, B_res, chi.data_ptr(), st) == 0
    assert lib.qc_backward_expval(d.prog, d.trig_dev, d.umat_dev, d.ajets_val_dev, d.qbar_val_dev, ab_val.data_ptr(), th2,
                                  fs.stride, rows_res, B_val, None, 0, st) == 0
    torch.cuda.synchronize()
    o_post = lay["postprocessor.0.weight"][0]
    P2 = part2[:, o_post:].cpu().numpy().astype(np.float64)
    assert np.isfinite(P2).all(), np.argwhere(~np.isfinite(P2))[:4]
    got2 = np.concatenate([np.zeros(o_post), P2.sum(axis=0)])
    _check(f"{case} stand-alone qc_post + qc_backward_jets_kept", got2, ref, lay, n_theta, ("post", "theta"))
