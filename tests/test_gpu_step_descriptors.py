"""The records the step classes of hip/engine.py hand to the library, field by field, against
tests/golden/step_descriptors.json: one step of every kind (FusedStep analytic / tabulated / coefficient mode / adaptive
armed, CausalStep, SystemStep with and without residual targets, InverseStep, BalancedStep) at the smallest shapes that
reach every branch of the constructors: cascade n = 2, H = 3 (register family: the step workspace does not depend on free
memory), (B_res, n_ic, n_bc) = (128, 3, 5), (0, 3, 5) (the null ``coef_res_dev`` / ``target_res_dev`` branches) and
(128, 0, 0), history capacity 0 and 4, two time slabs.  No kernel of a step runs.

Per step: the bytes of every non-pointer field of ``QcStepDesc`` (``pde`` and ``hyper`` whole, so the NaN patterns of the
inverse step are pinned); per pointer field whether it is null and which tensor of the step it addresses; the same for the
side records (``data``, ``coef``, ``sys``, ``learn``, ``bal``, ``causal``, ``adapt``) after ``set_dataset`` and again
after ``set_dataset(None)``; and the name of the export the step calls.  The fixture was recorded on the GPU at the commit
BEFORE the step classes were put on one base class (tests/golden/make_step_descriptor_golden.py), so these tests say that
the refactor changed no byte the library reads.

Two assertions are newer than the fixture and fail on that earlier commit by design: every step binds its entry point
once (``_entry``, there only FusedStep's), and ``BalancedStep`` has no ``learn`` / ``coef_hist`` attribute (it used to
inherit and delete InverseStep's)."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN, pkg

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "step_descriptors.json")
N_QUBITS, HIDDEN, N_SLABS = 2, 3, 2
SHAPES = ((128, 3, 5), (0, 3, 5), (128, 0, 0))
HIST_CAPS = (0, 4)
DS_ROWS = (11, 4, 6)                    # residual, IC, BC rows of the resident dataset
SEED, OFFSETS = 0xFEDCBA9876543210, (7, 2, 3)
COEFFS, C_U = (1.0, 0.5, -0.25, 0.01, 0.02), 0.125
LOSS_WEIGHTS = (3.0, 5.0, 7.0)
SIDE_RECORDS = ("data", "coef", "sys", "learn", "bal", "causal", "adapt")
# kind -> (the export it calls, the records behind its arguments in order)
ENTRY = {"fused_analytic": ("qc_fused_pinn_residual_step", ("desc",)),
         "fused_tabulated": ("qc_fused_pinn_data_step", ("desc", "data")),
         "fused_coef": ("qc_fused_pinn_coef_step", ("desc", "data", "coef")),
         "fused_adaptive": ("qc_fused_pinn_adaptive_step", ("desc", "data", None, "adapt")),
         "causal": ("qc_fused_pinn_causal_step", ("desc", "data", "causal")),
         "system": ("qc_fused_pinn_system_step", ("desc", "sys")),
         "system_no_res_targets": ("qc_fused_pinn_system_step", ("desc", "sys")),
         "inverse": ("qc_fused_pinn_inverse_step", ("desc", "data", "learn")),
         "balanced": ("qc_fused_pinn_balanced_step", ("desc", "data", "bal"))}
KINDS = tuple(ENTRY)


def cases(kind):
    """The (B_res, n_ic, n_bc, hist_cap) the kind can be built at: the causal step needs B_res a positive multiple of
    64 * n_slabs, adaptive sampling a residual batch."""
    need_res = kind in ("causal", "fused_adaptive")
    return [(*s, h) for s in SHAPES for h in HIST_CAPS if s[0] or not need_res]


def _circuit(dev):
    circuits, engine = pkg("circuits"), pkg("hip.engine")
    return engine.Circuit(circuits.build_program("cascade", N_QUBITS, 1, False), None, dev)


def build(kind, circ, B_res, n_ic, n_bc, hist_cap):
    """(step, flat parameter vector, dataset tensors by name) of one kind, through the public constructors only."""
    L, engine = pkg("hip.lib"), pkg("hip.engine")
    dev = circ.device
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.rand(*shape, generator=g).to(dev)
    ds = {"ds_X_res": rnd(DS_ROWS[0], 3), "ds_X_ic": rnd(DS_ROWS[1], 3), "ds_X_bc": rnd(DS_ROWS[2], 3)}
    NP = engine.param_layout(HIDDEN, N_QUBITS, circ.n_params)["__total__"][0]
    kw = {}
    if kind.startswith("system"):
        K, n_eq = 2, 3
        NP = engine.param_layout(HIDDEN, N_QUBITS, circ.n_params, K)["__total__"][0]
        flat = rnd(NP)
        opt = engine.OptimState(NP, 0.005, dev, hist_cap=hist_cap, loss_weights=LOSS_WEIGHTS)
        terms = [(0, 0, 1, -1, -1, 1.0), (1, 1, 2, 0, -1, 0.5), (2, 0, 4, -1, -1, -0.25), (2, 1, 0, 0, 1, 2.0)]
        rec = L.system_record(K, n_eq, terms, (1.0, 0.5, 2.0), (1.0, 3.0))
        res_targets = kind == "system"
        fs = engine.SystemStep(circ, HIDDEN, flat, rec, B_res, n_ic, n_bc, opt, counts=(2 * B_res, 2 * n_ic, 2 * n_bc),
                               loss_weights=LOSS_WEIGHTS, res_targets=res_targets)
        ds.update(ds_r=rnd(DS_ROWS[0], n_eq) if res_targets else None, ds_u_ic=rnd(DS_ROWS[1], K), ds_u_bc=rnd(DS_ROWS[2], K))
    elif kind in ("inverse", "balanced"):
        n_own = L.QC_COEF_COLS if kind == "inverse" else L.QC_BAL_TERMS
        flat = rnd(NP + n_own)
        opt = engine.OptimState(NP + n_own, 0.005, dev, hist_cap=hist_cap, loss_weights=LOSS_WEIGHTS)
        counts = (2 * B_res, 2 * n_ic, 2 * n_bc)
        if kind == "inverse":
            fs = engine.InverseStep(circ, HIDDEN, flat, [0.1 * k for k in range(7)], [1.0, 0.0, 0.5, 2.0, 0.01, 0.02, 0.0],
                                    B_res, n_ic, n_bc, opt, counts=counts, loss_weights=LOSS_WEIGHTS)
        else:
            fs = engine.BalancedStep(circ, HIDDEN, flat, [1.0, 0.0, 0.5], B_res, n_ic, n_bc, opt, COEFFS, C_U, counts=counts,
                                     loss_weights=LOSS_WEIGHTS)
        ds.update(ds_r=rnd(DS_ROWS[0]), ds_u_ic=rnd(DS_ROWS[1]), ds_u_bc=rnd(DS_ROWS[2]))
    else:
        flat = rnd(NP)
        eng = engine.SolverEngine(circ, HIDDEN, flat, D=0.02, vx=0.75, vy=1.25)
        eng.loss_weights = LOSS_WEIGHTS
        if kind != "fused_analytic":
            eng.problem, eng.coeffs, eng.c_u = L.QC_PROBLEM_TABULATED, COEFFS, C_U
        eng.coef_mode = kind == "fused_coef"
        opt = engine.OptimState(NP, 0.005, dev, hist_cap=hist_cap, loss_weights=LOSS_WEIGHTS)
        counts = (2 * B_res, 2 * n_ic, 2 * n_bc)
        if kind == "causal":
            fs = engine.CausalStep(eng, B_res, n_ic, n_bc, opt, N_SLABS, 0.5, 2.0, 8.0, 0.99, capacity=hist_cap, counts=counts)
        else:
            fs = engine.FusedStep(eng, B_res, n_ic, n_bc, opt, counts)
        ds.update(ds_r=rnd(DS_ROWS[0]), ds_u_ic=rnd(DS_ROWS[1]), ds_u_bc=rnd(DS_ROWS[2]))
        if kind == "fused_coef":
            ds["ds_coef"] = rnd(DS_ROWS[0], L.QC_COEF_COLS)
        kw = {"bc_face_points": 9}
    fs.set_sampler(SEED, *OFFSETS, **kw)
    return fs, flat, ds


def set_dataset(kind, fs, ds):
    """``set_dataset`` (``ds`` None: removes it), with what follows it in the trainers: slab offsets, adaptive arming."""
    if ds is None:
        if kind == "fused_adaptive":        # an armed CDF belongs to residual rows: cleared before they go
            fs.clear_adaptive()
        fs.set_dataset(None)
        if kind == "causal":
            fs.set_slabs(None)
        return
    seg = ((ds["ds_X_res"], ds["ds_r"]), (ds["ds_X_ic"], ds["ds_u_ic"]), (ds["ds_X_bc"], ds["ds_u_bc"]))
    if kind == "fused_coef":
        fs.set_dataset(seg, ds["ds_coef"])
    else:
        fs.set_dataset(seg)
    if kind == "causal":
        fs.set_slabs([0, 5, DS_ROWS[0]])
    if kind == "fused_adaptive":
        fs.set_adaptive(2, 0.5)


def _tensors(fs, circ, flat, ds):
    """name -> address of every tensor a record of the step may point at."""
    opt = fs.opt
    out = {"circuit.handle": circ.handle.value, "circuit.trig": circ.trig.data_ptr(), "flat": flat.data_ptr(),
           "opt.m": opt.m.data_ptr(), "opt.v": opt.v.data_ptr(), "opt.state": opt.state.data_ptr(),
           "opt.hist": opt.hist.data_ptr()}
    for i in range(4):
        out[f"ws_res[{i}]"], out[f"ws_val[{i}]"] = fs.ws_res[i].data_ptr(), fs.ws_val[i].data_ptr()
    for name in ("X_res", "X_val", "target_res", "target_val", "coef_res", "part", "flat_grad", "step_ws", "adapt_buf",
                 "coef_hist", "weight_hist", "state", "causal_hist", "slab_lo"):
        t = getattr(fs, name, None)
        if t is not None:
            out[name] = t.data_ptr()
    out.update({k: t.data_ptr() for k, t in ds.items() if t is not None})
    assert len(set(out.values())) == len(out), "two tensors of a step share an address"
    return out


def _record(rec, names):
    """field -> hex of its bytes, or for a pointer "null" / the name of the tensor it addresses."""
    raw, by_addr, out = bytes(rec), {v: k for k, v in names.items()}, {}
    for name, ctype in rec._fields_:
        if ctype is C.c_void_p:
            v = getattr(rec, name)
            out[name] = "null" if v is None else "-> " + by_addr.get(v, "UNKNOWN")
        else:
            f = getattr(type(rec), name)
            out[name] = raw[f.offset:f.offset + f.size].hex()
    return out


def _sides(fs, names):
    return {r: _record(getattr(fs, r), names) for r in SIDE_RECORDS if getattr(fs, r, None) is not None}


def describe(kind, circ, B_res, n_ic, n_bc, hist_cap):
    """What the fixture holds for one step; the generator and the tests both call this."""
    fs, flat, ds = build(kind, circ, B_res, n_ic, n_bc, hist_cap)
    set_dataset(kind, fs, ds)
    names = _tensors(fs, circ, flat, ds)
    out = {"desc": _record(fs.desc, names), "with_dataset": _sides(fs, names),
           "kept_alive": len(fs._dataset), "stride": fs.stride, "part": list(fs.part.shape),
           "step_ws": fs.step_ws.numel(), "entry": fs._entry[0] if hasattr(fs, "_entry") else ENTRY[kind][0]}
    set_dataset(kind, fs, None)
    out["without_dataset"] = _sides(fs, _tensors(fs, circ, flat, {}))
    out["entry_without_dataset"] = fs._entry[0] if hasattr(fs, "_entry") else ENTRY[kind][0]
    return out, fs


def key(kind, B_res, n_ic, n_bc, hist_cap):
    return f"{kind} B_res={B_res} n_ic={n_ic} n_bc={n_bc} hist_cap={hist_cap}"


@pytest.fixture(scope="module")
def circuit(gpu_device):
    return _circuit(gpu_device)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("kind", KINDS)
def test_records_match_the_recorded_ones(kind, circuit, golden):
    for case in cases(kind):
        got, _ = describe(kind, circuit, *case)
        want = golden[key(kind, *case)]
        for part in want:
            assert got[part] == want[part], (key(kind, *case), part)
        assert "UNKNOWN" not in json.dumps(got)


@pytest.mark.parametrize("kind", KINDS)
def test_entry_is_bound_once_to_the_steps_own_records(kind, circuit):
    """``run`` builds no ``byref`` per call: the entry holds them, and each refers to the record the step exposes."""
    B_res, n_ic, n_bc, hist_cap = cases(kind)[0]
    fs, flat, ds = build(kind, circuit, B_res, n_ic, n_bc, hist_cap)
    set_dataset(kind, fs, ds)
    name, fn, args = fs._entry
    want_name, want_args = ENTRY[kind]
    assert name == want_name and fn is getattr(pkg("hip.lib").load(), want_name)
    assert len(args) == len(want_args)
    for a, rec in zip(args, want_args):
        assert (a is None) if rec is None else (a._obj is getattr(fs, rec)), (kind, rec)


def test_balanced_step_has_no_operator_record(circuit):
    """Fails before the step classes shared a base: BalancedStep then inherited InverseStep's record and deleted it."""
    engine = pkg("hip.engine")
    fs, _, _ = build("balanced", circuit, 128, 3, 5, 4)
    assert not hasattr(fs, "learn") and not hasattr(fs, "coef_hist")
    assert not issubclass(engine.BalancedStep, engine.InverseStep)
    assert fs.NP_L == fs.NP_B == fs.NP + engine.BalancedStep.N_OWN and hasattr(fs, "weight_hist")
    inv, _, _ = build("inverse", circuit, 128, 3, 5, 4)
    assert hasattr(inv, "learn") and tuple(inv.coef_hist.shape) == (4, pkg("hip.lib").QC_COEF_COLS)
