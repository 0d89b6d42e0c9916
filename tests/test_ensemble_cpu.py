"""The ensemble step without a GPU: every refusal of qc_fused_pinn_ensemble_step returns its code before any launch (the
descriptors are those of tests/step_refusal_cases.py: made-up addresses that nothing dereferences, phases = 0 unless the
fault is one of a phase), the stride helper, and the EnsembleTrainer's member checks, stacking and write-back with the step
replaced by a stub."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_refusal_cases as S
from conftest import pkg
from test_gpu_fullsize import Log, base_args

M = 3


class Call(S.Call):
    """A valid ensemble call: the analytic descriptor of the refusal table with a workspace slice, and the smallest
    strides for M members."""

    def __init__(self, lib):
        super().__init__(lib, "residual")
        L = pkg("hip.lib")
        self.d.prog = C.addressof(self.prog)
        self.d.hist_dev, self.d.hist_cap = S.fake(50), 10
        self.d.circ_ws_dev = S.fake(51)
        self.d.circ_ws_bytes = lib.qc_step_workspace_bytes(C.byref(self.prog), S.B_RES, S.N_IC + S.N_BC)
        self.ens = L.QcStepEnsemble()
        assert lib.qc_ensemble_strides(C.byref(self.d), M, C.byref(self.ens)) == S.OK
        self.null_ens = False

    def restride(self):
        """the strides again, after a fault replaced the program or a batch size"""
        self.d.prog = C.addressof(self.prog)
        tables = self.ens.pde_dev, self.ens.hyper_dev
        self.lib.qc_ensemble_strides(C.byref(self.d), M, C.byref(self.ens))
        self.ens.pde_dev, self.ens.hyper_dev = tables

    def run(self) -> int:
        self.d.prog = C.addressof(self.prog) if self.prog is not None else None
        return self.lib.qc_fused_pinn_ensemble_step(None if "d" in self.null else C.byref(self.d),
                                                    None if self.null_ens else C.byref(self.ens), self.phases, None)


def _ens(**fields):
    def f(c):
        for k, v in fields.items():
            setattr(c.ens, k, v(getattr(c.ens, k)) if callable(v) else v)
    return f


def _then_restride(fault):
    def f(c):
        fault(c)
        c.restride()
    return f


def _null_ens(c):
    c.null_ens = True


short = lambda v: v - 1
ARG = {
    "null_desc": S.FAULTS["null_desc"], "null_ens": _null_ens, "comm": S.FAULTS["comm"],
    "M_zero": _ens(M=0), "M_negative": _ens(M=-1), "M_above_grid": _ens(M=65536),
    "params_stride_short": _ens(params_stride=short), "flat_stride_short": _ens(flat_stride=short),
    "hist_stride_short": _ens(hist_stride=short), "trig_stride_short": _ens(trig_stride=lambda v: v - 256),
    "trig_stride_unaligned": _ens(trig_stride=lambda v: v + 16), "x_res_stride_short": _ens(x_res_stride=short),
    "x_val_stride_short": _ens(x_val_stride=short), "jets_res_stride_short": _ens(jets_res_stride=short),
    "jets_val_stride_short": _ens(jets_val_stride=short), "ws_stride_short": _ens(ws_stride=lambda v: v - 256),
    "ws_stride_unaligned": _ens(ws_stride=lambda v: v + 4), "pde_table_misaligned": _ens(pde_dev=S.fake(52) + 4),
    "hyper_table_misaligned": _ens(hyper_dev=S.fake(53) + 2),
    "null_prog": S.FAULTS["null_prog"], "null_trig": S.FAULTS["null_trig"], "null_params": S.FAULTS["null_params"],
    "null_part": S.FAULTS["null_part"], "null_flat": S.FAULTS["null_flat"],
    **{"null_" + k: S._set(**{k + "_dev": None}) for k in (
        "X_res", "X_val", "ajets_res", "qjets_res", "qbar_res", "abar_res", "ajets_val", "qjets_val", "qbar_val", "abar_val",
        "circ_ws")},
    "ws_slice_too_small": lambda c: S._set(circ_ws_bytes=c.d.circ_ws_bytes - 1)(c),
    "no_residual_points": _then_restride(S._set(B_res=0)), "no_value_points": _then_restride(S._set(B_val=0, n_ic=0)),
    "n_ic_above_B_val": S._set(n_ic=S.N_IC + S.N_BC + 1),
    "n_mismatch": S.FAULTS["n_mismatch"], "n_theta_mismatch": S.FAULTS["n_theta_mismatch"], "H_zero": S.FAULTS["H_zero"],
    "stride_one_short": S.FAULTS["stride_one_short"], "rows_cap_one_short": S.FAULTS["rows_cap_one_short"],
    "problem_tabulated": S.FAULTS["problem_tabulated"], "problem_out_of_range": S.FAULTS["problem_out_of_range"],
    "problem_negative": S.FAULTS["problem_negative"], "face_rule_below_random": S.FAULTS["face_rule_below_random"],
    "u4_without_umat": _then_restride(S.FAULTS["u4_without_umat"]),
    "update_null_m": S.FAULTS["update_null_m"], "update_null_v": S.FAULTS["update_null_v"],
    "update_null_opt_state": S.FAULTS["update_null_opt_state"],
    "sample_null_X_val": S.FAULTS["sample_null_X_val"],
}
UNSUPPORTED = {
    "wave_family": _then_restride(S.FAULTS["n6"]),
    "hbm_family": S._prog(n=9, n_params=9, fam="hbm"),      # (a mirror without the family's plan: sized by nobody)
    "no_family": _then_restride(S.FAULTS["no_family"]),
    "amplitude": S.FAULTS["amplitude"],
    "input_map": S.FAULTS["input_map"],
    "embed_program": _then_restride(S.FAULTS["embed_program"]),
    "H_above_fused_post": _then_restride(S._set(H=129)),
    "H_too_large": _then_restride(S.FAULTS["H_too_large"]),
}
# two faults: the first check decides
PAIRS = [(("comm", "amplitude"), S.ERR_ARG), (("wave_family", "M_zero"), S.ERR_ARG), (("null_part", "embed_program"), S.ERR_ARG),
         (("problem_tabulated", "input_map"), S.ERR_ARG), (("amplitude", "params_stride_short"), S.ERR_UNSUPPORTED),
         (("embed_program", "null_X_res"), S.ERR_UNSUPPORTED)]


@pytest.fixture(scope="module")
def lib():
    return pkg("hip.lib").load()


def test_the_baseline_passes_validation(lib):
    S.check_program_mirror(lib)
    assert Call(lib).run() == S.OK            # phases = 0: validated, nothing to do


@pytest.mark.parametrize("fault", list(ARG))
def test_argument_refusals(fault, lib):
    c = Call(lib)
    ARG[fault](c)
    assert c.run() == S.ERR_ARG


@pytest.mark.parametrize("fault", list(UNSUPPORTED))
def test_unsupported_refusals(fault, lib):
    c = Call(lib)
    UNSUPPORTED[fault](c)
    assert c.run() == S.ERR_UNSUPPORTED


@pytest.mark.parametrize("faults,code", PAIRS, ids=["+".join(p[0]) for p in PAIRS])
def test_the_first_check_decides(faults, code, lib):
    c = Call(lib)
    for f in faults:
        {**ARG, **UNSUPPORTED}[f](c)
    assert c.run() == code


def test_stride_helper(lib):
    L = pkg("hip.lib")
    c = Call(lib)
    e, d = c.ens, c.d
    NP = pkg("hip.engine").param_layout(S.H, S.N, S.N_THETA)["__total__"][0]
    B_val = S.N_IC + S.N_BC
    assert (e.M, e.params_stride, e.flat_stride, e.hist_stride) == (M, NP, NP + 3, 10)
    assert (e.x_res_stride, e.x_val_stride, e.jets_res_stride, e.jets_val_stride) == (3 * S.B_RES, 3 * B_val, 6 * S.N * S.B_RES,
                                                                                     S.N * B_val)
    trig, ws = lib.qc_trig_bytes(C.byref(c.prog)), lib.qc_step_workspace_bytes(C.byref(c.prog), S.B_RES, B_val)
    assert e.trig_stride % 256 == 0 and trig <= e.trig_stride < trig + 256
    assert e.ws_stride % 256 == 0 and ws <= e.ws_stride < ws + 256
    assert e.pde_dev is None and e.hyper_dev is None
    out = L.QcStepEnsemble()
    assert lib.qc_ensemble_strides(None, M, C.byref(out)) == S.ERR_ARG
    assert lib.qc_ensemble_strides(C.byref(d), M, None) == S.ERR_ARG
    assert lib.qc_ensemble_strides(C.byref(d), 0, C.byref(out)) == S.ERR_ARG
    d.prog = None
    assert lib.qc_ensemble_strides(C.byref(d), M, C.byref(out)) == S.ERR_ARG


# ---------------------------------------------------------------- the trainer, with the step stubbed
def _models(k=3, **kw):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    out = []
    for m in range(k):
        torch.manual_seed(10 + m)
        out.append(Solver(base_args(lr=0.001 * (m + 1), **kw), Log(), device="cpu"))
    return out


class StubStep:
    """What EnsembleTrainer asks of its step, on CPU tensors: stacked parameters (five unused floats behind every row)
    and the members' optimiser states."""

    def __init__(self, circuit, hidden, flats, opts, pdes, B_res, n_ic, n_bc):
        self.NP, self.opts, self.pdes, self.hidden = flats[0].numel(), opts, pdes, hidden
        self.params = torch.full((len(flats), self.NP + 5), -7.0)
        for m, x in enumerate(flats):
            self.params[m, : self.NP] = x
        self.seed = None

    def refresh_gates(self):
        pass

    def set_sampler(self, seed):
        self.seed = seed

    def member(self, m):
        return self.opts[m]

    def read(self, m):
        return self.opts[m].read()

    def loss_history(self, m, steps=None):
        return self.opts[m].loss_history(steps)


def test_trainer_refuses_members_that_cannot_share_a_step():
    ET = pkg("trainer.ensemble_train")
    a = _models(1)[0]
    for other in (dict(classic_network=[3, 40, 1]), dict(num_qubits=3), dict(q_ansatz="farhi"), dict(num_quantum_layers=2),
                  dict(classic_network=[3, 50, 2]), dict(fourier_features=4)):
        with pytest.raises(ValueError):
            ET.check_members([a, _models(1, **other)[0]])
    with pytest.raises(ValueError):
        ET.check_members([])
    with pytest.raises(ValueError):
        ET.check_members([a, torch.nn.Linear(3, 1)])
    # the fixed two-wire unitaries come from args["seed"]: members of an ansatz that applies them must share it
    b = _models(1, seed=5)[0]
    if a.quantum_layer.program.use_haar:
        with pytest.raises(ValueError):
            ET.check_members([a, b])
    else:
        ET.check_members([a, b])
    ET.check_members(_models(3))
    with pytest.raises(ValueError):
        ET.EnsembleTrainer(_models(2), 64, 4, loss_weights=[(1, 1, 1)] * 3, step_factory=StubStep)
    with pytest.raises(ValueError):
        ET.EnsembleTrainer(_models(2), 64, 4, pde=[dict(D=0.01, vx=1, vy=1, problem=0), dict(D=0.01, vx=1, vy=1, problem=1)],
                           step_factory=StubStep)


def test_stacking_and_write_back_round_trip_the_flat_layout():
    ET = pkg("trainer.ensemble_train")
    engine = pkg("hip.engine")
    models = _models(3)
    before = [{k: v.clone() for k, v in m.state_dict().items()} for m in models]
    tr = ET.EnsembleTrainer(models, 64, capacity=4, loss_weights=[None, (1.0, 10.0, 1.0), None],
                            pde=[None, None, dict(D=0.05, vx=1.0, vy=1.0)], step_factory=StubStep)
    fs = tr.fs
    n, H = models[0].num_qubits, models[0].hidden_width
    lay = engine.param_layout(H, n, models[0].quantum_layer.params.numel())
    assert fs.NP == lay["__total__"][0] and fs.hidden == H and isinstance(fs.seed, int)
    # stacking: row m is model m's parameters in param_layout order, exactly
    for m, sd in enumerate(before):
        for name, (off, shape) in lay.items():
            if name != "__total__":
                assert torch.equal(fs.params[m, off:off + int(np.prod(shape))], sd[name].reshape(-1)), (m, name)
    # the per-member records: learning rates, loss weights and operator constants
    assert [round(fs.read(m)["lr"], 6) for m in range(3)] == [0.001, 0.002, 0.003]
    assert [(o.hyper.w_res, o.hyper.w_bc, o.hyper.w_ic) for o in fs.opts] == [(2.0, 4.0, 2.0), (1.0, 10.0, 1.0), (2.0, 4.0, 2.0)]
    assert [round(p.D, 6) for p in fs.pdes] == [0.01, 0.01, 0.05] and round(fs.pdes[2].d_xx, 6) == 0.05
    assert fs.pdes[1].w_res == pytest.approx(2.0 * 1.0 / 64) and fs.pdes[1].w_val_b == pytest.approx(2.0 * 10.0 / 21)
    # write-back without a step: bit for bit what went in
    tr.sync_to_torch()
    for m, sd in enumerate(before):
        for name, v in models[m].state_dict().items():
            assert torch.equal(v, sd[name]), (m, name)
    # write-back of new values: every named parameter receives its own slice of its own row, nothing of the padding
    for m in range(3):
        fs.params[m, : fs.NP] = torch.arange(fs.NP, dtype=torch.float32) + 1000.0 * m
        fs.opts[m].m[:] = 0.5 + m
        fs.opts[m].write(lr=0.01 * (m + 1), step=7, num_bad=2, best=0.25)
    tr.sync_to_torch()
    for m, model in enumerate(models):
        sd = model.state_dict()
        for name, (off, shape) in lay.items():
            if name != "__total__":
                want = torch.arange(off, off + int(np.prod(shape)), dtype=torch.float32) + 1000.0 * m
                assert torch.equal(sd[name].reshape(-1), want), (m, name)
        assert model.optimizer.param_groups[0]["lr"] == pytest.approx(0.01 * (m + 1))
        st = model.optimizer.state[next(iter(model.parameters()))]
        assert float(st["step"]) == 7 and torch.all(st["exp_avg"] == 0.5 + m)
        assert model.scheduler.num_bad_epochs == 2 and model.scheduler.best == pytest.approx(0.25)
