"""The system step without a GPU: the three new exports, the ctypes mirrors against the header's layout, every argument
refusal of include/qcpinn_hip.h, TabulatedSystem / SystemTrainer ValueErrors, navier_stokes_2D_terms against the formulas
of nn.pde.navier_stokes_2D_operator, param_layout(K) against model.parameters(), and that the float64 references of the
seeded GPU cases (tests/system_reference.py) are not vacuous: every gradient block is well above the tolerance and every
negative control differs from the true reference by more than ten times it."""
import ctypes as C

import numpy as np
import pytest
import torch

import system_reference as S
from conftest import pkg
from test_tabulated_cpu import _desc

TOL_G, TOL_L = 2e-4, 1e-4
THETA_MIN = 20 * TOL_G
FAKE = 4096


# ---- 1. ABI
def test_exports_load_and_records_match_the_header_layout():
    L = pkg("hip.lib")
    lib = L.load()
    for name in ("qc_post_system", "qc_sample_dataset_system", "qc_fused_pinn_system_step"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert (L.QC_KMAX, L.QC_EQMAX, L.QC_TERMS_MAX) == (4, 4, 32)
    assert C.sizeof(L.QcSysTerm) == 24 and L.QcSysTerm.coef.offset == 20
    # three ints, 32 terms, 4 + 4 floats, padded to 8; two pointers; three (pointer, pointer, int64) triples
    head = 12 + 32 * 24 + 32
    assert L.QcStepSystem.terms.offset == 12 and L.QcStepSystem.w_eq.offset == 12 + 32 * 24 and L.QcStepSystem.w_out.offset == head - 16
    assert L.QcStepSystem.target_res_dev.offset == (head + 7) // 8 * 8 == 816
    assert L.QcStepSystem.ds_X_res.offset == 832 and L.QcStepSystem.ds_n_bc.offset == 896
    assert C.sizeof(L.QcStepSystem) == 904
    assert lib.qc_version() == 4


def _sys(L, K=3, n_eq=3, terms=None, w_eq=S.W_EQ, w_out=S.W_OUT, ds=(10, 10, 10)):
    s = L.system_record(K, n_eq, S.ns_terms() if terms is None else terms, w_eq, w_out)
    s.target_res_dev = s.target_val_dev = FAKE
    for name, n in zip(("res", "ic", "bc"), ds):
        setattr(s, "ds_X_" + name, FAKE)
        setattr(s, {"res": "ds_r", "ic": "ds_u_ic", "bc": "ds_u_bc"}[name], FAKE)
        setattr(s, "ds_n_" + name, n)
    return s


def _bad_systems(L):
    """(what, record) of every refusal of the operator itself."""
    nan, inf = float("nan"), float("inf")
    t0 = S.ns_terms()
    mod = lambda i, **kw: [tuple(kw.get(f, v) for f, v in zip(("eq", "out", "chan", "mul0", "mul1", "coef"), t)) if j == i else t
                           for j, t in enumerate(t0)]
    out = [("K = 0", _sys(L, K=0)), ("K = 5", _sys(L, K=5)), ("n_eq = 0", _sys(L, n_eq=0)), ("n_eq = 5", _sys(L, n_eq=5)),
           ("n_terms = 0", _sys(L, terms=[])), ("eq = n_eq", _sys(L, terms=mod(3, eq=3))), ("eq < 0", _sys(L, terms=mod(3, eq=-1))),
           ("out = K", _sys(L, terms=mod(0, out=3))), ("out < 0", _sys(L, terms=mod(0, out=-1))),
           ("chan = 6", _sys(L, terms=mod(5, chan=6))), ("chan < 0", _sys(L, terms=mod(5, chan=-1))),
           ("mul0 = K", _sys(L, terms=mod(3, mul0=3))), ("mul0 = -2", _sys(L, terms=mod(3, mul0=-2))),
           ("mul1 = K", _sys(L, terms=mod(13, mul1=3))), ("mul1 = -2", _sys(L, terms=mod(13, mul1=-2))),
           ("coef nan", _sys(L, terms=mod(7, coef=nan))), ("coef inf", _sys(L, terms=mod(7, coef=inf))),
           ("w_eq nan", _sys(L, w_eq=(1.0, nan, 1.0))), ("w_eq inf", _sys(L, w_eq=(1.0, 1.0, -inf))),
           ("w_out nan", _sys(L, w_out=(nan, 1.0, 1.0))), ("w_out inf", _sys(L, w_out=(1.0, 1.0, inf)))]
    s = _sys(L)
    s.n_terms = 33
    return out + [("n_terms = 33", s)]


def test_argument_errors_do_not_need_a_gpu():
    L = pkg("hip.lib")
    lib = L.load()
    pde = L.QcPde()
    good = _sys(L)
    stride = 10 ** 4
    post = lambda s, prm=FAKE, q=FAKE, tg=FAKE, qbar=FAKE, part=FAKE, stride=stride, row0=0, B=64, nch=6, pde=pde: \
        lib.qc_post_system(prm, 50, 4, 12, None if s is None else C.byref(s), None if pde is None else C.byref(pde), q, tg, qbar,
                           part, stride, row0, B, nch, None)
    # qc_post_system: the operator, then its buffers and the row width NP_K + 3
    assert post(None) == -1
    for what, s in _bad_systems(L):
        assert post(s) == -1, what
    NP3 = pkg("hip.engine").param_layout(50, 4, 12, 3)["__total__"][0]
    assert NP3 == pkg("hip.engine").param_layout(50, 4, 12)["__total__"][0] + 2 * 51
    for kw in (dict(prm=None), dict(q=None), dict(qbar=None), dict(part=None), dict(pde=None), dict(row0=-1), dict(B=0),
               dict(nch=3), dict(nch=1, tg=None), dict(stride=NP3 + 2)):
        assert post(good, **kw) == -1, kw
    # qc_sample_dataset_system: absent record, widths out of range, missing buffers, absent / empty / oversized segments
    call = lambda s, Xr=FAKE, tr=FAKE, Xv=FAKE, tv=FAKE, n=(5, 3, 2): lib.qc_sample_dataset_system(
        Xr, tr, n[0], 0, Xv, tv, n[1], 0, n[2], 0, None if s is None else C.byref(s), 1, 1, None)
    assert call(None) == -1 and call(_sys(L, K=5)) == -1 and call(_sys(L, n_eq=0)) == -1
    assert call(good, tv=None) == -1 and call(good, Xr=None) == -1 and call(good, Xv=None) == -1
    for field, bad in (("ds_n_res", 0), ("ds_n_ic", 0), ("ds_n_bc", 0), ("ds_n_res", 2 ** 31), ("ds_n_bc", 2 ** 31),
                       ("ds_X_ic", None), ("ds_X_res", None), ("ds_u_ic", None), ("ds_u_bc", None)):
        s = _sys(L)
        setattr(s, field, bad)
        assert call(s) == -1, field
    # qc_fused_pinn_system_step.  The entry checks the system, its targets, the dataset (under QC_PHASE_SAMPLE) and the row
    # width before it looks at the program; a program needs a device, so the descriptor's is null and a call that passed
    # these checks would be refused all the same: tests/test_gpu_system.py::test_refusals_name_one_fault_each repeats them
    # on a descriptor that runs but for the one fault named.
    d = _desc(L, L.QC_PROBLEM_TABULATED, 5, 3, 2)
    both = L.QC_PHASE_GRADS | L.QC_PHASE_SAMPLE
    step = lambda s, phases=L.QC_PHASE_GRADS: lib.qc_fused_pinn_system_step(C.byref(d), None if s is None else C.byref(s), phases, None)
    assert step(None) == -1 and lib.qc_fused_pinn_system_step(None, C.byref(good), L.QC_PHASE_GRADS, None) == -1
    for what, s in _bad_systems(L):
        assert step(s) == -1, what
    s = _sys(L)
    s.target_val_dev = None
    assert step(s) == -1
    for field, bad in (("ds_n_res", 0), ("ds_X_bc", None), ("ds_n_ic", 2 ** 31), ("ds_u_ic", None)):
        s = _sys(L)
        setattr(s, field, bad)
        assert step(s, both) == -1, field
    d.part_stride = NP3 + 2
    assert step(good) == -1


# ---- 2. TabulatedSystem / SystemTrainer
def _segments(n=(5, 3, 2), K=3, n_eq=3):
    g = torch.Generator().manual_seed(0)
    X = [torch.rand(m, 3, generator=g) for m in n]
    return X, torch.rand(n[0], n_eq, generator=g), torch.rand(n[1], K, generator=g), torch.rand(n[2], K, generator=g)


def test_tabulated_system_validates_its_segments_and_terms():
    TS = pkg("data.tabulated").TabulatedSystem
    terms = pkg("nn.pde").navier_stokes_2D_terms()
    (Xr, Xi, Xb), Rr, Ui, Ub = _segments()
    p = TS((Xr, Rr), (Xi, Ui), (Xb, Ub), terms, eq_weights=(1, 2, 3), out_weights=(1, 1, 0))
    assert (p.K, p.n_eq, p.sizes()) == (3, 3, (5, 3, 2)) and len(p.terms) == 14 and p.to("cpu") is p
    assert TS((Xr, None), (Xi, Ui), (Xb, Ub), terms).R is None
    assert TS((Xr, None), (Xi, Ui), (Xb, Ub), terms).n_eq == 3 and p.eq_weights == (1.0, 2.0, 3.0)
    with pytest.raises(ValueError, match=r"shape \(N, 3\)"):
        TS((Xr[:, :2], Rr), (Xi, Ui), (Xb, Ub), terms)
    with pytest.raises(ValueError, match="float32"):
        TS((Xr, Rr.double()), (Xi, Ui), (Xb, Ub), terms)
    with pytest.raises(ValueError, match="5 points but 3 target rows"):
        TS((Xr, Rr[:3]), (Xi, Ui), (Xb, Ub), terms)
    with pytest.raises(ValueError, match=r"targets must have shape \(N, 3\)"):
        TS((Xr, Rr), (Xi, Ui), (Xb, Ub[:, :2]), terms)
    with pytest.raises(ValueError, match="1 <= K <= 4"):
        TS((Xr, Rr), (Xi, torch.rand(3, 5)), (Xb, torch.rand(2, 5)), terms)
    with pytest.raises(ValueError, match="targets are required"):
        TS((Xr, Rr), (Xi, Ui), (Xb, None), terms)
    with pytest.raises(ValueError, match="1..32 terms"):
        TS((Xr, Rr), (Xi, Ui), (Xb, Ub), terms * 3)
    with pytest.raises(ValueError, match="equation 3 outside"):
        TS((Xr, Rr), (Xi, Ui), (Xb, Ub), terms + [(3, 0, 0, -1, -1, 1.0)])
    with pytest.raises(ValueError, match="channel 6"):
        TS((Xr, Rr), (Xi, Ui), (Xb, Ub), [(0, 0, 6, -1, -1, 1.0)])
    with pytest.raises(ValueError, match="multipliers"):
        TS((Xr, Rr), (Xi, Ui), (Xb, Ub), [(0, 0, 0, 3, -1, 1.0)])
    with pytest.raises(ValueError, match="not finite"):
        TS((Xr, Rr), (Xi, Ui), (Xb, Ub), [(0, 0, 0, -1, -1, float("nan"))])
    with pytest.raises(ValueError, match="3 / 3 entries"):
        TS((Xr, Rr), (Xi, Ui), (Xb, Ub), terms, eq_weights=(1, 2))
    with pytest.raises(ValueError, match="finite"):
        TS((Xr, Rr), (Xi, Ui), (Xb, Ub), terms, out_weights=(1, float("inf"), 0))


class _Log:
    def print(self, *a): pass
    def get_output_dir(self): return "."


def _args(network):
    return {"batch_size": 64, "epochs": 1, "lr": 0.005, "seed": 1, "print_every": 10 ** 9, "num_qubits": 4,
            "num_quantum_layers": 1, "classic_network": network, "q_ansatz": "cascade", "shots": 1024, "problem": "diffusion",
            "solver": "DV", "encoding": "None", "use_ibm_hardware": False}


def test_system_trainer_argument_errors():
    ST = pkg("trainer.system_train").SystemTrainer
    TS = pkg("data.tabulated").TabulatedSystem
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    terms = pkg("nn.pde").navier_stokes_2D_terms()
    (Xr, Xi, Xb), Rr, Ui, Ub = _segments()
    ds = TS((Xr, Rr), (Xi, Ui), (Xb, Ub), terms)
    m3 = Solver(_args([3, 8, 3]), _Log(), device="cpu")
    with pytest.raises(ValueError, match="TabulatedSystem"):
        ST(m3, 64, dataset=None)
    with pytest.raises(ValueError, match="two-input"):
        ST(Solver(_args([2, 8, 3]), _Log(), device="cpu"), 64, dataset=ds)
    with pytest.raises(ValueError, match="1 outputs but the dataset prescribes 3"):
        ST(Solver(_args([3, 8, 1]), _Log(), device="cpu"), 64, dataset=ds)
    with pytest.raises(ValueError, match="sampler"):
        ST(m3, 64, dataset=ds, sampler="numpy")
    # the existing refusals stay: FusedTrainer on n_out != 1, residual() on a K-output model
    with pytest.raises(ValueError, match=r"\[3, H, 1\]"):
        pkg("trainer.diffusion_train").FusedTrainer(m3, 64, 1)
    with pytest.raises(NotImplementedError):
        m3._engine_for(torch.device("cuda", 0))


# ---- 3. the Navier-Stokes term list is the operator's formulas
def test_navier_stokes_terms_are_the_operators_formulas():
    pde = pkg("nn.pde")
    terms = pde.navier_stokes_2D_terms()
    assert len(terms) == 14 and {t[0] for t in terms} == {0, 1, 2}
    g = torch.Generator().manual_seed(3)
    J = torch.randn(3, 6, 40, generator=g, dtype=torch.float64)          # (K, channel, B)

    class Model:                                                        # the duck type of the operator's fused branch
        n_out, input_dim = 3, 3
        def jets(self, X): raise AssertionError
        def jets_all(self, X): return J.permute(2, 0, 1)
    z = torch.zeros(40, 1, dtype=torch.float64)
    want = torch.stack([r[:, 0] for r in pde.navier_stokes_2D_operator(Model(), z.clone(), z.clone(), z.clone())])
    got = S.eval_terms(J, terms, 3)
    assert (got - want).abs().max().item() < 1e-14
    assert want.abs().min(1).values.min().item() > 0
    # the defaults are the reference's constants; the arguments scale them
    got2 = S.eval_terms(J, pde.navier_stokes_2D_terms(viscosity=0.05, density=1 / 0.7), 3)
    assert (got2[0] - want[0]).abs().max().item() == 0 and (got2[1] - want[1]).abs().max().item() > 1e-3


# ---- 4. param_layout(K) is model.parameters() order
@pytest.mark.parametrize("K", [1, 3, 4])
def test_param_layout_is_parameters_order(K):
    Solver = pkg("nn.DVPDESolver").DVPDESolver
    model = Solver(_args([3, 8, K]), _Log(), device="cpu")
    lay = pkg("hip.engine").param_layout(8, 4, 12, K)
    off = 0
    for name, p in model.named_parameters():
        assert lay[name][0] == off and int(np.prod(lay[name][1])) == p.numel(), name
        if name != "quantum_layer.params":       # (the layer keeps its parameters as (layers, per layer))
            assert lay[name][1] == tuple(p.shape), name
        off += p.numel()
    assert lay["__total__"][0] == off
    ref, NP = S.layout(8, 4, 12, K)
    assert NP == off and ref["W4"][0] == lay["postprocessor.2.weight"][0] and ref["theta"][0] == lay["quantum_layer.params"][0]
    if K == 1:
        assert lay == pkg("hip.engine").param_layout(8, 4, 12)


# ---- 5. the references of the GPU cases are not vacuous
def _n_theta(case):
    ans, n, Lq = S.CASES[case][:3]
    return Lq * int(pkg("circuits").params_per_layer(ans, n))


@pytest.mark.parametrize("case", list(S.CASES))
def test_reference_blocks_carry_weight(case):
    ans, n, Lq, enc, B_res, n_ic, n_bc, K = S.CASES[case]
    ref = S.case_reference(case)
    for name, s in S.blocks(S.H, n, _n_theta(case), K).items():
        assert np.abs(ref["grad"][s]).max() >= THETA_MIN, name
    if K == 3:         # the pressure is not prescribed (w_out = 0) and enters through p_x, p_y only
        lay, _ = S.layout(S.H, n, _n_theta(case), K)
        assert ref["grad"][lay["b4"][0] + 2] == 0.0


@pytest.mark.parametrize("variant", S.CONTROLS)
@pytest.mark.parametrize("case", S.CONTROL_CASES)
def test_negative_controls_of_the_gpu_cases_are_not_vacuous(case, variant):
    ans, n, Lq, enc, B_res, n_ic, n_bc, K = S.CASES[case]
    ref, bad = S.case_reference(case), S.case_reference(case, variant)
    got = np.concatenate([ref["grad"], ref["parts"]])
    err = S.errors(got, bad["grad"], bad["parts"], S.H, n, _n_theta(case), K, TOL_G, TOL_L)
    print(case, variant, {k: round(float(v), 1) for k, v in err.items()})
    for name in ("pre", "post", "theta"):
        assert err[name] > 10.0, (name, err)
