"""The refusal table of the ten ``qc_fused_pinn_*_step`` exports: one row per (entry point, fault), a few rows with two
coinciding faults, each answered by the library's return code.  ``tests/golden/make_step_refusals.py`` records the codes,
``tests/test_step_refusals_cpu.py`` compares them.

Nothing here needs a GPU, and nothing may launch: the rows pass fixed non-null addresses that are never dereferenced, every
validation row runs with ``phases = 0``, the sample-phase rows with ``QC_PHASE_SAMPLE`` alone and the optimiser-buffer rows
with ``QC_PHASE_UPDATE`` alone, and every row but the baseline of each entry is refused before anything would run.  So the
table is evaluated only where no GPU is visible.

``qc_program_create`` allocates device memory, so the program of a descriptor is a host mirror of ``qc_program``
(csrc/qc_types.h) whose kernel family is the library's own record; ``check_program_mirror`` asks the library's host-only
accessors whether the mirror's fields lie where the library reads them.
"""
import ctypes as C
import math

from conftest import pkg

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
N, H, N_THETA = 2, 3, 2                      # cascade, n = 2: two trainable angles
B_RES, N_IC, N_BC = 128, 64, 5               # two residual tiles, a full and a partial value tile
DS_ROWS = (11, 4, 6)                         # residual, IC, BC rows of the resident dataset


class QcProgram(C.Structure):
    """Host mirror of ``qc_program`` (csrc/qc_types.h), field for field."""
    _fields_ = [("n_qubits", C.c_int), ("n_gates", C.c_int), ("n_params", C.c_int), ("n_u4", C.c_int), ("static_id", C.c_int),
                ("d_gates", C.c_void_p), ("h_gates", C.c_void_p), ("h2", C.c_void_p),
                ("amplitude", C.c_int), ("lead_rx", C.c_int), ("n_diag_runs", C.c_int),
                ("diag_g0", C.c_int * 8), ("diag_g1", C.c_int * 8), ("d_diag_list", C.c_void_p),
                ("fam", C.c_void_p), ("angle_map", C.c_int), ("ff_m", C.c_int), ("d_ff_freq", C.c_void_p),
                ("n_embed", C.c_int), ("embed_scaled", C.c_int)]


def fake(i: int) -> int:
    """A non-null, 64-byte aligned address that nothing dereferences."""
    return 0x100000 + 4096 * i


def family(lib, name):
    """Address of the library's kernel-family record ``qc_family_<name>``; None: a program without a family."""
    return None if name is None else C.addressof(C.c_char.in_dll(lib, "qc_family_" + name))


def program(lib, n=N, n_params=N_THETA, fam="reg", **fields) -> QcProgram:
    p = QcProgram(n_qubits=n, n_gates=4, n_params=n_params, static_id=-1, fam=family(lib, fam))
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def check_program_mirror(lib) -> None:
    """The library reads the mirror's fields where the mirror has them (its accessors that touch no device)."""
    L = pkg("hip.lib")
    p = program(lib, n=3, n_diag_runs=1)
    p.n_gates = 5
    assert lib.qc_trig_bytes(C.byref(p)) == 16 * (5 + 8)                    # n_gates, n_diag_runs, n_qubits
    assert lib.qc_step_workspace_bytes(C.byref(p), 64, 0) > 0               # fam: the register family keeps final states
    assert lib.qc_program_set_angle_map(C.byref(p), L.QC_ANGLE_MAP_TANH_PI) == OK and p.angle_map == L.QC_ANGLE_MAP_TANH_PI
    p.ff_m = 5
    assert lib.qc_program_set_input_map(C.byref(p), None, 0) == OK and p.ff_m == 0
    assert lib.qc_program_set_encoding(C.byref(p), 1) == OK and p.amplitude == 1       # h2 is null: no plan to rebuild
    p.n_embed = 1
    assert lib.qc_program_set_encoding(C.byref(p), 0) == OK
    assert lib.qc_program_set_encoding(C.byref(p), 1) == ERR_UNSUPPORTED    # n_embed


# ---- the records of one call
ENTRIES = {   # entry -> the side records it takes, in order
    "residual": (), "data": ("data",), "coef": ("data", "coef"), "inverse": ("data", "learn"), "balanced": ("data", "bal"),
    "adaptive": ("data", "coef", "adapt"), "system": ("sys",), "causal": ("data", "causal"),
    "gradnorm": ("data", "coef", "gn"), "coef_tt": ("data", "coef_tt"),
}
OPTIONAL = {("adaptive", "coef"), ("gradnorm", "data"), ("gradnorm", "coef")}      # records an entry accepts as NULL
ANALYTIC = ("residual",)                     # entries on analytic targets; the system entry reads no problem id
STEP = tuple(e for e in ENTRIES if e != "coef_tt")      # entries whose descriptor checks are fused_step's


class Call:
    """Everything one call passes; a fault is a function that edits it."""

    def __init__(self, lib, entry):
        L = pkg("hip.lib")
        self.lib, self.entry, self.phases = lib, entry, 0
        self.prog = program(lib)
        d = self.d = L.QcStepDesc()
        d.trig_dev, d.H, d.n, d.n_theta = fake(1), H, N, N_THETA
        d.params_dev, d.m_dev, d.v_dev, d.opt_state_dev = fake(2), fake(3), fake(4), fake(5)
        d.X_res_dev, d.B_res, d.X_val_dev, d.B_val = fake(6), B_RES, fake(7), N_IC + N_BC
        d.ajets_res_dev, d.qjets_res_dev, d.qbar_res_dev, d.abar_res_dev = fake(8), fake(9), fake(10), fake(11)
        d.ajets_val_dev, d.qjets_val_dev, d.qbar_val_dev, d.abar_val_dev = fake(12), fake(13), fake(14), fake(15)
        d.part_dev, d.part_rows_cap, d.flat_dev = fake(16), 2 + 2, fake(17)
        self.fit_stride()
        d.pde.problem = L.QC_PROBLEM_CONVECTION_DIFFUSION if entry in ANALYTIC else L.QC_PROBLEM_TABULATED
        d.hyper.beta1, d.hyper.beta2, d.hyper.eps = 0.9, 0.999, 1e-8
        d.hyper.w_res, d.hyper.w_bc, d.hyper.w_ic = 2.0, 4.0, 2.0
        d.n_ic, d.sample_seed = N_IC, 7
        self.data = L.QcStepData(fake(20), fake(21), 0.0, fake(22), fake(23), DS_ROWS[0], fake(24), fake(25), DS_ROWS[1],
                                 fake(26), fake(27), DS_ROWS[2])
        self.coef = L.QcStepCoef(fake(30), fake(31))
        self.coef_tt = L.QcStepCoefTT(fake(32), fake(33))
        self.learn = L.QcStepLearn()
        self.bal = L.QcStepBalance()
        for k in range(L.QC_COEF_COLS):
            self.learn.base[k], self.learn.scale[k] = 0.5, 1.0
        for k in range(L.QC_BAL_TERMS):
            self.bal.scale[k] = 1.0
        self.adapt = L.QcStepAdapt(fake(34), DS_ROWS[0])
        self.sys = L.system_record(2, 1, [(0, 0, 1, -1, -1, 1.0)], [1.0], [1.0, 1.0])
        self.sys.target_res_dev, self.sys.target_val_dev = fake(35), fake(36)
        self.sys.ds_X_res, self.sys.ds_r, self.sys.ds_n_res = fake(22), fake(23), DS_ROWS[0]
        self.sys.ds_X_ic, self.sys.ds_u_ic, self.sys.ds_n_ic = fake(24), fake(25), DS_ROWS[1]
        self.sys.ds_X_bc, self.sys.ds_u_bc, self.sys.ds_n_bc = fake(26), fake(27), DS_ROWS[2]
        self.causal = L.QcStepCausal(2, 1.0, 2.0, 100.0, 0.99, fake(37), fake(38), None, 0)
        self.gn = L.QcStepGradnorm(0.1, 100.0, 1, 1.0, 1.0, fake(39), None, 0)
        self.null = set()                    # records passed as NULL ("d": the descriptor)

    def fit_stride(self) -> None:
        """part_stride: exactly what the entry's layout asks for (its parameters, then the three loss sums)."""
        L, d = pkg("hip.lib"), self.d
        own = {"inverse": L.QC_COEF_COLS, "balanced": L.QC_BAL_TERMS}.get(self.entry, 0)
        NP = pkg("hip.engine").param_layout(d.H, d.n, d.n_theta, K=2 if self.entry == "system" else 1)["__total__"][0]
        self.stride = d.part_stride = NP + own + 3

    def run(self) -> int:
        self.d.prog = C.addressof(self.prog) if self.prog is not None else None
        ref = lambda name: None if name in self.null else C.byref(getattr(self, name))
        fn = getattr(self.lib, f"qc_fused_pinn_{self.entry}_step")
        return fn(ref("d"), *(ref(r) for r in ENTRIES[self.entry]), self.phases, None)


# ---- faults
def _set(**fields):
    def f(c):
        for k, v in fields.items():
            setattr(c.d, k, v)
    return f


def _prog(**kw):
    """Another program; the descriptor follows its qubit and parameter counts."""
    def f(c):
        c.prog = program(c.lib, **kw)
        c.d.n, c.d.n_theta = c.prog.n_qubits, c.prog.n_params
        c.fit_stride()
    return f


def _null(name):
    return lambda c: c.null.add(name)


def _rec(rec, **fields):
    def f(c):
        for k, v in fields.items():
            setattr(getattr(c, rec), k, v)
    return f


def _phase(name):
    def f(c):
        c.phases = getattr(pkg("hip.lib"), "QC_PHASE_" + name)
    return f


def _no_prog(c):
    c.prog = None


def _problem(v):
    return lambda c: setattr(c.d.pde, "problem", v)


FAULTS = {
    "null_desc": _null("d"),
    "null_prog": _no_prog, "null_trig": _set(trig_dev=None), "null_params": _set(params_dev=None),
    "null_part": _set(part_dev=None), "null_flat": _set(flat_dev=None),
    "n_mismatch": _set(n=N + 1), "n_theta_mismatch": _set(n_theta=N_THETA + 1),
    "u4_without_umat": _prog(n=4, n_params=4, n_u4=1),
    "H_zero": _set(H=0), "H_too_large": _set(H=1025),
    "stride_one_short": lambda c: _set(part_stride=c.stride - 1)(c), "rows_cap_one_short": _set(part_rows_cap=3),
    "problem_out_of_range": _problem(4), "problem_negative": _problem(-1),
    "problem_not_tabulated": _problem(0), "problem_tabulated": _problem(3),
    "no_family": _prog(n=N, n_params=N_THETA, fam=None, n_embed=1),
    "amplitude_without_workspace": _prog(amplitude=1),
    "input_map": _prog(ff_m=2, d_ff_freq=fake(40)),
    "face_rule_below_random": _set(sample_bc_face_points=-2),
    # the seven-channel entry
    "n6": _prog(n=6, n_params=6, fam="wave"), "embed_program": _prog(fam="reup", n_embed=1),
    "amplitude": _prog(amplitude=1), "angle_map": _prog(angle_map=1),
    "null_X_res": _set(X_res_dev=None), "null_ajets_res": _set(ajets_res_dev=None), "null_qjets_res": _set(qjets_res_dev=None),
    "null_qbar_res": _set(qbar_res_dev=None), "null_abar_res": _set(abar_res_dev=None),
    "null_coef_res": lambda c: _rec("coef_tt" if c.entry == "coef_tt" else "coef", coef_res_dev=None)(c),
    "null_target_res": _rec("data", target_res_dev=None), "null_target_val": _rec("data", target_val_dev=None),
    # the side records' own rules
    "learn_base_nan": lambda c: c.learn.base.__setitem__(2, math.nan),
    "bal_scale_inf": lambda c: c.bal.scale.__setitem__(1, math.inf),
    "adapt_rows_differ": _rec("adapt", n_rows=DS_ROWS[0] - 1), "adapt_null_buffer": _rec("adapt", adapt_dev=None),
    "adaptive_no_residual": _set(B_res=0),
    "sys_K_zero": _rec("sys", K=0), "sys_null_target_val": _rec("sys", target_val_dev=None),
    "causal_B_res_not_whole_slabs": _set(B_res=64), "causal_B_res_zero": _set(B_res=0),
    "causal_offset_negative": _set(sample_off_res=-64), "causal_offset_mid_tile": _set(sample_off_res=32),
    "causal_one_slab": _rec("causal", n_slabs=1), "causal_rows_cap_2p31": _set(part_rows_cap=1 << 31),
    "gradnorm_n_ic_mid_tile": _set(n_ic=60), "gradnorm_n_ic_negative": _set(n_ic=-1), "gradnorm_n_ic_above_B_val": _set(n_ic=128),
    "gradnorm_alpha": _rec("gn", alpha=1.5), "gradnorm_coef_without_data": _null("data"),
    "comm": _set(comm=fake(41)),
    # QC_PHASE_SAMPLE alone
    "sample_negative_offset": lambda c: (_phase("SAMPLE")(c), _set(sample_off_ic=-1)(c)),
    "sample_null_segment": lambda c: (_phase("SAMPLE")(c), _rec("sys" if c.entry == "system" else "data", ds_X_bc=None)(c)),
    "sample_null_ds_coef": lambda c: (_phase("SAMPLE")(c), _rec("coef_tt" if c.entry == "coef_tt" else "coef", ds_coef=None)(c)),
    "sample_null_X_val": lambda c: (_phase("SAMPLE")(c), _set(X_val_dev=None)(c)),
    # QC_PHASE_UPDATE alone
    "update_null_m": lambda c: (_phase("UPDATE")(c), _set(m_dev=None)(c)),
    "update_null_v": lambda c: (_phase("UPDATE")(c), _set(v_dev=None)(c)),
    "update_null_opt_state": lambda c: (_phase("UPDATE")(c), _set(opt_state_dev=None)(c)),
}

TABULATED = tuple(e for e in ENTRIES if e not in ANALYTIC and e != "system")


def rows():
    """[(entry, (fault, ...))]: the baseline of each entry, its single faults, then the coinciding pairs."""
    out = []
    for e, recs in ENTRIES.items():
        out.append((e, ()))
        single = ["null_desc"] + ["null_" + r for r in recs if (e, r) not in OPTIONAL]
        single += ["null_prog", "null_trig", "null_params", "null_part", "null_flat", "n_mismatch", "n_theta_mismatch", "H_zero",
                   "H_too_large", "stride_one_short", "rows_cap_one_short", "sample_negative_offset",
                   "sample_null_X_val", "update_null_m", "update_null_v", "update_null_opt_state"]
        if e not in ANALYTIC:                # the coordinate draw reads no dataset
            single += ["sample_null_segment"]
        if e != "system":                    # a system's source has no boundary rule
            single += ["face_rule_below_random"]
        if e in STEP:
            single += ["no_family", "amplitude_without_workspace"]
        if e in ANALYTIC:
            single += ["problem_out_of_range", "problem_negative", "problem_tabulated"]
        if e in TABULATED:
            single += ["problem_out_of_range", "problem_not_tabulated", "null_target_res", "null_target_val"]
        single += {
            "coef": ["null_coef_res", "sample_null_ds_coef"],
            "inverse": ["learn_base_nan"], "balanced": ["bal_scale_inf"],
            "adaptive": ["adapt_rows_differ", "adapt_null_buffer", "adaptive_no_residual", "sample_null_ds_coef"],
            "system": ["sys_K_zero", "sys_null_target_val", "input_map"],
            "causal": ["causal_B_res_not_whole_slabs", "causal_B_res_zero", "causal_offset_negative", "causal_offset_mid_tile",
                       "causal_one_slab", "causal_rows_cap_2p31", "comm"],
            "gradnorm": ["gradnorm_n_ic_mid_tile", "gradnorm_n_ic_negative", "gradnorm_n_ic_above_B_val", "gradnorm_alpha",
                         "gradnorm_coef_without_data", "comm"],
            "coef_tt": ["u4_without_umat", "n6", "embed_program", "amplitude", "input_map", "angle_map", "null_X_res",
                        "null_ajets_res", "null_qjets_res", "null_qbar_res", "null_abar_res", "null_coef_res", "sample_null_ds_coef"],
        }.get(e, [])
        out += [(e, (f,)) for f in single]
    out += [   # two faults at once: the code is that of the check that comes first
        ("coef_tt", ("null_part", "embed_program")), ("coef_tt", ("problem_not_tabulated", "n6")),
        ("coef_tt", ("null_trig", "amplitude")), ("coef_tt", ("embed_program", "n_mismatch")), ("coef_tt", ("n6", "null_X_res")),
        ("coef_tt", ("input_map", "stride_one_short")), ("coef_tt", ("angle_map", "update_null_m")),
        ("coef_tt", ("null_coef_res", "stride_one_short")), ("coef_tt", ("update_null_m", "rows_cap_one_short")),
        ("causal", ("comm", "causal_B_res_not_whole_slabs")), ("causal", ("null_causal", "comm")),
        ("causal", ("comm", "no_family")), ("gradnorm", ("comm", "gradnorm_n_ic_mid_tile")), ("gradnorm", ("gradnorm_alpha", "comm")),
        ("system", ("input_map", "sys_K_zero")), ("system", ("input_map", "null_part")),
        ("residual", ("no_family", "stride_one_short")), ("residual", ("no_family", "null_part")),
        ("data", ("H_too_large", "no_family")), ("data", ("no_family", "update_null_m")),
        ("data", ("update_null_m", "stride_one_short")), ("balanced", ("n_mismatch", "no_family")),
        ("inverse", ("problem_not_tabulated", "no_family")),
    ]
    return out


def evaluate(lib):
    """The table as the library answers it: [{"entry", "faults", "phases", "code"}]."""
    check_program_mirror(lib)
    table = []
    for entry, faults in rows():
        c = Call(lib, entry)
        for f in faults:
            (_null(f[5:]) if f.startswith("null_") and f[5:] in ENTRIES[entry] else FAULTS[f])(c)
        table.append({"entry": entry, "faults": list(faults), "phases": c.phases, "code": c.run()})
    return table
