"""ctypes binding of ``libqcpinn_hip.so`` (C ABI in ``include/qcpinn_hip.h``).

The library is the product: there is no CPU or torch fallback behind these calls.  Loading
fails loudly when the shared object is missing, and every call raises ``QcError`` on a
non-zero return code.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# (QC_LIB: a diagnostic build of the same library, e.g. one compiled with -DH2_ABLATE_GATES / -DH2_ABLATE_SYNC, csrc/qc_h2_shared.h)
LIB_PATH = os.environ.get("QC_LIB") or os.path.join(os.path.dirname(_HERE), "libqcpinn_hip.so")

QC_PHASE_GRADS = 1
QC_PHASE_UPDATE = 2
QC_PHASE_SAMPLE = 4
QC_STAGE_PRE_FWD, QC_STAGE_CIRCUIT_FWD, QC_STAGE_POST, QC_STAGE_CIRCUIT_BWD, QC_STAGE_PRE_BWD = range(5)

# every symbol include/qcpinn_hip.h declares
EXPORTS = (
    "qc_version", "qc_error_string", "qc_last_hip_error", "qc_program_create", "qc_program_destroy",
    "qc_trig_bytes", "qc_program_set_encoding", "qc_amp_forward", "qc_amp_backward", "qc_prepare_gates",
    "qc_circuit_workspace_bytes", "qc_circuit_workspace_bytes_batch", "qc_hbm_plan_describe", "qc_wave_sched_describe", "qc_forward_expval", "qc_backward_expval", "qc_forward_jets",
    "qc_backward_jets", "qc_forward_jets_keep", "qc_backward_jets_kept", "qc_pre_forward", "qc_pre_backward", "qc_post", "qc_reduce_rows", "qc_adam_step",
    "qc_sample_collocation", "qc_sample_collocation_faces", "qc_step_workspace_bytes", "qc_fused_pinn_residual_step",
    "qc_fused_step_stage", "qc_post_multi", "qc_comm_unique_id", "qc_comm_create", "qc_comm_destroy", "qc_allreduce_grads",
    "qc_pre_forward_map", "qc_pre_backward_map", "qc_program_set_angle_map",
    "qc_post_data", "qc_sample_dataset", "qc_fused_pinn_data_step",
    "qc_post_coef", "qc_sample_dataset_coef", "qc_fused_pinn_coef_step",
    "qc_dataset_scores", "qc_adapt_bytes", "qc_adapt_build", "qc_sample_dataset_adaptive", "qc_fused_pinn_adaptive_step",
    "qc_post_system", "qc_sample_dataset_system", "qc_fused_pinn_system_step",
    "qc_post_learn", "qc_fused_pinn_inverse_step",
    "qc_lbfgs_workspace_bytes", "qc_lbfgs_init", "qc_lbfgs_restart", "qc_lbfgs_step",
    "qc_post_balance", "qc_balance_adam_step", "qc_fused_pinn_balanced_step",
    "qc_causal_init", "qc_sample_dataset_slabs", "qc_causal_fold", "qc_fused_pinn_causal_step",
    "qc_gradnorm_init", "qc_gradnorm_fold", "qc_fused_pinn_gradnorm_step",
    "qc_program_set_input_map", "qc_pre_forward_ff", "qc_pre_backward_ff",
    "qc_pre_forward_tt", "qc_pre_backward_tt", "qc_forward_jets_tt", "qc_backward_jets_tt", "qc_post_coef_tt",
    "qc_post_jets_tt", "qc_sample_dataset_coef_tt", "qc_fused_pinn_coef_tt_step",
    "qc_ensemble_strides", "qc_fused_pinn_ensemble_step",
)


QC_PROBLEM_CONVECTION_DIFFUSION, QC_PROBLEM_PURE_DIFFUSION, QC_PROBLEM_GAUSSIAN_PULSE = 0, 1, 2      # qc_pde.problem
QC_PROBLEM_TABULATED = 3        # targets as data: accepted by qc_post_data / qc_fused_pinn_data_step only
QC_COEF_COLS = 7                # operator row of a residual point: c_u, c_t, c_x, c_y, d_xx, d_yy, c_3 (qc_step_coef)
QC_NCH_TT = 7                   # derivative channels of the seven-channel entry points: the six, then d2/dt2
QC_COEF_TT_COLS = 8             # their operator row: the QC_COEF_COLS columns, then d_tt (qc_step_coef_tt)
QC_BAL_TERMS = 3                # loss terms of a balancer: residual, BC, IC (qc_step_balance)
QC_CAUSAL_MAX_SLABS = 64        # most time slabs of a causal record (qc_step_causal)
QC_CAUSAL_HEAD = 4              # words {eps, n_raised, n_steps, hist_base} ahead of W[M], L[M] in a causal record
QC_GRADNORM_STATE_WORDS = 16    # 4-byte words of a gradient-norm record (qc_step_gradnorm)
QC_GRADNORM_HIST_COLS = 7       # lam_bc, lam_ic, m_r, a_bc, a_ic, lambda-weighted loss, updated: a row of its history
QC_ADAPT_BLOCK = 1024           # rows per entry of the coarse table of an adaptive-sampling buffer (qc_adapt_bytes)
QC_ADAPT_FLOOR_MAX = 256.0      # largest floor_c qc_adapt_build accepts
QC_KMAX, QC_EQMAX, QC_TERMS_MAX = 4, 4, 32            # outputs, equations and terms of a system (qc_step_system)
QC_ANGLE_MAP_NONE, QC_ANGLE_MAP_TANH_PI = 0, 1       # output map of the pre network (qc_program_set_angle_map)
QC_FF_MAX = 64                                       # most frequencies of an input map (qc_program_set_input_map)
QC_BC_RANDOM_FACE = -1                               # sample_bc_face_points: a random face per boundary point
QC_LBFGS_MAX_HISTORY = 32                            # most curvature pairs of an L-BFGS workspace (qc_lbfgs_init)
QC_LBFGS_FIXED, QC_LBFGS_ARMIJO = 0, 1               # qc_lbfgs_hyper.line_search
QC_LBFGS_REC_WORDS = 32                              # 4-byte words of the record at the head of an L-BFGS workspace


class QcError(RuntimeError):
    pass


class QcPde(C.Structure):
    _fields_ = [("D", C.c_float), ("vx", C.c_float), ("vy", C.c_float),
                ("c_t", C.c_float), ("c_x", C.c_float), ("c_y", C.c_float), ("d_xx", C.c_float), ("d_yy", C.c_float),
                ("w_res", C.c_float),
                ("inv_n_res", C.c_float), ("w_val_a", C.c_float), ("w_val_b", C.c_float),
                ("inv_n_a", C.c_float), ("inv_n_b", C.c_float), ("problem", C.c_int), ("n_seg_a", C.c_int64)]


class QcOptHyper(C.Structure):
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float), ("max_norm", C.c_float),
                ("sched_factor", C.c_float), ("sched_threshold", C.c_float), ("sched_min_lr", C.c_float),
                ("sched_eps", C.c_float), ("sched_patience", C.c_int), ("w_res", C.c_float),
                ("w_bc", C.c_float), ("w_ic", C.c_float)]


class QcLbfgsHyper(C.Structure):
    """qc_lbfgs_hyper: history size, line search and its constants, and the loss weights of f."""
    _fields_ = [("history", C.c_int), ("line_search", C.c_int), ("max_ls", C.c_int),
                ("lr", C.c_float), ("c1", C.c_float), ("shrink_lo", C.c_float), ("shrink_hi", C.c_float),
                ("curv_eps", C.c_float), ("w_res", C.c_float), ("w_bc", C.c_float), ("w_ic", C.c_float)]


class QcStepDesc(C.Structure):
    _fields_ = [
        ("prog", C.c_void_p), ("trig_dev", C.c_void_p), ("umat_dev", C.c_void_p),
        ("H", C.c_int), ("n", C.c_int), ("n_theta", C.c_int),
        ("params_dev", C.c_void_p), ("m_dev", C.c_void_p), ("v_dev", C.c_void_p), ("opt_state_dev", C.c_void_p),
        ("hist_dev", C.c_void_p), ("hist_cap", C.c_int),
        ("X_res_dev", C.c_void_p), ("B_res", C.c_int64),
        ("X_val_dev", C.c_void_p), ("B_val", C.c_int64),
        ("ajets_res_dev", C.c_void_p), ("qjets_res_dev", C.c_void_p), ("qbar_res_dev", C.c_void_p),
        ("abar_res_dev", C.c_void_p),
        ("ajets_val_dev", C.c_void_p), ("qjets_val_dev", C.c_void_p), ("qbar_val_dev", C.c_void_p),
        ("abar_val_dev", C.c_void_p),
        ("part_dev", C.c_void_p), ("part_stride", C.c_int64), ("part_rows_cap", C.c_int64),
        ("flat_dev", C.c_void_p),
        ("pde", QcPde), ("hyper", QcOptHyper),
        ("n_ic", C.c_int64), ("sample_off_res", C.c_int64), ("sample_off_ic", C.c_int64),
        ("sample_off_bc", C.c_int64), ("sample_seed", C.c_uint64), ("sample_step", C.c_uint64),
        ("sample_bc_face_points", C.c_int64),
        ("circ_ws_dev", C.c_void_p), ("circ_ws_bytes", C.c_size_t),
        ("comm", C.c_void_p),
    ]


class QcStepData(C.Structure):
    """qc_step_data: batch targets, c_u and the resident dataset of the tabulated step."""
    _fields_ = [
        ("target_res_dev", C.c_void_p), ("target_val_dev", C.c_void_p), ("c_u", C.c_float),
        ("ds_X_res", C.c_void_p), ("ds_r", C.c_void_p), ("ds_n_res", C.c_int64),
        ("ds_X_ic", C.c_void_p), ("ds_u_ic", C.c_void_p), ("ds_n_ic", C.c_int64),
        ("ds_X_bc", C.c_void_p), ("ds_u_bc", C.c_void_p), ("ds_n_bc", C.c_int64),
    ]


class QcStepCoef(C.Structure):
    """qc_step_coef: the [7][B_res] operator rows of the current residual batch and the dataset's [N_res][7] table."""
    _fields_ = [("coef_res_dev", C.c_void_p), ("ds_coef", C.c_void_p)]


class QcStepCoefTT(C.Structure):
    """qc_step_coef_tt: the [8][B_res] operator rows (c_u, c_t, c_x, c_y, d_xx, d_yy, c_3, d_tt) of the current residual
    batch and the dataset's [N_res][8] table."""
    _fields_ = [("coef_res_dev", C.c_void_p), ("ds_coef", C.c_void_p)]


class QcStepLearn(C.Structure):
    """qc_step_learn: base and scale of the trainable operator c_k = fmaf(scale_k, p_k, base_k) (QC_COEF_COLS order) and the
    optional [cap][7] history of the c_k each step used."""
    _fields_ = [("base", C.c_float * QC_COEF_COLS), ("scale", C.c_float * QC_COEF_COLS),
                ("coef_hist_dev", C.c_void_p), ("coef_hist_cap", C.c_int)]


class QcStepBalance(C.Structure):
    """qc_step_balance: scale of the three log-variances s_k = scale_k p_k (order residual, BC, IC) and the optional
    [cap][3] history of the effective weights w_k exp(-s_k) each step used."""
    _fields_ = [("scale", C.c_float * QC_BAL_TERMS), ("weight_hist_dev", C.c_void_p), ("weight_hist_cap", C.c_int)]


class QcStepCausal(C.Structure):
    """qc_step_causal: slab count, the annealing of eps (start, growth, cap, threshold on the smallest weight), the
    [M + 1] int64 slab offsets of the sorted residual segment, the device record {eps, n_raised, n_steps, hist_base, W[M],
    L[M]} and the optional [cap][1 + 2 M] history of (eps, W, L) per step."""
    _fields_ = [("n_slabs", C.c_int32), ("eps0", C.c_float), ("eps_growth", C.c_float), ("eps_max", C.c_float),
                ("delta", C.c_float), ("slab_lo_dev", C.c_void_p), ("state_dev", C.c_void_p), ("hist_dev", C.c_void_p),
                ("hist_cap", C.c_int32)]


class QcStepGradnorm(C.Structure):
    """qc_step_gradnorm: the moving average (alpha), the cap of the weights, the update period, the starting weights of the
    BC and the IC term, the device record {lam_bc, lam_ic, n_steps, hist_base, n_updates, m_r, a_bc, a_ic, hat_bc, hat_ic, 0..}
    of QC_GRADNORM_STATE_WORDS words and the optional [cap][QC_GRADNORM_HIST_COLS] history."""
    _fields_ = [("alpha", C.c_float), ("lam_max", C.c_float), ("every", C.c_int32), ("lam0_bc", C.c_float),
                ("lam0_ic", C.c_float), ("state_dev", C.c_void_p), ("hist_dev", C.c_void_p), ("hist_cap", C.c_int32)]


class QcStepEnsemble(C.Structure):
    """qc_step_ensemble: members, the distance between two members' slices of every per-model buffer of the descriptor
    (floats; trig_stride and ws_stride bytes) and the optional device tables of M qc_pde / qc_opt_hyper records."""
    _fields_ = [("M", C.c_int), ("params_stride", C.c_int64), ("flat_stride", C.c_int64), ("hist_stride", C.c_int64),
                ("trig_stride", C.c_int64), ("x_res_stride", C.c_int64), ("x_val_stride", C.c_int64),
                ("jets_res_stride", C.c_int64), ("jets_val_stride", C.c_int64), ("ws_stride", C.c_int64),
                ("pde_dev", C.c_void_p), ("hyper_dev", C.c_void_p)]


class QcStepAdapt(C.Structure):
    """qc_step_adapt: the buffer of qc_adapt_build ({64-byte record, cdf[n_rows], coarse[ceil(n_rows / 1024)]}) and its rows."""
    _fields_ = [("adapt_dev", C.c_void_p), ("n_rows", C.c_int64)]


class QcSysTerm(C.Structure):
    """qc_sys_term: coef * q[out][chan] * (mul0 >= 0 ? u[mul0] : 1) * (mul1 >= 0 ? u[mul1] : 1) in equation eq."""
    _fields_ = [("eq", C.c_int32), ("out", C.c_int32), ("chan", C.c_int32), ("mul0", C.c_int32), ("mul1", C.c_int32),
                ("coef", C.c_float)]


class QcStepSystem(C.Structure):
    """qc_step_system: the operator of a K-output system as a term list, the weights of its equations and outputs, the
    batch-minor targets of the current batches ([n_eq][B_res] or NULL, [K][B_val]) and the resident dataset with row-major
    target tables ([N][n_eq] or NULL, [N][K], [N][K])."""
    _fields_ = [
        ("K", C.c_int32), ("n_eq", C.c_int32), ("n_terms", C.c_int32),
        ("terms", QcSysTerm * QC_TERMS_MAX), ("w_eq", C.c_float * QC_EQMAX), ("w_out", C.c_float * QC_KMAX),
        ("target_res_dev", C.c_void_p), ("target_val_dev", C.c_void_p),
        ("ds_X_res", C.c_void_p), ("ds_r", C.c_void_p), ("ds_n_res", C.c_int64),
        ("ds_X_ic", C.c_void_p), ("ds_u_ic", C.c_void_p), ("ds_n_ic", C.c_int64),
        ("ds_X_bc", C.c_void_p), ("ds_u_bc", C.c_void_p), ("ds_n_bc", C.c_int64),
    ]


def system_record(K, n_eq, terms, w_eq, w_out) -> "QcStepSystem":
    """A qc_step_system with its operator filled from ``terms`` = rows (eq, out, chan, mul0, mul1, coef); nothing is
    validated here (the library refuses what is out of range)."""
    s = QcStepSystem()
    s.K, s.n_eq, s.n_terms = int(K), int(n_eq), len(terms)
    for i, t in enumerate(terms[:QC_TERMS_MAX]):
        s.terms[i] = QcSysTerm(int(t[0]), int(t[1]), int(t[2]), int(t[3]), int(t[4]), float(t[5]))
    for e, w in enumerate(list(w_eq)[:QC_EQMAX]):
        s.w_eq[e] = float(w)
    for k, w in enumerate(list(w_out)[:QC_KMAX]):
        s.w_out[k] = float(w)
    return s


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the in-tree library (built by ``__graft_entry__.build()`` / ``make -C csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QcError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C {os.path.join(os.path.dirname(_HERE), 'csrc')}`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, fp = C.c_void_p, C.c_int, C.c_int64, C.c_void_p
    lib.qc_version.restype = i32
    lib.qc_error_string.restype = C.c_char_p
    lib.qc_error_string.argtypes = [i32]
    lib.qc_last_hip_error.restype = i32
    lib.qc_program_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    lib.qc_program_destroy.argtypes = [vp]
    lib.qc_trig_bytes.restype = C.c_size_t
    lib.qc_trig_bytes.argtypes = [vp]
    lib.qc_prepare_gates.argtypes = [vp, fp, vp, vp]
    lib.qc_circuit_workspace_bytes.restype = C.c_size_t
    lib.qc_circuit_workspace_bytes.argtypes = [vp, i32, i32]
    lib.qc_circuit_workspace_bytes_batch.restype = C.c_size_t
    lib.qc_circuit_workspace_bytes_batch.argtypes = [vp, i32, i32, i64]
    lib.qc_hbm_plan_describe.argtypes = [vp, i32, i32, i32, vp, i32]
    lib.qc_wave_sched_describe.argtypes = [vp, i32, i32, i32, vp, i32]
    lib.qc_forward_expval.argtypes = [vp, vp, fp, fp, fp, i64, vp, C.c_size_t, vp]
    lib.qc_backward_expval.argtypes = [vp, vp, fp, fp, fp, fp, fp, i64, i64, i64, vp, C.c_size_t, vp]
    lib.qc_forward_jets.argtypes = [vp, vp, fp, fp, fp, i64, vp, C.c_size_t, vp]
    lib.qc_backward_jets.argtypes = [vp, vp, fp, fp, fp, fp, fp, i64, i64, i64, vp, C.c_size_t, vp]
    lib.qc_forward_jets_keep.argtypes = [vp, vp, fp, fp, fp, i64, fp, vp]
    lib.qc_backward_jets_kept.argtypes = [vp, vp, fp, fp, fp, fp, fp, i64, i64, i64, fp, vp]
    lib.qc_pre_forward.argtypes = [fp, fp, i32, i32, i32, fp, i64, i32, vp]
    lib.qc_pre_backward.argtypes = [fp, fp, i32, i32, i32, fp, fp, i64, i64, i64, i32, vp]
    lib.qc_pre_forward_map.argtypes = [fp, fp, i32, i32, i32, i32, fp, i64, i32, vp]
    lib.qc_pre_backward_map.argtypes = [fp, fp, i32, i32, i32, i32, fp, fp, fp, i64, i64, i64, i32, vp]
    lib.qc_program_set_angle_map.argtypes = [vp, i32]
    lib.qc_program_set_input_map.argtypes = [vp, fp, i32]
    lib.qc_pre_forward_ff.argtypes = [fp, fp, i32, i32, i32, i32, fp, i32, fp, i64, i32, vp]
    lib.qc_pre_backward_ff.argtypes = [fp, fp, i32, i32, i32, i32, fp, i32, fp, fp, fp, i64, i64, i64, i32, vp]
    lib.qc_post.argtypes = [i32, fp, fp, i32, i32, i32, C.POINTER(QcPde), fp, fp, fp, fp, fp, fp, fp, i64, i64,
                            i64, i32, vp]
    lib.qc_post_multi.argtypes = [i32, fp, i32, i32, i32, i32, fp, fp, fp, fp, fp, fp, i64, fp, i64, i64, i64, vp]
    lib.qc_reduce_rows.argtypes = [fp, i64, i64, i32, fp, vp]
    lib.qc_adam_step.argtypes = [fp, i32, fp, fp, fp, vp, C.POINTER(QcOptHyper), fp, i32, vp, i32, vp, vp]
    lib.qc_sample_collocation.argtypes = [fp, i64, i64, fp, i64, i64, i64, i64, C.c_uint64, C.c_uint64, vp]
    lib.qc_sample_collocation_faces.argtypes = [fp, i64, i64, fp, i64, i64, i64, i64, i64, C.c_uint64, C.c_uint64, vp]
    lib.qc_fused_step_stage.argtypes = [C.POINTER(QcStepDesc), i32, vp]
    lib.qc_step_workspace_bytes.restype = C.c_size_t
    lib.qc_step_workspace_bytes.argtypes = [vp, i64, i64]
    lib.qc_program_set_encoding.argtypes = [vp, i32]
    lib.qc_amp_forward.argtypes = [fp, fp, i32, i64, i32, vp]
    lib.qc_amp_backward.argtypes = [fp, fp, fp, i32, i64, i32, vp]
    lib.qc_fused_pinn_residual_step.argtypes = [C.POINTER(QcStepDesc), i32, vp]
    lib.qc_post_data.argtypes = [fp, i32, i32, i32, C.POINTER(QcPde), fp, fp, C.c_float, fp, fp, fp, fp, i64, i64, i64, i32, vp]
    lib.qc_sample_dataset.argtypes = [fp, fp, i64, i64, fp, fp, i64, i64, i64, i64, C.POINTER(QcStepData), C.c_uint64,
                                      C.c_uint64, vp]
    lib.qc_fused_pinn_data_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), i32, vp]
    lib.qc_post_coef.argtypes = [fp, i32, i32, i32, C.POINTER(QcPde), fp, fp, fp, fp, fp, fp, i64, i64, i64, vp]
    lib.qc_sample_dataset_coef.argtypes = [fp, fp, i64, i64, fp, fp, i64, i64, i64, i64, fp, C.POINTER(QcStepData),
                                           C.POINTER(QcStepCoef), C.c_uint64, C.c_uint64, vp]
    lib.qc_fused_pinn_coef_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), C.POINTER(QcStepCoef), i32, vp]
    lib.qc_dataset_scores.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), C.POINTER(QcStepCoef), i64, i64, fp, vp]
    lib.qc_adapt_bytes.restype = C.c_size_t
    lib.qc_adapt_bytes.argtypes = [i64]
    lib.qc_adapt_build.argtypes = [fp, i64, i32, C.c_float, vp, vp]
    lib.qc_sample_dataset_adaptive.argtypes = [fp, fp, i64, i64, fp, fp, i64, i64, i64, i64, fp, C.POINTER(QcStepData),
                                               C.POINTER(QcStepCoef), C.POINTER(QcStepAdapt), C.c_uint64, C.c_uint64, vp]
    lib.qc_fused_pinn_adaptive_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), C.POINTER(QcStepCoef),
                                                C.POINTER(QcStepAdapt), i32, vp]
    lib.qc_post_system.argtypes = [fp, i32, i32, i32, C.POINTER(QcStepSystem), C.POINTER(QcPde), fp, fp, fp, fp, i64, i64, i64,
                                   i32, vp]
    lib.qc_sample_dataset_system.argtypes = [fp, fp, i64, i64, fp, fp, i64, i64, i64, i64, C.POINTER(QcStepSystem), C.c_uint64,
                                             C.c_uint64, vp]
    lib.qc_fused_pinn_system_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepSystem), i32, vp]
    lib.qc_post_learn.argtypes = [fp, i32, i32, i32, C.POINTER(QcPde), C.POINTER(QcStepLearn), fp, fp, fp, fp, fp, i64, i64,
                                  i64, vp]
    lib.qc_fused_pinn_inverse_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), C.POINTER(QcStepLearn), i32, vp]
    lib.qc_lbfgs_workspace_bytes.restype = C.c_size_t
    lib.qc_lbfgs_workspace_bytes.argtypes = [i32, i32]
    lib.qc_lbfgs_init.argtypes = [vp, i32, i32, vp]
    lib.qc_lbfgs_restart.argtypes = [vp, i32, vp]
    lib.qc_lbfgs_step.argtypes = [fp, i32, fp, vp, C.POINTER(QcLbfgsHyper), fp, i32, vp, i32, vp, vp]
    lib.qc_post_balance.argtypes = [fp, i32, i32, i32, C.POINTER(QcPde), C.POINTER(QcStepBalance), fp, fp, C.c_float, fp, fp,
                                    fp, fp, i64, i64, i64, i32, vp]
    lib.qc_balance_adam_step.argtypes = [fp, i32, fp, fp, fp, vp, C.POINTER(QcOptHyper), C.POINTER(QcStepBalance), fp, i32, vp,
                                         i32, vp, vp]
    lib.qc_fused_pinn_balanced_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), C.POINTER(QcStepBalance), i32, vp]
    lib.qc_causal_init.argtypes = [vp, C.POINTER(QcStepCausal), vp]
    lib.qc_sample_dataset_slabs.argtypes = [fp, fp, i64, i64, fp, fp, i64, i64, i64, i64, C.POINTER(QcStepData), i32, vp,
                                            C.c_uint64, C.c_uint64, vp]
    lib.qc_causal_fold.argtypes = [fp, i64, i64, i64, i32, C.POINTER(QcStepCausal), fp, vp]
    lib.qc_fused_pinn_causal_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), C.POINTER(QcStepCausal), i32, vp]
    lib.qc_gradnorm_init.argtypes = [vp, C.POINTER(QcStepGradnorm), vp]
    lib.qc_gradnorm_fold.argtypes = [fp, i64, i64, i64, i64, i32, C.POINTER(QcStepGradnorm), fp, fp, vp]
    lib.qc_fused_pinn_gradnorm_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), C.POINTER(QcStepCoef),
                                                C.POINTER(QcStepGradnorm), i32, vp]
    lib.qc_pre_forward_tt.argtypes = [fp, fp, i32, i32, i32, fp, i64, vp]
    lib.qc_pre_backward_tt.argtypes = [fp, fp, i32, i32, i32, fp, fp, i64, i64, i64, vp]
    lib.qc_forward_jets_tt.argtypes = [vp, vp, fp, fp, fp, i64, vp]
    lib.qc_backward_jets_tt.argtypes = [vp, vp, fp, fp, fp, fp, fp, i64, i64, i64, vp]
    lib.qc_post_coef_tt.argtypes = [fp, i32, i32, i32, C.POINTER(QcPde), fp, fp, fp, fp, fp, fp, i64, i64, i64, vp]
    lib.qc_post_jets_tt.argtypes = [i32, fp, i32, i32, i32, fp, fp, fp, fp, i64, i64, i64, vp]
    lib.qc_sample_dataset_coef_tt.argtypes = [fp, fp, i64, i64, fp, fp, i64, i64, i64, i64, fp, C.POINTER(QcStepData),
                                              C.POINTER(QcStepCoefTT), C.c_uint64, C.c_uint64, vp]
    lib.qc_fused_pinn_coef_tt_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepData), C.POINTER(QcStepCoefTT), i32, vp]
    lib.qc_ensemble_strides.argtypes = [C.POINTER(QcStepDesc), i32, C.POINTER(QcStepEnsemble)]
    lib.qc_fused_pinn_ensemble_step.argtypes = [C.POINTER(QcStepDesc), C.POINTER(QcStepEnsemble), i32, vp]
    lib.qc_comm_unique_id.argtypes = [vp]
    lib.qc_comm_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    lib.qc_comm_destroy.argtypes = [vp]
    lib.qc_allreduce_grads.argtypes = [fp, i64, vp, vp]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("qc_error_string", "qc_trig_bytes", "qc_circuit_workspace_bytes", "qc_circuit_workspace_bytes_batch",
                        "qc_step_workspace_bytes", "qc_adapt_bytes", "qc_lbfgs_workspace_bytes"):
            fn.restype = i32
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        lib = load()
        msg = lib.qc_error_string(rc).decode()
        raise QcError(f"{what or 'libqcpinn_hip'} failed: {msg} (code {rc}, hipError {lib.qc_last_hip_error()})")
