// Internal structs and launcher prototypes shared by the translation units of libqcpinn_hip.so.
#pragma once
#include "qc_common.h"

struct QcLayout {  // column offsets of the flat parameter / gradient vector
  int H, n;
  int oW1, ob1, oW2, ob2, oW3, ob3, oW4, ob4, oTh, NP;
};

// K: rows of the last layer (outputs of the post network), W4[K][H] b4[K]; K = 1 is the single-output layout
// n_op: trainable entries behind theta (the inverse step: QC_COEF_N; the balanced step: QC_BAL_N), counted in NP; no offset moves
// n_in: columns of W1: 3 (t, x, y), or 2 m behind a Fourier-feature map of m frequencies (W1[H][2m], sines then cosines)
inline QcLayout qc_layout(int H, int n, int n_theta, int K = 1, int n_op = 0, int n_in = 3) {
  QcLayout L;
  L.H = H;
  L.n = n;
  L.oW1 = 0;
  L.ob1 = n_in * H;
  L.oW2 = L.ob1 + H;
  L.ob2 = L.oW2 + n * H;
  L.oW3 = L.ob2 + n;
  L.ob3 = L.oW3 + H * n;
  L.oW4 = L.ob3 + H;
  L.ob4 = L.oW4 + K * H;
  L.oTh = L.ob4 + K;
  L.NP = L.oTh + n_theta + n_op;
  return L;
}

constexpr int QC_PB_CONVECTION_DIFFUSION = 0, QC_PB_PURE_DIFFUSION = 1,
              QC_PB_GAUSSIAN_PULSE = 2;   // == QC_PROBLEM_* of the public header
constexpr int QC_PB_TABULATED = 3;        // targets read from memory (the *_data entry points), never computed in-kernel

// Targets of the tabulated mode-2 post kernels: one float per point of the batch (value points: IC first, then BC), and
// the zeroth-order coefficient of the residual c_u u + c_t u_t + ... (not part of QcPde, whose layout is public).
struct QcTab {
  const float* tg_res;
  const float* tg_val;
  float c_u;
};

// Per-point operator rows of the coefficient step (qc_post_coef): columns c_u, c_t, c_x, c_y, d_xx, d_yy, c_3, stored
// batch-minor [QC_COEF_COLS][B] next to the residual targets.  == QC_COEF_COLS of the public header.
constexpr int QC_COEF_N = 7;

// The trainable global operator of the inverse step: c_k = fmaf(scale[k], p[k], base[k]) with p the QC_COEF_N flat entries
// behind theta (params[NP_L - 7 ..]); scale[k] = 0 freezes c_k at base[k].  hist / st: tile 0 of a residual launch stores
// the seven c_k it used in hist[(st->step - st->hist_base) * 7 + k] when that row lies in [0, hist_cap); null: no history.
struct QcOptState;
struct QcLearn {
  float base[QC_COEF_N], scale[QC_COEF_N];
  float* hist;
  int hist_cap;
  const QcOptState* st;
};

// Uncertainty balancing of the three loss terms (the balanced step): F = sum_k (w_k e_k L_k + s_k), s_k = scale[k] p[k],
// e_k = exp(-s_k), with p the QC_BAL_N flat entries behind theta (params[NP_B - 3 ..]) in the order of the loss columns:
// residual, BC, IC.  scale[k] = 0 freezes term k (e_k = 1, gradient entry exactly 0).  hist (the optimiser launch only):
// row step - 1 - hist_base of [hist_cap][3] receives the effective weights w_k e_k the step used; null: no history.
constexpr int QC_BAL_N = 3;   // == QC_BAL_TERMS of the public header
struct QcBal {
  float scale[QC_BAL_N];
  float* hist;
  int hist_cap;
};
// THE factor e_k, for the post stage (cotangent scales) and the optimiser launch (gradient entries, F, weight history)
// alike: the precise exponential, so both see the same bits
__device__ __forceinline__ float qc_bal_factor(const float scale, const float p) { return expf(-(scale * p)); }

// Where a post stage takes its targets and its operator from: analytic (functions of X, the operator of QcPde),
// tabulated (tab), tabulated with a coefficient table [QC_COEF_N][B_res] for the residual points (tab.c_u is then not
// read), or tabulated with the trainable global operator `learn` (tab.c_u and the operator of QcPde are not read; the
// layout then counts QC_COEF_N more entries, n_op()), or tabulated with balanced loss weights `bal` (the tabulated kind's
// arithmetic on cotangent scales taken from params; QC_BAL_N more entries).  The post launchers and everything above them
// pass this one value; the kernels receive nothing, tab, tab and coef, tab and learn, or tab and bal as their last arguments.
enum QcTargetKind { QC_TARGET_ANALYTIC = 0, QC_TARGET_TAB, QC_TARGET_COEF, QC_TARGET_LEARN, QC_TARGET_BAL };
struct QcTarget {
  QcTargetKind kind = QC_TARGET_ANALYTIC;
  QcTab tab = {nullptr, nullptr, 0.f};
  const float* coef = nullptr;
  QcLearn learn = {};
  QcBal bal = {};

  static QcTarget tabulated(const float* tg_res, const float* tg_val, float c_u) {
    return {QC_TARGET_TAB, {tg_res, tg_val, c_u}, nullptr, {}, {}};
  }
  static QcTarget with_coef(const float* tg_res, const float* tg_val, const float* coef) {
    return {QC_TARGET_COEF, {tg_res, tg_val, 0.f}, coef, {}, {}};
  }
  static QcTarget learned(const float* tg_res, const float* tg_val, const QcLearn& lr) {
    return {QC_TARGET_LEARN, {tg_res, tg_val, 0.f}, nullptr, lr, {}};
  }
  static QcTarget balanced(const float* tg_res, const float* tg_val, float c_u, const QcBal& bl) {
    return {QC_TARGET_BAL, {tg_res, tg_val, c_u}, nullptr, {}, bl};
  }
  int n_op() const { return kind == QC_TARGET_LEARN ? QC_COEF_N : (kind == QC_TARGET_BAL ? QC_BAL_N : 0); }
  // the value points of a step have no operator: the same targets without the table (a learned operator and balanced
  // weights stay: the value tiles zero those columns in their rows)
  QcTarget value_side() const { return kind == QC_TARGET_COEF ? tabulated(tab.tg_res, tab.tg_val, tab.c_u) : *this; }
  // THE validity rule: a coefficient table needs tabulated targets (it has them by construction), mode 2 and six
  // channels; tabulated targets need mode 2 and problem id 3
  bool ok(int mode, int nch, int problem) const {
    if (kind == QC_TARGET_ANALYTIC) return true;
    if (mode != 2 || problem != QC_PB_TABULATED) return false;
    return kind != QC_TARGET_COEF || (nch == 6 && coef != nullptr);
  }
};

// Where a step's three batches go, and the counters that draw them: the residual rows, then the value rows, IC first and
// BC behind them (X_val, tg_val); off_* is the GLOBAL index of the first point of each batch (data parallelism).  The
// target pointers are null for the coordinate draw, which has no targets to fill.
struct QcBatches {
  float *X_res, *tg_res;
  int64_t n_res, off_res;
  float *X_val, *tg_val;
  int64_t n_ic, off_ic, n_bc, off_bc;
  uint64_t seed, step;
};

// One segment of the tabulated step's resident dataset; it serves a batch that is empty, or with 1 <= n < 2^31 rows.
struct QcDsSeg {
  const float* X;   // [n][3]
  const float* tg;  // [n]
  int64_t n;
  bool serves(int64_t n_batch) const { return n_batch <= 0 || (X && tg && n >= 1 && n < ((int64_t)1 << 31)); }
};

// The operator of the system step as data (== the head of qc_step_system of the public header): K outputs of one shared
// network, n_eq equations, each the sum of its terms  coef * q[out][chan] * (mul0 >= 0 ? u[mul0] : 1) * (mul1 >= 0 ?
// u[mul1] : 1),  q[k][c] channel c of output k and u[k] = q[k][0]; w_eq / w_out weigh the equations in L_r and the
// outputs in L_bc / L_ic.  A kernel argument of k_post_system: the term fields are wave-uniform run-time values.
constexpr int QC_SYS_K = 4, QC_SYS_EQ = 4, QC_SYS_TERMS = 32;   // == QC_KMAX, QC_EQMAX, QC_TERMS_MAX
struct QcSysTerm {
  int eq, out, chan, mul0, mul1;
  float coef;
};
struct QcSys {
  int K, n_eq, n_terms;
  QcSysTerm terms[QC_SYS_TERMS];
  float w_eq[QC_SYS_EQ], w_out[QC_SYS_K];
};

// Where those batches come from: coordinates drawn in the boxes of the three analytic problems (face_pts: the boundary
// faces, from QC_FACE_RANDOM up), rows of a resident dataset drawn uniformly, or the same with the residual row
// drawn from the integer CDF of qc_adapt_build (cdf over cdf_rows rows, coarse table behind it).  With `table` (a
// qc_step_coef was given) a residual point also copies its operator row, ds_coef[idx][QC_COEF_N] -> coef_res.  The
// sampler's launchers and everything above them pass this one value; qc_sample.hip maps it to a kernel.
// QC_SOURCE_SLABS (the causal step): uniform rows with the residual row drawn inside the time slab of the point's tile, slab
// (g / 64) mod n_slabs of the table slab_lo[n_slabs + 1] of row offsets (the residual segment sorted by t).
enum QcSourceKind { QC_SOURCE_DRAW = 0, QC_SOURCE_ROWS, QC_SOURCE_CDF, QC_SOURCE_SLABS };
constexpr int QC_CAUSAL_SLABS = 64;      // == QC_CAUSAL_MAX_SLABS of the public header
constexpr int64_t QC_FACE_RANDOM = -1;   // == QC_BC_RANDOM_FACE of the public header: the smallest face_pts
struct QcSource {
  QcSourceKind kind = QC_SOURCE_DRAW;
  int64_t face_pts = 0;
  QcDsSeg res = {}, ic = {}, bc = {};
  bool table = false;
  float* coef_res = nullptr;
  const float* ds_coef = nullptr;
  const uint64_t *cdf = nullptr, *coarse = nullptr;
  int64_t cdf_rows = 0;
  // target width of a system's dataset (uniform rows only): 0, one float per row; else the rows of the target tables are
  // [w_res] / [w_val] floats, written batch-minor, and the residual table (and the batch's buffer) may be absent
  int w_res = 0, w_val = 0;
  const int64_t* slab_lo = nullptr;   // QC_SOURCE_SLABS
  int n_slabs = 0;

  // THE validity rule, in two steps.  holds(): what a step asks of batches that are already filled (a call without
  // QC_PHASE_SAMPLE asks no more): a known boundary rule; of dataset kinds a split of the value batch, a target buffer
  // behind every non-empty batch, and a CDF buffer that is 8-byte aligned and lies over exactly the rows of the residual
  // segment (1 <= rows < 2^31).
  bool holds(const QcBatches& b) const {
    if (face_pts < QC_FACE_RANDOM) return false;
    if (kind == QC_SOURCE_DRAW) return true;
    if (b.n_ic < 0 || b.n_bc < 0 || (b.n_res > 0 && !b.tg_res && w_res == 0) || (b.n_ic + b.n_bc > 0 && !b.tg_val)) return false;
    return kind != QC_SOURCE_CDF ||
           (cdf && ((uintptr_t)cdf & 7) == 0 && cdf_rows >= 1 && cdf_rows < ((int64_t)1 << 31) && cdf_rows == res.n);
  }
  // ok(): what filling them asks on top: counts and offsets from 0, a point buffer and a dataset segment behind every
  // non-empty batch, and the coefficient pair whole where a table is wanted (n_res = 0: neither pointer is read)
  bool ok(const QcBatches& b) const {
    if (!holds(b) || b.n_res < 0 || b.n_ic < 0 || b.n_bc < 0 || b.off_res < 0 || b.off_ic < 0 || b.off_bc < 0) return false;
    if ((b.n_res > 0 && !b.X_res) || (b.n_ic + b.n_bc > 0 && !b.X_val)) return false;
    if (kind == QC_SOURCE_DRAW) return true;
    if (table && b.n_res > 0 && (!coef_res || !ds_coef)) return false;
    // slabs: a table, a slab count in range, whole tiles of one slab each and as many tiles of every slab
    if (kind == QC_SOURCE_SLABS && (!slab_lo || n_slabs < 2 || n_slabs > QC_CAUSAL_SLABS || table || w_res > 0 || w_val > 0 ||
                                    b.n_res % (64 * (int64_t)n_slabs) != 0 || b.off_res % 64 != 0))
      return false;
    if (w_res > 0 && !res.tg) return QcDsSeg{res.X, res.X, res.n}.serves(b.n_res) && ic.serves(b.n_ic) && bc.serves(b.n_bc);
    return res.serves(b.n_res) && ic.serves(b.n_ic) && bc.serves(b.n_bc);
  }
};

// Residual-adaptive sampling (qc_adapt.hip, the CDF rules of k_gather): the caller's buffer holds this record, then the
// inclusive uint64 CDF of the rows' integer weights, then one coarse entry per QC_ADAPT_ROWS rows (the CDF at the last row
// of each block of rows).  == the layout documented at qc_adapt_bytes in the public header.
constexpr int QC_ADAPT_ROWS = 1024;   // == QC_ADAPT_BLOCK
struct QcAdaptRec {
  uint64_t total, q_sum, add;   // cdf[n - 1]; sum of the quantised powers; the floor term added to every row
  float max_p;                  // M = max_j p_j
  int32_t shift;                // s = 23 - ilogb(M) (0 when M = 0)
  int32_t pad[8];
};

struct QcPde {  // == qc_pde of the public header
  float D, vx, vy;                 // physical constants: analytic targets of mode 2
  float c_t, c_x, c_y, d_xx, d_yy; // operator coefficients (sigma scalings folded in)
  float w_res;
  float inv_n_res;
  float w_val_a, w_val_b;
  float inv_n_a, inv_n_b;
  int problem;
  int64_t n_seg_a;
};

// device-resident optimiser state (64-byte record; host reads it back on demand)
struct QcOptState {
  float lr;
  float best;
  int num_bad;
  int step;  // number of Adam steps taken
  float last_loss;
  float last_norm;
  float loss_parts[3];
  int hist_base;  // steps taken before this history buffer started: the loss of step s goes to hist[s - 1 - hist_base]
  int pad[6];
};

struct QcOptHyper {  // == qc_opt_hyper of the public header
  double beta1, beta2;  // kept in double: torch forms the bias corrections in Python floats
  float eps, max_norm;
  float sched_factor, sched_threshold, sched_min_lr, sched_eps;
  int sched_patience;
  float w_res, w_bc, w_ic;  // loss = w_res*L_r + w_bc*L_bc + w_ic*L_ic   (2, 4, 2)
};

// The head of the L-BFGS workspace (qc_lbfgs.hip; == the 128-byte record documented at qc_lbfgs_step in the public header)
constexpr int QC_LBFGS_REC_WORDS = 32;
struct QcLbfgsRec {
  int phase;            // 0: the next call is a first evaluation; 1: a trial point is pending
  int n_eval, n_iter;   // calls so far; accepted points so far (first evaluations included)
  int n_pairs, head;    // kept pairs; the ring slot the next pair goes to
  int ls_trials;        // rejected trials of the running line search
  int n_rejected, n_skipped_pairs, n_resets, stalled;
  int sd_failed;        // the running search is the steepest-descent restart behind an exhausted one
  int NP, history, accepted;
  int pad0[2];
  float t, f0, gtd0, gamma;   // step of the pending trial; loss and g.d at x_k; y.s / y.y of the newest kept pair
  float f, loss_parts[3];     // of the last call
  float t_led;                // the step that led from x_k to the pending point (0: the point is x_k itself)
  float pad1[7];
};
static_assert(sizeof(QcLbfgsRec) == 4 * QC_LBFGS_REC_WORDS, "L-BFGS record");

struct QcLbfgsHyper {  // == qc_lbfgs_hyper of the public header
  int history, line_search, max_ls;
  float lr, c1, shrink_lo, shrink_hi, curv_eps;
  float w_res, w_bc, w_ic;
};

// ---- circuit families: one record per kernel family, chosen once per program (qc_program_create)
// Scratch and kept final states of one pipeline.  HBM family: `p`/`bytes` is the scratch, `keep` keeps every tile
// resident from the forward pass to the adjoint pass of the same batch.  Register and wave families: `p` is the store
// of the forward pass's final states when `keep` is set, else ignored (the adjoint pass recomputes them).
struct QcCircStore {
  void* p;
  size_t bytes;
  bool keep;
};
// `nch` = 1: expectation values of the angles (value pipeline); 6: jets of the angles (residual pipeline).
struct QcFamily {
  int (*fwd)(const qc_program*, const QcTrig*, const float* umat, const float* in, float* out, int64_t B, int nch,
             QcCircStore, hipStream_t);
  int (*bwd)(const qc_program*, const QcTrig*, const float* umat, const float* in, const float* cot, float* d_in,
             float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, QcCircStore, hipStream_t);
  size_t (*store_bytes)(const qc_program*, int nch, int64_t B);   // what `keep` needs; 0 = this family keeps nothing
};
// (not `const`: a const global with a constant initializer would be emitted for the device as well, where the host
// launchers it points to do not exist)
extern QcFamily qc_family_reg;    // registers, one lane per statevector: 2 <= n <= 5 (qc_circuit_reg.hip)
extern QcFamily qc_family_wave;   // lanes as amplitudes: n = 1, 6..8 (qc_circuit_wave.hip)
extern QcFamily qc_family_hbm;    // statevector tiles in HBM: n = 9..20 (qc_circuit_hbm2.hip)
extern QcFamily qc_family_reup;   // programs with EMBED gates (data re-uploading): 2 <= n <= 5 (qc_circuit_reup.hip)

// the generated program whose rows (n_gates x (op, ba, bb, slot), device encoding) are this program's gates;
// never with QC_NO_STATIC=1 (read once)
bool qc_static_match(const qc_program* pg, int n_qubits, int n_gates, const int* rows);
int qc_reg_match_static(const qc_program* pg);
int qc_wave_match_static(const qc_program* pg);
// merged residual + value stages of the fused step (register family only)
int qc_reg_circ_fwd_both(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, float* qjets,
                         int64_t Br, float* chi_store, const float* angles, float* expval, int64_t Bv, hipStream_t st);
int qc_reg_circ_bwd_both(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets,
                         const float* qbar, float* abar, int64_t row0_r, int64_t Br, const float* chi_store,
                         const float* angles, const float* cot, float* d_angles, int64_t row0_v, int64_t Bv, float* part,
                         int64_t part_stride, hipStream_t st);

// ---- launchers, one group per .hip file
// `map`: output map of the pre network (QC_ANGLE_MAP_*); its reverse pass reads the forward pass's angle jets aj / ajr / ajv
int qc_mlp_pre_fwd_both(const QcBatches& b, int draw, int64_t face_pts, const float* prm, QcLayout L, float* ajr, float* ajv,
                        hipStream_t st, int map);
int qc_mlp_pre_bwd_both(const float* Xr, const float* Xv, const float* prm, QcLayout L, const float* abr, const float* abv,
                        float* part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br, int64_t Bv,
                        hipStream_t st, int map, const float* ajr, const float* ajv);
// `tg` (both post launchers, checked with QcTarget::ok): the tabulated kinds select the kernels that read their targets
// from memory; with a coefficient table ubr / out_u is a [6][B] cotangent scratch and rbr / out_res is not used
int qc_mlp_post_both(const float* prm, QcLayout L, QcPde pde, const float* Xr, const float* qjr, float* ubr, float* rbr,
                     float* qbr, int64_t row0_r, int64_t Br, const float* Xv, const float* qjv, float* ubv, float* qbv,
                     int64_t row0_v, int64_t Bv, float* part, int64_t part_stride, hipStream_t st,
                     const QcTarget& tg);
int qc_mlp_pre_fwd(const float* X, const float* prm, QcLayout L, float* ajets, int64_t B, int nch, hipStream_t,
                   int map = 0);
int qc_mlp_pre_bwd(const float* X, const float* prm, QcLayout L, const float* abar, float* part,
                   int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t, int map = 0,
                   const float* aj = nullptr);
int qc_mlp_post(int mode, const float* X, const float* prm, QcLayout L, QcPde pde, const float* qjets,
                float* out_u, float* out_res, const float* in_ubar, const float* in_rbar, float* qbar,
                float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t,
                const QcTarget& tg);
// The pre stages behind a Fourier-feature input map (freq: [3][m] on the device, 1 <= m <= QC_FF_MAX; L laid out with
// n_in = 2 m): the same arguments as the plain launchers, which serve the programs without a map
int qc_mlp_pre_ff_fwd(const float* X, const float* prm, QcLayout L, float* ajets, int64_t B, int nch, hipStream_t, int map,
                      const float* freq, int m);
int qc_mlp_pre_ff_bwd(const float* X, const float* prm, QcLayout L, const float* abar, float* part, int64_t part_stride,
                      int64_t row0, int64_t B, int nch, hipStream_t, int map, const float* aj, const float* freq, int m);
int qc_mlp_pre_ff_fwd_both(const QcBatches& b, int draw, int64_t face_pts, const float* prm, QcLayout L, float* ajr, float* ajv,
                           hipStream_t st, int map, const float* freq, int m);
int qc_mlp_pre_ff_bwd_both(const float* Xr, const float* Xv, const float* prm, QcLayout L, const float* abr, const float* abv,
                           float* part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br, int64_t Bv,
                           hipStream_t st, int map, const float* ajr, const float* ajv, const float* freq, int m);
// the system post stage (k_post_system): forward, terms, loss columns, cotangents and reverse of one batch in one kernel;
// L is the K-row layout; nch = 6: tg = [n_eq][B] residual targets or null (zero); nch = 1: tg = [K][B] value targets
int qc_mlp_post_system(const float* prm, QcLayout L, const QcSys& sys, QcPde pde, const float* qjets, const float* tg,
                       float* qbar, float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t);
int qc_mlp_post_multi(int mode, const float* prm, QcLayout L, int K, const float* w4k, const float* qjets, float* out_u,
                      const float* ubar, float* qbar, float* part, int64_t part_stride, float* partk, int64_t partk_stride,
                      int64_t row0, int64_t B, hipStream_t);
int qc_opt_reduce_rows(const float* part, int64_t rows, int64_t stride, int ncols, float* out, hipStream_t);
int qc_opt_fold_rows(float* part, int64_t rows, int64_t stride, int ncols, hipStream_t);
// `bal` (both optimiser launchers; the balanced step): NP counts its QC_BAL_N entries, whose gradients are formed in the
// launch from the loss columns; null: the plain update
int qc_opt_adam_fold(const float* part, int64_t stride, int RS, float* flat, int NP, float* prm, float* m, float* v,
                     QcOptState* state, QcOptHyper hp, float* hist, int hist_cap, const qc_program* pg, int theta_off,
                     QcTrig* trig, hipStream_t, const QcBal* bal = nullptr);
int qc_opt_adam(float* flat, int NP, float* prm, float* m, float* v, QcOptState* state, QcOptHyper hp,
                float* hist, int hist_cap, const qc_program* pg, int theta_off, QcTrig* trig, hipStream_t,
                const QcBal* bal = nullptr);
int qc_opt_prep_trig(const qc_program* pg, const float* theta, QcTrig* trig, hipStream_t);
// Causal weighting (the causal step).  rec: the device record {float eps; int n_raised, n_steps, hist_base; float W[M], L[M]}
// (== the layout documented at qc_step_causal in the public header); tile_off: the global tile index of row 0, mod M.
constexpr int QC_CAUSAL_HEAD = 4;
struct QcCausal {
  int M, tile_off;
  float growth, eps_max, delta;
  float* rec;
  float* hist;
  int hist_cap;
};
int qc_opt_causal_init(float* rec, int M, float eps0, hipStream_t);
// weights from column ncols - 3 of rows [0, rows_res), then qc_opt_fold_rows with residual row r scaled by its slab's weight
int qc_opt_causal_fold(float* part, int64_t rows, int64_t rows_res, int64_t stride, int ncols, const QcCausal& cz, hipStream_t);
// Gradient-norm loss weights (the gradient-norm step).  rec: the device record of QC_GRADNORM_WORDS 4-byte words {float
// lam_bc, lam_ic; int n_steps, hist_base, n_updates; float m_r, a_bc, a_ic, hat_bc, hat_ic; 0 ..} (== the layout
// documented at qc_step_gradnorm in the public header); w: the loss weights of the lambda-weighted loss in the history row.
constexpr int QC_GRADNORM_WORDS = 16, QC_GRADNORM_COLS = 7;
struct QcGradnorm {
  float alpha, lam_max;
  int every;
  float w[3];   // residual, BC, IC
  float* rec;
  float* hist;
  int hist_cap;
};
int qc_opt_gradnorm_init(float* rec, float lam_bc, float lam_ic, hipStream_t);
// The three row classes of a partial-row matrix: residual rows [0, n_res), IC rows behind them, BC rows behind those.  The
// class fold (in place, every class like qc_opt_fold_rows on its own rows), then the single-block launch that forms the
// class sums, moves the weights and writes flat[ncols] = [G_res + lam_bc G_bc + lam_ic G_ic | L_r, L_bc, L_ic];
// class_out: [3][ncols] (G_res, G_ic, G_bc) or null.
int qc_opt_gradnorm_fold(float* part, int64_t n_res, int64_t n_ic, int64_t n_bc, int64_t stride, int ncols, const QcGradnorm& gn,
                         float* flat, float* class_out, hipStream_t);
// qc_lbfgs.hip: floats of a workspace; zero it and write its record; make the next call a first evaluation; one call
size_t qc_lbfgs_words(int NP, int m);
int qc_lbfgs_init_launch(void* ws, int NP, int m, hipStream_t);
int qc_lbfgs_restart_launch(void* ws, int keep, hipStream_t);
int qc_lbfgs_step_launch(const float* flat, int NP, float* prm, void* ws, QcLbfgsHyper hp, float* hist, int hist_cap,
                         const qc_program* pg, int theta_off, QcTrig* trig, hipStream_t);
// qc_sample.hip: fill the batches `b` from a source that QcSource::ok passed: the coordinate draw, or the dataset kinds
int qc_sample_launch(const QcBatches& b, int64_t bc_face_points, hipStream_t);
int qc_gather_launch(const QcBatches& b, const QcSource& s, hipStream_t);
// qc_adapt.hip: |res - target| of c rows from their [6][c] channels (coef_rows [c][7] or null: the scalar operator), and
// scores -> record, CDF and coarse table
int qc_adapt_score_launch(const float* uj, int64_t c, QcPde pde, float c_u, const float* coef_rows, const float* tg,
                          float* score, hipStream_t);
int qc_adapt_build_launch(const float* score, int64_t n, int power, float floor_c, void* adapt, hipStream_t);
// HBM family, n >= 9 (qc_circuit_hbm2.hip, qc_circuit_h2s_kernels.h): all tiles of a batch resident when the workspace allows
void* qc_h2_create(const qc_program* pg, int absorb, int amplitude);   // amplitude: the encoding the plan is built for
void qc_h2_destroy(void* h2);
int qc_h2_describe_gates(const QcGate* gates, int n_gates, int n_qubits, int absorb, int32_t* out, int cap);   // host only
size_t qc_h2_bytes(const qc_program* pg, void* h2, int nch, bool backward, int64_t tiles);
int64_t qc_h2_tiles_that_fit(const qc_program* pg, void* h2, int nch, bool backward, size_t ws_bytes);
int qc_comm_allreduce(float* buf, int64_t count, void* comm, hipStream_t st);   // qc_comm.hip: RCCL sum, fp32, in place
int qc_amp_fwd_launch(const float* a, float* u, int n, int64_t B, int nch, hipStream_t);
int qc_amp_bwd_launch(const float* a, const float* ub, float* ab, int n, int64_t B, int nch, hipStream_t);
// ---- seven derivative channels (channel 6 = d2/dt2), 2 <= n <= 5: jets [7][n][B], operator rows [QC_COEF_TT_N][B]
constexpr int QC_NCH_TT_N = 7;    // == QC_NCH_TT of the public header
constexpr int QC_COEF_TT_N = 8;   // == QC_COEF_TT_COLS: the QC_COEF_N columns, then d_tt
// qc_tt.hip: the pre network (plain inputs, no angle map) and the post network; QC_ERR_UNSUPPORTED outside 2 <= L.n <= 5.
// qc_tt_post mode 2: the coefficient form (io = the [7][B] channel cotangents, written); 3: the reverse pass from given
// cotangents io[7][B]; 4: forward only, io = the seven channels of u
int qc_tt_pre_fwd(const float* X, const float* prm, QcLayout L, float* ajets, int64_t B, hipStream_t);
int qc_tt_pre_bwd(const float* X, const float* prm, QcLayout L, const float* abar, float* part, int64_t part_stride,
                  int64_t row0, int64_t B, hipStream_t);
int qc_tt_post(int mode, const float* prm, QcLayout L, QcPde pde, const float* qjets, const float* target, const float* coef,
               float* io, float* qbar, float* part, int64_t part_stride, int64_t row0, int64_t B, hipStream_t);
// qc_circuit_tt.hip: the register family's interpreter kernels with seven waves (angle encoding, no EMBED gates)
int qc_tt_circ_fwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, float* qjets, int64_t B,
                   hipStream_t);
int qc_tt_circ_bwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, const float* qbar,
                   float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B, hipStream_t);

// ---- ensembles: M independent models per launch (qc_fused_pinn_ensemble_step).  Every per-model buffer of the step is M
// consecutive slices; these are the distances between them, in floats except trig and ws (bytes).  A stage's ensemble
// kernel has the grid (tiles of one member, M): it offsets its pointers by blockIdx.y slices with scalar arithmetic and
// calls the single-model body.  pde / hyper: device tables of M records, or null (every member takes the launch's own).
struct QcEns {
  int M;
  int64_t prm, flat, hist, trig, X_res, X_val, jets_res, jets_val, part, ws;
  const QcPde* pde;
  const QcOptHyper* hyper;
};
// record m of a device table, through the constant address space: m is wave-uniform (a block index), so the record arrives
// by scalar loads
template <class T>
__device__ __forceinline__ T qc_ens_record(const T* table, const int m) {
  static_assert(sizeof(T) % 4 == 0 && alignof(T) >= 4, "whole words");
  T r;
#if defined(__HIP_DEVICE_COMPILE__)
  const auto* w = (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)(table + m);
#else
  const uint32_t* w = (const uint32_t*)(table + m);
#endif
  uint32_t* o = (uint32_t*)&r;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); ++i) o[i] = w[i];
  return r;
}
// the stage launchers: the arguments of the merged single-model launchers (member 0's slices) and the strides
int qc_mlp_pre_fwd_ens(const QcBatches& b, int draw, int64_t face_pts, const float* prm, QcLayout L, float* ajr, float* ajv,
                       hipStream_t st, int map, const QcEns& e);
int qc_mlp_post_ens(const float* prm, QcLayout L, QcPde pde, const float* Xr, const float* qjr, float* ubr, float* rbr, float* qbr,
                    int64_t row0_r, int64_t Br, const float* Xv, const float* qjv, float* ubv, float* qbv, int64_t row0_v,
                    int64_t Bv, float* part, int64_t part_stride, hipStream_t st, const QcEns& e);
int qc_mlp_pre_bwd_ens(const float* Xr, const float* Xv, const float* prm, QcLayout L, const float* abr, const float* abv,
                       float* part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br, int64_t Bv, hipStream_t st,
                       int map, const float* ajr, const float* ajv, const QcEns& e);
bool qc_mlp_ens_ok(const QcLayout& L);   // the fused post kernel serves this hidden width
int qc_reg_circ_fwd_ens(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, float* qjets,
                        int64_t Br, float* chi_store, const float* angles, float* expval, int64_t Bv, hipStream_t st,
                        const QcEns& e);
int qc_reg_circ_bwd_ens(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, const float* qbar,
                        float* abar, int64_t row0_r, int64_t Br, const float* chi_store, const float* angles, const float* cot,
                        float* d_angles, int64_t row0_v, int64_t Bv, float* part, int64_t part_stride, hipStream_t st,
                        const QcEns& e);
// the tail, one block per member: rows of the member's partial-row matrix -> flat [gradient | 3 loss sums]; with `update`
// then adam_block on the member's slices and state record (hp: every member's without a table); rows = 0: flat is given
int qc_opt_ens_tail(float* part, int64_t rows, int64_t stride, float* flat, int NP, float* prm, float* m, float* v,
                    QcOptState* state, QcOptHyper hp, float* hist, int hist_cap, const qc_program* pg, int theta_off,
                    QcTrig* trig, int update, const QcEns& e, hipStream_t);
