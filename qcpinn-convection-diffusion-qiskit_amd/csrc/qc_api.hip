// extern "C" entry points of libqcpinn_hip.so (declared in include/qcpinn_hip.h).
// Argument checking happens here, once, on the host: the kernels assume validated shapes.
#include "qc_internal.h"
#include "qc_wave_sched.h"
#include "../../include/qcpinn_hip.h"

#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

static_assert(sizeof(QcPde) == sizeof(qc_pde), "qc_pde layout");
static_assert(QC_PB_CONVECTION_DIFFUSION == QC_PROBLEM_CONVECTION_DIFFUSION && QC_PB_PURE_DIFFUSION == QC_PROBLEM_PURE_DIFFUSION &&
              QC_PB_GAUSSIAN_PULSE == QC_PROBLEM_GAUSSIAN_PULSE && QC_PB_TABULATED == QC_PROBLEM_TABULATED, "problem ids");
static_assert(QC_COEF_N == QC_COEF_COLS, "coefficient columns");
static_assert(QC_FACE_RANDOM == QC_BC_RANDOM_FACE, "boundary rule");
static_assert(sizeof(QcOptHyper) == sizeof(qc_opt_hyper), "qc_opt_hyper layout");
static_assert(QC_SYS_K == QC_KMAX && QC_SYS_EQ == QC_EQMAX && QC_SYS_TERMS == QC_TERMS_MAX, "system limits");
static_assert(sizeof(QcSysTerm) == sizeof(qc_sys_term) && ((sizeof(QcSys) + 7) & ~(size_t)7) == offsetof(qc_step_system, target_res_dev),
              "qc_step_system head");

static thread_local int g_last_hip = 0;

static inline int hip_fail(hipError_t e) {
  g_last_hip = (int)e;
  return QC_ERR_HIP;
}
static inline int after_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? QC_OK : hip_fail(e);
}

static QcLayout make_layout(int H, int n, int n_theta) { return qc_layout(H, n, n_theta); }
// columns of W1 in the flat vector of the network in front of this program: 2 m behind a Fourier-feature map, else 3
static int prog_n_in(const qc_program* p) { return p->ff_m > 0 ? 2 * p->ff_m : 3; }
static_assert(QC_FF_MAX == 64, "the trig rows of a tile at QC_FF_MAX (32 KB) are sized into the stages' LDS budget");
static QcPde to_pde(const qc_pde* p) {
  QcPde q;
  memcpy(&q, p, sizeof(q));
  return q;
}

// Which kernel family serves n qubits: registers (one lane per statevector) up to 5, lanes-as-amplitudes up to 8,
// statevector tiles in HBM up to 20 (the round-structured plan of qc_circuit_hbm2.hip; compile-time stage programs
// where one is registered, the plan interpreter with QC_NO_STATIC=1).  QC_FORCE_WAVE=1 is a test hook: it routes
// n <= 5 through the wave family too (cross-checks the two families).
static const QcFamily* pick_family(int n) {
  static const bool force_wave = [] { const char* e = getenv("QC_FORCE_WAVE"); return e && e[0] == '1'; }();
  if (n >= 2 && n <= 5 && !force_wave) return &qc_family_reg;
  if (n >= 1 && n <= 8) return &qc_family_wave;
  if (n >= 9 && n <= 20) return &qc_family_hbm;
  return nullptr;
}
// Budget of the resident per-tile stores: QC_HBM_KEEP_GB (default 96), never more than 85 % of the memory that is free
// on the current device when a workspace is sized (a smaller or partly occupied GPU gets fewer resident tiles, not an
// allocation failure).
static inline double hbm_budget_bytes() {
  static const double cap_gb = [] { const char* e = getenv("QC_HBM_KEEP_GB"); return e ? atof(e) : 96.0; }();
  double b = cap_gb * 1073741824.0;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
    const double avail = 0.85 * (double)free_b;
    if (avail < b) b = avail;
  }
  return b;
}

// A side stream per device so the (small) boundary/initial-value pipeline of a step can overlap the
// residual pipeline; created once, on first use, never inside a graph capture of the caller.
struct QcSide {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool ok = false, tried = false;
};
static QcSide* side_stream() {
  static QcSide tab[64];
  static std::mutex mu;
  static const bool off = [] { const char* e = getenv("QC_NO_OVERLAP"); return e && e[0] == '1'; }();
  if (off) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  QcSide& q = tab[dev];
  if (!q.tried) {
    q.tried = true;
    q.ok = hipStreamCreateWithFlags(&q.s, hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&q.fork, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&q.join, hipEventDisableTiming) == hipSuccess;
  }
  return q.ok ? &q : nullptr;
}
// fork: the stream the value pipeline runs on, the side stream behind an event of `st`; without one (`side` is then
// null) `st` itself.  join: `st` waits for what the side stream was given since.
static hipStream_t side_fork(QcSide*& side, hipStream_t st) {
  if (side && hipEventRecord(side->fork, st) == hipSuccess && hipStreamWaitEvent(side->s, side->fork, 0) == hipSuccess)
    return side->s;
  side = nullptr;
  return st;
}
static int side_join(QcSide* side, hipStream_t st) {
  if (!side) return QC_OK;
  hipError_t e = hipEventRecord(side->join, side->s);
  if (e == hipSuccess) e = hipStreamWaitEvent(st, side->join, 0);
  return e == hipSuccess ? QC_OK : hip_fail(e);
}

bool qc_static_match(const qc_program* pg, int n_qubits, int n_gates, const int* rows) {
  static const bool off = [] { const char* e = getenv("QC_NO_STATIC"); return e && e[0] == '1'; }();
  if (off || n_qubits != pg->n_qubits || n_gates != pg->n_gates) return false;
  for (int g = 0; g < n_gates; ++g) {
    const QcGate& a = pg->h_gates[g];
    const int* b = rows + 4 * g;
    if (a.op != b[0] || a.ba != b[1] || a.bb != b[2] || a.slot != b[3]) return false;
  }
  return true;
}

extern "C" {

int qc_version(void) { return QC_ABI_VERSION; }

const char* qc_error_string(int code) {
  switch (code) {
    case QC_OK: return "ok";
    case QC_ERR_ARG: return "invalid argument";
    case QC_ERR_UNSUPPORTED: return "unsupported shape (qubit count / hidden width outside the built kernels)";
    case QC_ERR_HIP: return "HIP runtime error (see qc_last_hip_error)";
    case QC_ERR_ALLOC: return "allocation failed";
    default: return "unknown error";
  }
}

int qc_last_hip_error(void) { return g_last_hip; }

// gate rows (opcode, wire_a, wire_b, slot) -> bit-indexed gates; returns false on an invalid row.  EMBED rows
// (wire, -1, -1) and EMBED_S rows (wire, -1, slot) are valid only for a caller that counts them (n_embed_out): the plan
// describers never see one
static bool parse_rows(const int32_t* rows, int n_gates, int n_qubits, int n_params, QcGate* h, int* n_u4_out,
                       int* n_embed_out = nullptr, int* scaled_out = nullptr) {
  int n_u4 = 0, n_embed = 0, scaled = 0;
  for (int g = 0; g < n_gates; ++g) {
    const int op = rows[4 * g], a = rows[4 * g + 1], b = rows[4 * g + 2], slot = rows[4 * g + 3];
    bool ok = op >= QC_RX && op <= QC_EMBED_S && a >= 0 && a < n_qubits;
    if (op == QC_EMBED) {
      ok = ok && n_embed_out != nullptr && b == -1 && slot == -1;
      ++n_embed;
    }
    if (op == QC_EMBED_S) {   // the scaling is a parameter: a slot is required
      ok = ok && n_embed_out != nullptr && scaled_out != nullptr && b == -1 && slot >= 0 && slot < n_params;
      ++n_embed;
      scaled = 1;
    }
    const bool two = (op == QC_CNOT || op == QC_CRX || op == QC_CRZ || op == QC_U4);
    if (two) ok = ok && b >= 0 && b < n_qubits && b != a;
    const bool par = (op == QC_RX || op == QC_RY || op == QC_RZ || op == QC_CRX || op == QC_CRZ);
    if (par) ok = ok && slot >= 0 && slot < n_params;
    if (op == QC_U4) {  // the kernels hard-wire slot 0 = wires [0,1], slot 1 = wires [2,3]
      ok = ok && n_qubits >= 4 && ((slot == 0 && a == 0 && b == 1) || (slot == 1 && a == 2 && b == 3));
      ++n_u4;
    }
    if (!ok) return false;
    h[g].op = op;
    h[g].ba = n_qubits - 1 - a;
    h[g].bb = two ? n_qubits - 1 - b : -1;
    h[g].slot = (par || op == QC_U4 || op == QC_EMBED_S) ? slot : -1;
  }
  *n_u4_out = n_u4;
  if (n_embed_out) *n_embed_out = n_embed;
  if (scaled_out) *scaled_out = scaled;
  return true;
}
// RX(p_w) right after the embedding RX(a_w), wire by wire, distinct slots
static int detect_lead_rx(const QcGate* h, int n_gates, int n_qubits) {
  if (n_gates < n_qubits) return 0;
  for (int g = 0; g < n_qubits; ++g)
    if (h[g].op != QC_RX || h[g].ba != n_qubits - 1 - g || h[g].slot < 0) return 0;
  for (int g = 0; g < n_qubits; ++g)
    for (int k = 0; k < g; ++k)
      if (h[k].slot == h[g].slot) return 0;
  return 1;
}
static bool absorb_enabled() {
  static const bool no_absorb = [] { const char* e = getenv("QC_NO_ABSORB"); return e && e[0] == '1'; }();
  return !no_absorb;
}

// the staged plan folds the leading RX layer only for angle encoding (the generated programs embed angles)
static void* h2_plan(const qc_program* p, int amplitude) {
  return qc_h2_create(p, (p->lead_rx && !amplitude && absorb_enabled()) ? 1 : 0, amplitude);
}

int qc_program_create(const int32_t* rows, int n_gates, int n_qubits, int n_params, qc_program** out) {
  if (!rows || !out || n_gates <= 0 || n_qubits < 1 || n_qubits > 24 || n_params < 0) return QC_ERR_ARG;
  qc_program* p = (qc_program*)calloc(1, sizeof(qc_program));
  QcGate* h = (QcGate*)malloc(sizeof(QcGate) * n_gates);
  if (!p || !h) {
    free(h);
    free(p);
    return QC_ERR_ALLOC;
  }
  p->n_qubits = n_qubits; p->n_gates = n_gates; p->n_params = n_params;
  p->h_gates = h;
  if (!parse_rows(rows, n_gates, n_qubits, n_params, h, &p->n_u4, &p->n_embed, &p->embed_scaled)) {
    qc_program_destroy(p);
    return QC_ERR_ARG;
  }
  if (p->n_embed > 0) {
    // data re-uploading: its own family for 2 <= n <= 5 (whatever QC_FORCE_WAVE says), no family otherwise - no other
    // interpreter knows the opcode.  No compile-time program, no folded leading RX layer.
    p->fam = (n_qubits >= 2 && n_qubits <= 5) ? &qc_family_reup : nullptr;
    p->static_id = -1;
  } else {
    p->fam = pick_family(n_qubits);
    p->static_id = (n_qubits >= 2 && n_qubits <= 5) ? qc_reg_match_static(p)
                   : ((n_qubits >= 6 && n_qubits <= 8) ? qc_wave_match_static(p) : -1);
  }
  qc_find_diag_runs(p);
  p->lead_rx = p->n_embed > 0 ? 0 : detect_lead_rx(h, n_gates, n_qubits);
  hipError_t e = hipMalloc((void**)&p->d_gates, sizeof(QcGate) * n_gates);
  if (e == hipSuccess) e = hipMemcpy(p->d_gates, h, sizeof(QcGate) * n_gates, hipMemcpyHostToDevice);
#ifndef QC_WAVE_NO_RUNS
  if (e == hipSuccess && n_qubits >= 6 && n_qubits <= 8 && p->static_id >= 0) {
    // the compile-time program of this gate list multiplies by one phase table per RZ run: the same schedule, evaluated
    // here, names the gates behind each table for the kernels that (re)build the trig buffer
    const QcWaveSched ws = qc_wave_schedule(h, n_gates, n_qubits);
    if (ws.n_runs > 0) {
      const int ne = ws.run_off[ws.n_runs];
      e = hipMalloc((void**)&p->d_diag_list, sizeof(int) * ne);
      if (e == hipSuccess) e = hipMemcpy(p->d_diag_list, ws.entry, sizeof(int) * ne, hipMemcpyHostToDevice);
      p->n_diag_runs = ws.n_runs;
      for (int r = 0; r < ws.n_runs; ++r) {
        p->diag_g0[r] = ws.run_off[r];
        p->diag_g1[r] = ws.run_off[r + 1];
      }
    }
  }
#endif
  int rc = e == hipSuccess ? QC_OK : hip_fail(e);
  if (rc == QC_OK && p->fam == &qc_family_hbm && !(p->h2 = h2_plan(p, 0))) rc = QC_ERR_ALLOC;
  if (rc != QC_OK) {
    qc_program_destroy(p);
    return rc;
  }
  *out = p;
  return QC_OK;
}

int qc_program_destroy(qc_program* p) {
  if (!p) return QC_ERR_ARG;
  if (p->h2) qc_h2_destroy(p->h2);
  if (p->d_gates) (void)hipFree(p->d_gates);
  if (p->d_diag_list) (void)hipFree(p->d_diag_list);
  if (p->d_ff_freq) (void)hipFree(p->d_ff_freq);
  free(p->h_gates);
  free(p);
  return QC_OK;
}

int qc_program_set_encoding(qc_program* p, int amplitude) {
  if (!p || (amplitude != 0 && amplitude != 1)) return QC_ERR_ARG;
  if (amplitude && ((int64_t)1 << p->n_qubits) < p->n_qubits) return QC_ERR_ARG;
  if (amplitude && p->n_embed > 0) return QC_ERR_UNSUPPORTED;   // no angle to re-upload
  if (p->amplitude != amplitude && p->h2) {   // a plan for the new encoding first; the program changes only with it
    void* h2 = h2_plan(p, amplitude);
    if (!h2) return QC_ERR_ALLOC;
    qc_h2_destroy(p->h2);
    p->h2 = h2;
  }
  p->amplitude = amplitude;
  return QC_OK;
}

static bool angle_map_ok(int m) { return m == QC_ANGLE_MAP_NONE || m == QC_ANGLE_MAP_TANH_PI; }
static bool problem_ok(int pb) { return pb >= QC_PROBLEM_CONVECTION_DIFFUSION && pb <= QC_PROBLEM_GAUSSIAN_PULSE; }
int qc_program_set_angle_map(qc_program* p, int angle_map) {
  if (!p || !angle_map_ok(angle_map)) return QC_ERR_ARG;
  p->angle_map = angle_map;
  return QC_OK;
}

// The Fourier-feature input map of the pre network in front of this program.  Both encodings: with amplitude encoding
// the pre stage goes through the same launchers (pipe_forward).  The program changes only when the copy has succeeded.
int qc_program_set_input_map(qc_program* p, const float* freq_host, int m) {
  if (!p || m < 0 || m > QC_FF_MAX || (m > 0 && !freq_host)) return QC_ERR_ARG;
  float* d = nullptr;
  if (m > 0) {
    for (int i = 0; i < 3 * m; ++i)
      if (!isfinite(freq_host[i])) return QC_ERR_ARG;
    hipError_t e = hipMalloc((void**)&d, sizeof(float) * 3 * m);
    if (e != hipSuccess) return QC_ERR_ALLOC;
    e = hipMemcpy(d, freq_host, sizeof(float) * 3 * m, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return hip_fail(e);
    }
  }
  if (p->d_ff_freq) (void)hipFree(p->d_ff_freq);
  p->d_ff_freq = d;
  p->ff_m = m;
  return QC_OK;
}

int qc_amp_forward(const float* ajets, float* ujets, int n, int64_t B, int nch, void* stream) {
  if (!ajets || !ujets || n < 1 || n > 24 || B <= 0 || (nch != 1 && nch != 6)) return QC_ERR_ARG;
  qc_amp_fwd_launch(ajets, ujets, n, B, nch, (hipStream_t)stream);
  return after_launch();
}

int qc_amp_backward(const float* ajets, const float* ubar, float* abar, int n, int64_t B, int nch, void* stream) {
  if (!ajets || !ubar || !abar || n < 1 || n > 24 || B <= 0 || (nch != 1 && nch != 6)) return QC_ERR_ARG;
  qc_amp_bwd_launch(ajets, ubar, abar, n, B, nch, (hipStream_t)stream);
  return after_launch();
}

size_t qc_trig_bytes(const qc_program* p) {
  return p ? sizeof(QcTrig) * ((size_t)p->n_gates + (size_t)p->n_diag_runs * ((size_t)1 << p->n_qubits)) : 0;
}

int qc_prepare_gates(const qc_program* p, const float* theta, void* trig, void* stream) {
  if (!p || !trig || (p->n_params > 0 && !theta)) return QC_ERR_ARG;
  qc_opt_prep_trig(p, theta, (QcTrig*)trig, (hipStream_t)stream);
  return after_launch();
}

static int check_circuit(const qc_program* p, const void* trig, const float* umat, int64_t B) {
  if (!p || !trig || B <= 0) return QC_ERR_ARG;
  if (p->n_u4 > 0 && !umat) return QC_ERR_ARG;
  if (!p->fam) return QC_ERR_UNSUPPORTED;
  return QC_OK;
}

size_t qc_circuit_workspace_bytes(const qc_program* p, int nch, int backward) {
  if (!p || p->fam != &qc_family_hbm || (nch != 1 && nch != 6)) return 0;
  return qc_h2_bytes(p, p->h2, nch, backward != 0, 1);
}

size_t qc_circuit_workspace_bytes_batch(const qc_program* p, int nch, int backward, int64_t B) {
  if (!p || B <= 0 || p->fam != &qc_family_hbm || (nch != 1 && nch != 6)) return 0;
  const int64_t tiles = qc_ceil_div(B, 64);
  const size_t all = qc_h2_bytes(p, p->h2, nch, backward != 0, tiles);
  if ((double)all <= hbm_budget_bytes()) return all;
  int64_t fit = qc_h2_tiles_that_fit(p, p->h2, nch, backward != 0, (size_t)hbm_budget_bytes());
  return qc_h2_bytes(p, p->h2, nch, backward != 0, fit < 1 ? 1 : fit);
}

static size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

// The workspace of one fused step, every piece 256-byte aligned:
//   [ circuit region | amplitude encoding: u_res | ub_res | u_val | ub_val ]
// The circuit region holds the residual pipeline's store, then the value pipeline's.  Register / wave family: the kept
// final states (optional: without them the adjoint pass recomputes; the value store only behind a residual store).
// HBM family: the resident tiles of both pipelines when the budget holds them all; otherwise as many six-channel tiles
// as it holds, shared by both pipelines (one launch sequence per group of resident tiles, the adjoint pass recomputes
// its group's forward pass); never less than one tile.  Called without a workspace it also sizes one.
struct QcStepLayout {
  size_t bytes;                             // (called without a workspace) what the whole workspace should hold
  bool fits;                                // the workspace holds what the family cannot do without (HBM: one tile)
  QcCircStore res, val;                     // circuit stores of the residual (six-channel) and value pipelines
  float *u_res, *ub_res, *u_val, *ub_val;   // amplitude encoding: initial-amplitude jets and their cotangents
};
static QcStepLayout step_layout(const qc_program* p, int64_t B_res, int64_t B_val, void* ws, size_t ws_bytes) {
  const QcFamily* f = p->fam;
  const bool hbm = f == &qc_family_hbm;
  const size_t rs = f ? round256(f->store_bytes(p, 6, B_res)) : 0, vs = f ? round256(f->store_bytes(p, 1, B_val)) : 0;
  const size_t one_tile = hbm ? round256(qc_h2_bytes(p, p->h2, 6, true, 1)) : 0;
  auto region = [&](size_t r, size_t v) -> size_t {
    if (!hbm) return r > 0 ? r + v : 0;
    const double budget = hbm_budget_bytes();
    if ((double)(r + v) <= budget) return r + v > one_tile ? r + v : one_tile;
    const int64_t fit = qc_h2_tiles_that_fit(p, p->h2, 6, true, (size_t)budget);
    const size_t some = round256(qc_h2_bytes(p, p->h2, 6, true, fit < 1 ? 1 : fit));
    return some > one_tile ? some : one_tile;
  };
  const size_t ar = round256(sizeof(float) * 6 * p->n_qubits * (size_t)B_res);
  const size_t av = round256(sizeof(float) * p->n_qubits * (size_t)B_val);
  QcStepLayout s = {};
  if (!ws) s.bytes = round256(region(rs, vs)) + (p->amplitude ? 2 * ar + 2 * av : 0);
  char* cws = (char*)ws;
  size_t cws_bytes = ws_bytes;
  if (p->amplitude && ws) {
    // the circuit region is carved for the residual tiles alone: the value tiles of the HBM family never get the
    // resident slots that `bytes` pays for (follow-up: round256(region(rs, vs)))
    cws_bytes = round256(region(rs, 0));
    char* a = (char*)ws + cws_bytes;
    s.u_res = (float*)a;
    s.ub_res = (float*)(a + ar);
    s.u_val = (float*)(a + 2 * ar);
    s.ub_val = (float*)(a + 2 * ar + av);
    if (cws_bytes == 0) cws = nullptr;
  }
  if (hbm) {
    s.fits = cws && cws_bytes >= one_tile;
    const bool resident = cws_bytes >= rs + vs;
    s.res = {cws, resident ? rs : cws_bytes, resident};
    s.val = {resident ? cws + rs : cws, resident ? vs : cws_bytes, resident};
  } else {
    s.fits = true;
    s.res = {cws, cws_bytes, cws && rs > 0 && cws_bytes >= rs};
    const bool keep_val = cws && rs > 0 && vs > 0 && cws_bytes >= rs + vs;   // one byte short: the residual store only
    s.val = keep_val ? QcCircStore{cws + rs, vs, true} : QcCircStore{cws, cws_bytes, false};
  }
  return s;
}

int qc_hbm_plan_describe(const int32_t* rows, int n_gates, int n_qubits, int n_params, int32_t* out, int cap) {
  if (!rows || n_gates <= 0 || n_qubits < 9 || n_qubits > 20 || n_params < 0 || cap < 0) return 0;
  QcGate* h = (QcGate*)malloc(sizeof(QcGate) * n_gates);
  if (!h) return 0;
  int n_u4 = 0, len = 0;
  if (parse_rows(rows, n_gates, n_qubits, n_params, h, &n_u4))
    len = qc_h2_describe_gates(h, n_gates, n_qubits, (detect_lead_rx(h, n_gates, n_qubits) && absorb_enabled()) ? 1 : 0, out, cap);
  free(h);
  return len;
}

int qc_wave_sched_describe(const int32_t* rows, int n_gates, int n_qubits, int n_params, int32_t* out, int cap) {
  if (!rows || n_gates <= 0 || n_gates > QC_WS_MAX_ITEMS || n_qubits < 1 || n_qubits > 8 || n_params < 0 || cap < 0) return 0;
  QcGate* h = (QcGate*)malloc(sizeof(QcGate) * n_gates);
  if (!h) return 0;
  int n_u4 = 0, len = 0;
  if (parse_rows(rows, n_gates, n_qubits, n_params, h, &n_u4)) {
    const QcWaveSched ws = qc_wave_schedule(h, n_gates, n_qubits);
    auto put = [&](int v) {
      if (out && len < cap) out[len] = v;
      ++len;
    };
    put(ws.n_items);
    put(ws.n_runs);
    for (int i = 0; i < ws.n_items; ++i) put(ws.item[i]);
    for (int r = 0; r < ws.n_runs; ++r) {
      put(ws.run_off[r + 1] - ws.run_off[r]);
      for (int e = ws.run_off[r]; e < ws.run_off[r + 1]; ++e) put(ws.entry[e]);
    }
  }
  free(h);
  return len;
}

size_t qc_step_workspace_bytes(const qc_program* p, int64_t B_res, int64_t B_val) {
  if (!p || B_res < 0 || B_val < 0) return 0;
  return step_layout(p, B_res, B_val, nullptr, 0).bytes;
}

int qc_forward_expval(const qc_program* p, const void* trig, const float* umat, const float* angles,
                      float* expval, int64_t B, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_circuit(p, trig, umat, B);
  if (rc) return rc;
  if (!angles || !expval) return QC_ERR_ARG;
  rc = p->fam->fwd(p, (const QcTrig*)trig, umat, angles, expval, B, 1, {ws, ws_bytes, false}, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_backward_expval(const qc_program* p, const void* trig, const float* umat, const float* angles,
                       const float* cot, float* d_angles, float* part, int64_t part_stride, int64_t row0,
                       int64_t B, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_circuit(p, trig, umat, B);
  if (rc) return rc;
  if (!angles || !cot || !d_angles || !part || part_stride < p->n_params || row0 < 0) return QC_ERR_ARG;
  rc = p->fam->bwd(p, (const QcTrig*)trig, umat, angles, cot, d_angles, part, part_stride, row0, B, 1, {ws, ws_bytes, false},
                   (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_forward_jets(const qc_program* p, const void* trig, const float* umat, const float* ajets, float* qjets,
                    int64_t B, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_circuit(p, trig, umat, B);
  if (rc) return rc;
  if (!ajets || !qjets) return QC_ERR_ARG;
  rc = p->fam->fwd(p, (const QcTrig*)trig, umat, ajets, qjets, B, 6, {ws, ws_bytes, false}, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_backward_jets(const qc_program* p, const void* trig, const float* umat, const float* ajets,
                     const float* qbar, float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B,
                     void* ws, size_t ws_bytes, void* stream) {
  int rc = check_circuit(p, trig, umat, B);
  if (rc) return rc;
  if (!ajets || !qbar || !abar || !part || part_stride < p->n_params || row0 < 0) return QC_ERR_ARG;
  rc = p->fam->bwd(p, (const QcTrig*)trig, umat, ajets, qbar, abar, part, part_stride, row0, B, 6, {ws, ws_bytes, false},
                   (hipStream_t)stream);
  return rc ? rc : after_launch();
}

// Register-family variants that hand the forward pass's final states to the adjoint pass through
// chi_dev [6][2*2^n][B] instead of recomputing them (12 instead of 18 circuit-equivalents per point).
int qc_forward_jets_keep(const qc_program* p, const void* trig, const float* umat, const float* ajets, float* qjets,
                         int64_t B, float* chi, void* stream) {
  int rc = check_circuit(p, trig, umat, B);
  if (rc) return rc;
  if (!ajets || !qjets || !chi) return QC_ERR_ARG;
  if (p->fam != &qc_family_reg) return QC_ERR_UNSUPPORTED;
  rc = p->fam->fwd(p, (const QcTrig*)trig, umat, ajets, qjets, B, 6, {chi, 0, true}, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_backward_jets_kept(const qc_program* p, const void* trig, const float* umat, const float* ajets,
                          const float* qbar, float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B,
                          const float* chi, void* stream) {
  int rc = check_circuit(p, trig, umat, B);
  if (rc) return rc;
  if (!ajets || !qbar || !abar || !part || !chi || part_stride < p->n_params || row0 < 0) return QC_ERR_ARG;
  if (p->fam != &qc_family_reg) return QC_ERR_UNSUPPORTED;
  rc = p->fam->bwd(p, (const QcTrig*)trig, umat, ajets, qbar, abar, part, part_stride, row0, B, 6,
                   {(void*)chi, 0, true}, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

static int check_mlp(int H, int n, int n_theta, int64_t B, int nch) {
  if (H < 1 || H > 1024 || n < 1 || n > 16 || n_theta < 0 || B <= 0 || (nch != 1 && nch != 6)) return QC_ERR_ARG;
  return QC_OK;
}

int qc_pre_forward_map(const float* X, const float* prm, int H, int n, int n_theta, int angle_map, float* ajets, int64_t B,
                       int nch, void* stream) {
  int rc = check_mlp(H, n, n_theta, B, nch);
  if (rc) return rc;
  if (!X || !prm || !ajets || !angle_map_ok(angle_map)) return QC_ERR_ARG;
  rc = qc_mlp_pre_fwd(X, prm, make_layout(H, n, n_theta), ajets, B, nch, (hipStream_t)stream, angle_map);
  return rc ? rc : after_launch();
}

int qc_pre_forward(const float* X, const float* prm, int H, int n, int n_theta, float* ajets, int64_t B, int nch,
                   void* stream) {
  return qc_pre_forward_map(X, prm, H, n, n_theta, QC_ANGLE_MAP_NONE, ajets, B, nch, stream);
}

int qc_pre_backward_map(const float* X, const float* prm, int H, int n, int n_theta, int angle_map, const float* ajets,
                        const float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream) {
  int rc = check_mlp(H, n, n_theta, B, nch);
  if (rc) return rc;
  const QcLayout L = make_layout(H, n, n_theta);
  if (!X || !prm || !abar || !part || part_stride < L.NP || row0 < 0 || !angle_map_ok(angle_map)) return QC_ERR_ARG;
  if (angle_map != QC_ANGLE_MAP_NONE && !ajets) return QC_ERR_ARG;
  rc = qc_mlp_pre_bwd(X, prm, L, abar, part, part_stride, row0, B, nch, (hipStream_t)stream, angle_map, ajets);
  return rc ? rc : after_launch();
}

int qc_pre_backward(const float* X, const float* prm, int H, int n, int n_theta, const float* abar, float* part,
                    int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream) {
  return qc_pre_backward_map(X, prm, H, n, n_theta, QC_ANGLE_MAP_NONE, nullptr, abar, part, part_stride, row0, B, nch,
                             stream);
}

int qc_pre_forward_ff(const float* X, const float* prm, int H, int n, int n_theta, int angle_map, const float* freq_dev, int m,
                      float* ajets, int64_t B, int nch, void* stream) {
  int rc = check_mlp(H, n, n_theta, B, nch);
  if (rc) return rc;
  if (!X || !prm || !ajets || !angle_map_ok(angle_map) || !freq_dev || m < 1 || m > QC_FF_MAX) return QC_ERR_ARG;
  rc = qc_mlp_pre_ff_fwd(X, prm, qc_layout(H, n, n_theta, 1, 0, 2 * m), ajets, B, nch, (hipStream_t)stream, angle_map, freq_dev, m);
  return rc ? rc : after_launch();
}

int qc_pre_backward_ff(const float* X, const float* prm, int H, int n, int n_theta, int angle_map, const float* freq_dev, int m,
                       const float* ajets, const float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B, int nch,
                       void* stream) {
  int rc = check_mlp(H, n, n_theta, B, nch);
  if (rc) return rc;
  if (!freq_dev || m < 1 || m > QC_FF_MAX) return QC_ERR_ARG;
  const QcLayout L = qc_layout(H, n, n_theta, 1, 0, 2 * m);
  if (!X || !prm || !abar || !part || part_stride < L.NP || row0 < 0 || !angle_map_ok(angle_map)) return QC_ERR_ARG;
  if (angle_map != QC_ANGLE_MAP_NONE && !ajets) return QC_ERR_ARG;
  rc = qc_mlp_pre_ff_bwd(X, prm, L, abar, part, part_stride, row0, B, nch, (hipStream_t)stream, angle_map, ajets, freq_dev, m);
  return rc ? rc : after_launch();
}

// the pre stage in front of program p: the plain launchers, or the Fourier-feature ones with the program's map
static int prog_pre_forward(const qc_program* p, const float* X, const float* prm, int H, int n, int n_theta, float* ajets,
                            int64_t B, int nch, void* stream) {
  if (p->ff_m > 0) return qc_pre_forward_ff(X, prm, H, n, n_theta, p->angle_map, p->d_ff_freq, p->ff_m, ajets, B, nch, stream);
  return qc_pre_forward_map(X, prm, H, n, n_theta, p->angle_map, ajets, B, nch, stream);
}
static int prog_pre_backward(const qc_program* p, const float* X, const float* prm, int H, int n, int n_theta, const float* ajets,
                             const float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream) {
  if (p->ff_m > 0)
    return qc_pre_backward_ff(X, prm, H, n, n_theta, p->angle_map, p->d_ff_freq, p->ff_m, ajets, abar, part, part_stride, row0, B,
                              nch, stream);
  return qc_pre_backward_map(X, prm, H, n, n_theta, p->angle_map, ajets, abar, part, part_stride, row0, B, nch, stream);
}

// qc_post, and by `tg` qc_post_data (mode 2 on tabulated targets: X is not read) or qc_post_coef (out_u = the [6][B]
// cotangents, out_res not used)
static int post_impl(int mode, const float* X, const float* prm, int H, int n, int n_theta, const qc_pde* pde,
                     const float* qjets, float* out_u, float* out_res, const float* in_ubar, const float* in_rbar,
                     float* qbar, float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream,
                     const QcTarget& tg, int n_in = 3) {
  int rc = check_mlp(H, n, n_theta, B, nch);
  if (rc) return rc;
  const QcLayout L = qc_layout(H, n, n_theta, 1, tg.n_op(), n_in);
  const bool analytic = tg.kind == QC_TARGET_ANALYTIC;
  if (mode < 0 || mode > 4 || (!X && analytic) || !prm || !pde || !qjets) return QC_ERR_ARG;
  // the analytic targets are defined for 0..2 only; the tabulated ones by the rule of their type
  if ((mode == 2 && analytic && !problem_ok(pde->problem)) || !tg.ok(mode, nch, pde->problem)) return QC_ERR_ARG;
  if (mode >= 3 && nch != 6) return QC_ERR_ARG;          // general jets: six channels only
  if (mode >= 1 && mode <= 3 && (!qbar || !part || row0 < 0 || part_stride < L.NP + (mode == 2 ? 3 : 0))) return QC_ERR_ARG;
  if (mode == 2 && (!out_u || (nch == 6 && !out_res && tg.kind != QC_TARGET_COEF && tg.kind != QC_TARGET_LEARN)))
    return QC_ERR_ARG;  // per-point cotangent scratch
  if ((mode == 3 && !in_ubar) || (mode == 4 && !out_u)) return QC_ERR_ARG;
  rc = qc_mlp_post(mode, X, prm, L, to_pde(pde), qjets, out_u, out_res, in_ubar, in_rbar, qbar, part, part_stride,
                   row0, B, nch, (hipStream_t)stream, tg);
  return rc ? rc : after_launch();
}

int qc_post(int mode, const float* X, const float* prm, int H, int n, int n_theta, const qc_pde* pde,
            const float* qjets, float* out_u, float* out_res, const float* in_ubar, const float* in_rbar,
            float* qbar, float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream) {
  return post_impl(mode, X, prm, H, n, n_theta, pde, qjets, out_u, out_res, in_ubar, in_rbar, qbar, part, part_stride, row0,
                   B, nch, stream, QcTarget{});
}

int qc_post_data(const float* prm, int H, int n, int n_theta, const qc_pde* pde, const float* qjets, const float* target,
                 float c_u, float* out_u, float* out_res, float* qbar, float* part, int64_t part_stride, int64_t row0,
                 int64_t B, int nch, void* stream) {
  if (!target) return QC_ERR_ARG;
  return post_impl(2, nullptr, prm, H, n, n_theta, pde, qjets, out_u, out_res, nullptr, nullptr, qbar, part, part_stride,
                   row0, B, nch, stream, QcTarget::tabulated(target, target, c_u));
}

int qc_post_coef(const float* prm, int H, int n, int n_theta, const qc_pde* pde, const float* qjets, const float* target,
                 const float* coef, float* cot, float* qbar, float* part, int64_t part_stride, int64_t row0, int64_t B,
                 void* stream) {
  if (!target || !coef || !cot) return QC_ERR_ARG;
  return post_impl(2, nullptr, prm, H, n, n_theta, pde, qjets, cot, nullptr, nullptr, nullptr, qbar, part, part_stride, row0, B,
                   6, stream, QcTarget::with_coef(target, target, coef));
}

// THE validity rule of a learned operator: finite base and scale, a history buffer behind a positive capacity
static bool learn_ok(const qc_step_learn* lr) {
  if (!lr || lr->coef_hist_cap < 0 || (lr->coef_hist_cap > 0 && !lr->coef_hist_dev)) return false;
  for (int k = 0; k < QC_COEF_COLS; ++k)
    if (!isfinite(lr->base[k]) || !isfinite(lr->scale[k])) return false;
  return true;
}
// the kernels' record: base and scale, and the history buffer with the optimiser record that places its rows (or neither)
static QcLearn to_learn(const qc_step_learn* lr, const void* opt_state) {
  QcLearn q;
  memcpy(q.base, lr->base, sizeof(q.base));
  memcpy(q.scale, lr->scale, sizeof(q.scale));
  const bool hist = opt_state && lr->coef_hist_dev && lr->coef_hist_cap > 0;
  q.hist = hist ? lr->coef_hist_dev : nullptr;
  q.hist_cap = hist ? lr->coef_hist_cap : 0;
  q.st = hist ? (const QcOptState*)opt_state : nullptr;
  return q;
}

int qc_post_learn(const float* prm, int H, int n, int n_theta, const qc_pde* pde, const qc_step_learn* learn,
                  const float* qjets, const float* target, float* cot, float* qbar, float* part, int64_t part_stride,
                  int64_t row0, int64_t B, void* stream) {
  if (!target || !cot || !learn_ok(learn)) return QC_ERR_ARG;
  return post_impl(2, nullptr, prm, H, n, n_theta, pde, qjets, cot, nullptr, nullptr, nullptr, qbar, part, part_stride, row0, B,
                   6, stream, QcTarget::learned(target, target, to_learn(learn, nullptr)));
}

// THE validity rule of a balancer: finite scales, a history buffer behind a positive capacity
static bool bal_ok(const qc_step_balance* b) {
  if (!b || b->weight_hist_cap < 0 || (b->weight_hist_cap > 0 && !b->weight_hist_dev)) return false;
  for (int k = 0; k < QC_BAL_TERMS; ++k)
    if (!isfinite(b->scale[k])) return false;
  return true;
}
// the kernels' record (the post stage reads the scales only; the history is the optimiser launch's)
static QcBal to_bal(const qc_step_balance* b) {
  QcBal q;
  memcpy(q.scale, b->scale, sizeof(q.scale));
  const bool hist = b->weight_hist_dev && b->weight_hist_cap > 0;
  q.hist = hist ? b->weight_hist_dev : nullptr;
  q.hist_cap = hist ? b->weight_hist_cap : 0;
  return q;
}

int qc_post_balance(const float* prm, int H, int n, int n_theta, const qc_pde* pde, const qc_step_balance* bal,
                    const float* qjets, const float* target, float c_u, float* out_u, float* out_res, float* qbar, float* part,
                    int64_t part_stride, int64_t row0, int64_t B, int nch, void* stream) {
  if (!target || !bal_ok(bal)) return QC_ERR_ARG;
  return post_impl(2, nullptr, prm, H, n, n_theta, pde, qjets, out_u, out_res, nullptr, nullptr, qbar, part, part_stride,
                   row0, B, nch, stream, QcTarget::balanced(target, target, c_u, to_bal(bal)));
}

int qc_post_multi(int mode, const float* prm, int H, int n, int n_theta, int K, const float* w4k, const float* qjets,
                  float* out_u, const float* in_ubar, float* qbar, float* part, int64_t part_stride, float* partk,
                  int64_t partk_stride, int64_t row0, int64_t B, void* stream) {
  int rc = check_mlp(H, n, n_theta, B, 6);
  if (rc) return rc;
  const QcLayout L = make_layout(H, n, n_theta);
  if ((mode != 3 && mode != 4) || K < 1 || K > 4 || !prm || !w4k || !qjets) return QC_ERR_ARG;
  if (mode == 4 && !out_u) return QC_ERR_ARG;
  if (mode == 3 && (!in_ubar || !qbar || !part || !partk || row0 < 0 || part_stride < L.NP || partk_stride < (int64_t)K * (H + 1)))
    return QC_ERR_ARG;
  rc = qc_mlp_post_multi(mode, prm, L, K, w4k, qjets, out_u, in_ubar, qbar, part, part_stride, partk, partk_stride, row0, B,
                         (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_reduce_rows(const float* part, int64_t rows, int64_t stride, int ncols, float* out, void* stream) {
  if (!part || !out || rows <= 0 || ncols <= 0 || stride < ncols) return QC_ERR_ARG;
  qc_opt_reduce_rows(part, rows, stride, ncols, out, (hipStream_t)stream);
  return after_launch();
}

// qc_adam_step, and with `bal` (validated by the caller) qc_balance_adam_step: the last QC_BAL_TERMS of the NP entries are
// the balancer's, at least one entry is the network's, and theta lies in front of them
static int adam_step_impl(float* flat, int NP, float* prm, float* m, float* v, void* state, const qc_opt_hyper* hp,
                          float* hist, int hist_cap, const qc_program* prog, int theta_off, void* trig, void* stream,
                          const QcBal* bal) {
  const int n_own = bal ? QC_BAL_TERMS : 0;
  if (!flat || NP <= n_own || !prm || !m || !v || !state || !hp) return QC_ERR_ARG;
  if (prog && (!trig || theta_off < 0 || theta_off + prog->n_params > NP - n_own)) return QC_ERR_ARG;
  QcOptHyper h;
  memcpy(&h, hp, sizeof(h));
  qc_opt_adam(flat, NP, prm, m, v, (QcOptState*)state, h, hist, hist_cap, prog, theta_off, (QcTrig*)trig,
              (hipStream_t)stream, bal);
  return after_launch();
}

int qc_adam_step(float* flat, int NP, float* prm, float* m, float* v, void* state, const qc_opt_hyper* hp,
                 float* hist, int hist_cap, const qc_program* prog, int theta_off, void* trig, void* stream) {
  return adam_step_impl(flat, NP, prm, m, v, state, hp, hist, hist_cap, prog, theta_off, trig, stream, nullptr);
}

int qc_balance_adam_step(float* flat, int NP_B, float* prm, float* m, float* v, void* state, const qc_opt_hyper* hp,
                         const qc_step_balance* bal, float* hist, int hist_cap, const qc_program* prog, int theta_off,
                         void* trig, void* stream) {
  if (!bal_ok(bal)) return QC_ERR_ARG;
  const QcBal q = to_bal(bal);
  return adam_step_impl(flat, NP_B, prm, m, v, state, hp, hist, hist_cap, prog, theta_off, trig, stream, &q);
}

// ---- L-BFGS (qc_lbfgs.hip)
static_assert(sizeof(QcLbfgsHyper) == sizeof(qc_lbfgs_hyper), "qc_lbfgs_hyper layout");
static bool lbfgs_shape_ok(int NP, int history) { return NP >= 1 && history >= 1 && history <= QC_LBFGS_MAX_HISTORY; }
static bool pos_finite(float v) { return isfinite(v) && v > 0.f; }

size_t qc_lbfgs_workspace_bytes(int NP, int history) {
  return lbfgs_shape_ok(NP, history) ? sizeof(float) * qc_lbfgs_words(NP, history) : 0;
}

int qc_lbfgs_init(void* ws, int NP, int history, void* stream) {
  if (!ws || ((uintptr_t)ws & 3) || !lbfgs_shape_ok(NP, history)) return QC_ERR_ARG;
  qc_lbfgs_init_launch(ws, NP, history, (hipStream_t)stream);
  return after_launch();
}

int qc_lbfgs_restart(void* ws, int keep_history, void* stream) {
  if (!ws || ((uintptr_t)ws & 3)) return QC_ERR_ARG;
  qc_lbfgs_restart_launch(ws, keep_history != 0, (hipStream_t)stream);
  return after_launch();
}

int qc_lbfgs_step(float* flat, int NP, float* prm, void* ws, const qc_lbfgs_hyper* hp, float* hist, int hist_cap,
                  const qc_program* prog, int theta_off, void* trig, void* stream) {
  if (!flat || !prm || !ws || ((uintptr_t)ws & 3) || !hp || !lbfgs_shape_ok(NP, hp->history)) return QC_ERR_ARG;
  if (hp->line_search != QC_LBFGS_FIXED && hp->line_search != QC_LBFGS_ARMIJO) return QC_ERR_ARG;
  if (hp->max_ls < 1 || !pos_finite(hp->lr) || !pos_finite(hp->c1) || !pos_finite(hp->shrink_lo) || !pos_finite(hp->shrink_hi) ||
      !pos_finite(hp->curv_eps) || hp->shrink_lo > hp->shrink_hi || hp->shrink_hi >= 1.f)
    return QC_ERR_ARG;
  if (!isfinite(hp->w_res) || !isfinite(hp->w_bc) || !isfinite(hp->w_ic) || hist_cap < 0) return QC_ERR_ARG;
  if (prog && (!trig || theta_off < 0 || theta_off + prog->n_params > NP)) return QC_ERR_ARG;
  QcLbfgsHyper h;
  memcpy(&h, hp, sizeof(h));
  qc_lbfgs_step_launch(flat, NP, prm, ws, h, hist, hist_cap, prog, theta_off, (QcTrig*)trig, (hipStream_t)stream);
  return after_launch();
}

// The one place that fills batches: the source's rule, the launch its kind selects, the launch status
static int fill_batches(const QcBatches& b, const QcSource& s, void* stream) {
  if (!s.ok(b)) return QC_ERR_ARG;
  if (s.kind == QC_SOURCE_DRAW) qc_sample_launch(b, s.face_pts, (hipStream_t)stream);
  else qc_gather_launch(b, s, (hipStream_t)stream);
  return after_launch();
}
// Source of a step or of a gather from the optional records of the public header: no data: the coordinate draw; data:
// its dataset's rows, with `cf` the operator rows as well (into coef_res), with `ad` the residual rows from its CDF
// (the caller's buffer {64-byte record, cdf[n_rows], coarse[ceil(n_rows / QC_ADAPT_BLOCK)]})
static QcSource make_source(const qc_step_data* t, const qc_step_coef* cf, float* coef_res, const qc_step_adapt* ad,
                            int64_t face_pts = 0) {
  QcSource s;
  s.face_pts = face_pts;
  if (!t) return s;
  s.kind = QC_SOURCE_ROWS;
  s.res = {t->ds_X_res, t->ds_r, t->ds_n_res};
  s.ic = {t->ds_X_ic, t->ds_u_ic, t->ds_n_ic};
  s.bc = {t->ds_X_bc, t->ds_u_bc, t->ds_n_bc};
  if (cf) { s.table = true; s.coef_res = coef_res; s.ds_coef = cf->ds_coef; }
  if (ad) {
    s.kind = QC_SOURCE_CDF;
    s.cdf_rows = ad->n_rows;
    if (ad->adapt_dev) {
      s.cdf = (const uint64_t*)((const char*)ad->adapt_dev + sizeof(QcAdaptRec));
      s.coarse = s.cdf + ad->n_rows;
    }
  }
  return s;
}

int qc_sample_collocation_faces(float* X_res, int64_t n_res, int64_t off_res, float* X_val, int64_t n_ic, int64_t off_ic,
                                int64_t n_bc, int64_t off_bc, int64_t bc_face_points, uint64_t seed, uint64_t step,
                                void* stream) {
  return fill_batches({X_res, nullptr, n_res, off_res, X_val, nullptr, n_ic, off_ic, n_bc, off_bc, seed, step},
                      make_source(nullptr, nullptr, nullptr, nullptr, bc_face_points), stream);
}

int qc_sample_collocation(float* X_res, int64_t n_res, int64_t off_res, float* X_val, int64_t n_ic, int64_t off_ic,
                          int64_t n_bc, int64_t off_bc, uint64_t seed, uint64_t step, void* stream) {
  return qc_sample_collocation_faces(X_res, n_res, off_res, X_val, n_ic, off_ic, n_bc, off_bc, 0, seed, step, stream);
}

// ---- residual-adaptive sampling
size_t qc_adapt_bytes(int64_t n_rows) {
  if (n_rows < 1 || n_rows >= ((int64_t)1 << 31)) return 0;
  return sizeof(QcAdaptRec) + sizeof(uint64_t) * ((size_t)n_rows + (size_t)((n_rows + QC_ADAPT_BLOCK - 1) / QC_ADAPT_BLOCK));
}

int qc_adapt_build(const float* score, int64_t n_rows, int power, float floor_c, void* adapt, void* stream) {
  if (!score || !adapt || ((uintptr_t)adapt & 7) != 0 || n_rows < 1 || n_rows >= ((int64_t)1 << 31)) return QC_ERR_ARG;
  if (power < 1 || power > 4 || !(floor_c >= 0.f) || !(floor_c <= QC_ADAPT_FLOOR_MAX)) return QC_ERR_ARG;
  const int rc = qc_adapt_build_launch(score, n_rows, power, floor_c, adapt, (hipStream_t)stream);
  return rc ? hip_fail(hipGetLastError()) : after_launch();
}

// the three gathers: rows and targets of the three batches; with a table the residual rows' operator coefficients as
// well (coef_res and ds_coef may be NULL only with n_res = 0); with a CDF the residual rows drawn from it
int qc_sample_dataset(float* X_res, float* target_res, int64_t n_res, int64_t off_res, float* X_val, float* target_val,
                      int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, const qc_step_data* t, uint64_t seed,
                      uint64_t step, void* stream) {
  if (!t) return QC_ERR_ARG;
  return fill_batches({X_res, target_res, n_res, off_res, X_val, target_val, n_ic, off_ic, n_bc, off_bc, seed, step},
                      make_source(t, nullptr, nullptr, nullptr), stream);
}

int qc_sample_dataset_coef(float* X_res, float* target_res, int64_t n_res, int64_t off_res, float* X_val, float* target_val,
                           int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, float* coef_res, const qc_step_data* t,
                           const qc_step_coef* cf, uint64_t seed, uint64_t step, void* stream) {
  if (!t || !cf) return QC_ERR_ARG;
  return fill_batches({X_res, target_res, n_res, off_res, X_val, target_val, n_ic, off_ic, n_bc, off_bc, seed, step},
                      make_source(t, cf, coef_res, nullptr), stream);
}

int qc_sample_dataset_adaptive(float* X_res, float* target_res, int64_t n_res, int64_t off_res, float* X_val, float* target_val,
                               int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, float* coef_res, const qc_step_data* t,
                               const qc_step_coef* cf, const qc_step_adapt* ad, uint64_t seed, uint64_t step, void* stream) {
  if (!t || !ad) return QC_ERR_ARG;   // without a table (cf NULL): rows and targets only
  return fill_batches({X_res, target_res, n_res, off_res, X_val, target_val, n_ic, off_ic, n_bc, off_bc, seed, step},
                      make_source(t, cf, coef_res, ad), stream);
}

// ---- merged residual + value stages of the fused step (register family, angle encoding)
static bool merged_ok(const qc_step_desc* d) {
  static const bool no_merge = [] { const char* e = getenv("QC_NO_MERGE"); return e && e[0] == '1'; }();
  return !no_merge && d->prog->fam == &qc_family_reg && !d->prog->amplitude && d->B_res > 0 && d->B_val > 0 &&
         d->circ_ws_dev && d->circ_ws_bytes >= qc_family_reg.store_bytes(d->prog, 6, d->B_res) && d->X_res_dev && d->ajets_res_dev &&
         d->qjets_res_dev && d->qbar_res_dev && d->abar_res_dev && d->X_val_dev && d->ajets_val_dev && d->qjets_val_dev &&
         d->qbar_val_dev && d->abar_val_dev;
}

// the step's batches as the sampler sees them (targets: those of `t`, or none)
static QcBatches step_batches(const qc_step_desc* d, const qc_step_data* t) {
  return {(float*)d->X_res_dev, t ? t->target_res_dev : nullptr, d->B_res, d->sample_off_res,
          (float*)d->X_val_dev, t ? t->target_val_dev : nullptr, d->n_ic, d->sample_off_ic, d->B_val - d->n_ic, d->sample_off_bc,
          d->sample_seed, d->sample_step};
}

// What fused_step, qc_fused_step_stage and qc_dataset_scores ask of a descriptor (non-null) before anything else of
// theirs that can coincide with it, in the order all three had it, so every refusal keeps its code: program and core
// buffers, n / n_theta, [umat behind U4 gates,] [`supported`: what the caller needs of the kernel family,] the network's
// shape, and with amplitude encoding the step workspace
static int check_step_desc(const qc_step_desc* d, bool need_umat, bool (*supported)(const qc_step_desc*)) {
  if (!d->prog || !d->trig_dev || !d->params_dev) return QC_ERR_ARG;
  if (d->prog->n_qubits != d->n || d->prog->n_params != d->n_theta) return QC_ERR_ARG;
  if (need_umat && d->prog->n_u4 > 0 && !d->umat_dev) return QC_ERR_ARG;
  if (supported && !supported(d)) return QC_ERR_UNSUPPORTED;
  const int rc = check_mlp(d->H, d->n, d->n_theta, d->B_res > 0 ? d->B_res : 1, 6);
  if (rc) return rc;
  // amplitude encoding: the circuit kernels run on the initial-amplitude jets u(a) and return cotangents w.r.t. them,
  // both kept in the step workspace
  if (d->prog->amplitude && (!d->circ_ws_dev || d->circ_ws_bytes < qc_step_workspace_bytes(d->prog, d->B_res, d->B_val)))
    return QC_ERR_ARG;
  return QC_OK;
}

static int merged_stage(const qc_step_desc* d, int stage, hipStream_t st, bool draw, const QcTarget& tg) {
  const qc_program* pg = d->prog;
  const QcLayout L = qc_layout(d->H, d->n, d->n_theta, 1, tg.n_op(), prog_n_in(pg));
  const int64_t rows_res = qc_ceil_div(d->B_res, 64);
  const QcTrig* trig = (const QcTrig*)d->trig_dev;
  const float* prm = d->params_dev;
  float* chi_store = (float*)d->circ_ws_dev;
  QcPde pde;
  memcpy(&pde, &d->pde, sizeof(pde));
  switch (stage) {
    case QC_STAGE_PRE_FWD:
      if (pg->ff_m > 0)
        return qc_mlp_pre_ff_fwd_both(step_batches(d, nullptr), draw ? 1 : 0, d->sample_bc_face_points, prm, L, d->ajets_res_dev,
                                      d->ajets_val_dev, st, pg->angle_map, pg->d_ff_freq, pg->ff_m);
      return qc_mlp_pre_fwd_both(step_batches(d, nullptr), draw ? 1 : 0, d->sample_bc_face_points, prm, L, d->ajets_res_dev,
                                 d->ajets_val_dev, st, d->prog->angle_map);
    case QC_STAGE_CIRCUIT_FWD:
      return qc_reg_circ_fwd_both(d->prog, trig, d->umat_dev, d->ajets_res_dev, d->qjets_res_dev, d->B_res, chi_store,
                                  d->ajets_val_dev, d->qjets_val_dev, d->B_val, st);
    case QC_STAGE_POST:
      // abar_* are written only by the adjoint sweep: their heads serve as per-point cotangent scratch here (two
      // B_res-float rows; with a coefficient table the [6][B_res] channel cotangents, of abar_res' 6 n B_res floats)
      return qc_mlp_post_both(prm, L, pde, (const float*)d->X_res_dev, d->qjets_res_dev, d->abar_res_dev,
                              d->abar_res_dev + d->B_res, d->qbar_res_dev, 0, d->B_res, (const float*)d->X_val_dev,
                              d->qjets_val_dev, d->abar_val_dev, d->qbar_val_dev, rows_res, d->B_val, d->part_dev,
                              d->part_stride, st, tg);
    case QC_STAGE_CIRCUIT_BWD:
      return qc_reg_circ_bwd_both(d->prog, trig, d->umat_dev, d->ajets_res_dev, d->qbar_res_dev, d->abar_res_dev, 0, d->B_res,
                                  chi_store, d->ajets_val_dev, d->qbar_val_dev, d->abar_val_dev, rows_res, d->B_val,
                                  d->part_dev + L.oTh, d->part_stride, st);
    case QC_STAGE_PRE_BWD:
      if (pg->ff_m > 0)
        return qc_mlp_pre_ff_bwd_both((const float*)d->X_res_dev, (const float*)d->X_val_dev, prm, L, d->abar_res_dev,
                                      d->abar_val_dev, d->part_dev, d->part_stride, 0, rows_res, d->B_res, d->B_val, st,
                                      pg->angle_map, d->ajets_res_dev, d->ajets_val_dev, pg->d_ff_freq, pg->ff_m);
      return qc_mlp_pre_bwd_both((const float*)d->X_res_dev, (const float*)d->X_val_dev, prm, L, d->abar_res_dev,
                                 d->abar_val_dev, d->part_dev, d->part_stride, 0, rows_res, d->B_res, d->B_val, st,
                                 d->prog->angle_map, d->ajets_res_dev, d->ajets_val_dev);
    default: return QC_ERR_ARG;
  }
}

int qc_fused_step_stage(const qc_step_desc* d, int stage, void* stream) {
  if (!d || !d->part_dev || stage < 0 || stage >= QC_STAGE_COUNT) return QC_ERR_ARG;
  // analytic targets and the coordinate draw only, like qc_fused_pinn_residual_step
  if (!problem_ok(d->pde.problem) || d->sample_bc_face_points < QC_BC_RANDOM_FACE) return QC_ERR_ARG;
  int rc = check_step_desc(d, false, merged_ok);
  if (rc) return rc;
  if ((rc = merged_stage(d, stage, (hipStream_t)stream, false, QcTarget{}))) return rc;
  return after_launch();
}

// ---- systems: K outputs, the operator as a term list
// THE validity rule of a system's operator: counts in range, every term field in range, finite coefficients and weights
static bool sys_ok(const qc_step_system* s) {
  if (!s || s->K < 1 || s->K > QC_KMAX || s->n_eq < 1 || s->n_eq > QC_EQMAX || s->n_terms < 1 || s->n_terms > QC_TERMS_MAX)
    return false;
  for (int t = 0; t < s->n_terms; ++t) {
    const qc_sys_term& m = s->terms[t];
    if (m.eq < 0 || m.eq >= s->n_eq || m.out < 0 || m.out >= s->K || m.chan < 0 || m.chan >= QC_NCH) return false;
    if (m.mul0 < -1 || m.mul0 >= s->K || m.mul1 < -1 || m.mul1 >= s->K || !isfinite(m.coef)) return false;
  }
  for (int e = 0; e < s->n_eq; ++e)
    if (!isfinite(s->w_eq[e])) return false;
  for (int k = 0; k < s->K; ++k)
    if (!isfinite(s->w_out[k])) return false;
  return true;
}
static QcSys to_sys(const qc_step_system* s) {   // the head of the record; unused slots zeroed
  QcSys q;
  memset(&q, 0, sizeof(q));
  q.K = s->K; q.n_eq = s->n_eq; q.n_terms = s->n_terms;
  memcpy(q.terms, s->terms, sizeof(QcSysTerm) * s->n_terms);
  for (int e = 0; e < s->n_eq; ++e) q.w_eq[e] = s->w_eq[e];
  for (int k = 0; k < s->K; ++k) q.w_out[k] = s->w_out[k];
  return q;
}

int qc_post_system(const float* prm, int H, int n, int n_theta, const qc_step_system* sys, const qc_pde* pde,
                   const float* qjets, const float* target, float* qbar, float* part, int64_t part_stride, int64_t row0,
                   int64_t B, int nch, void* stream) {
  int rc = check_mlp(H, n, n_theta, B, nch);
  if (rc) return rc;
  if (!sys_ok(sys) || !prm || !pde || !qjets || !qbar || !part || row0 < 0 || (nch == 1 && !target)) return QC_ERR_ARG;
  const QcLayout L = qc_layout(H, n, n_theta, sys->K);
  if (part_stride < L.NP + 3) return QC_ERR_ARG;
  rc = qc_mlp_post_system(prm, L, to_sys(sys), to_pde(pde), qjets, target, qbar, part, part_stride, row0, B, nch,
                          (hipStream_t)stream);
  return rc ? rc : after_launch();
}

// a system's dataset as a source: uniform rows, target rows of n_eq / K floats
static QcSource system_source(const qc_step_system* s) {
  QcSource src;
  src.kind = QC_SOURCE_ROWS;
  src.res = {s->ds_X_res, s->ds_r, s->ds_n_res};
  src.ic = {s->ds_X_ic, s->ds_u_ic, s->ds_n_ic};
  src.bc = {s->ds_X_bc, s->ds_u_bc, s->ds_n_bc};
  src.w_res = s->n_eq;
  src.w_val = s->K;
  return src;
}

int qc_sample_dataset_system(float* X_res, float* target_res, int64_t n_res, int64_t off_res, float* X_val, float* target_val,
                             int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, const qc_step_system* sys,
                             uint64_t seed, uint64_t step, void* stream) {
  if (!sys || sys->K < 1 || sys->K > QC_KMAX || sys->n_eq < 1 || sys->n_eq > QC_EQMAX) return QC_ERR_ARG;
  return fill_batches({X_res, target_res, n_res, off_res, X_val, target_val, n_ic, off_ic, n_bc, off_bc, seed, step},
                      system_source(sys), stream);
}

// One pipeline of the two-stream step: the value pipeline (nch = 1) or the residual pipeline (nch = 6)
struct QcPipe {
  const float* X;
  float *ajets, *qjets, *qbar, *abar;
  float *u, *ub;   // amplitude encoding: initial-amplitude jets and their cotangents, else null
  int64_t B, row0;
  int nch;
  QcCircStore store;
};

// the forward half of a pipeline: pre network -> [amplitudes] -> circuit, and the launch status
static int pipe_forward(const qc_step_desc* d, const QcPipe& q, hipStream_t st) {
  const qc_program* p = d->prog;
  int rc;
  if ((rc = prog_pre_forward(p, q.X, d->params_dev, d->H, d->n, d->n_theta, q.ajets, q.B, q.nch, st))) return rc;
  if (q.u && (rc = qc_amp_forward(q.ajets, q.u, d->n, q.B, q.nch, st))) return rc;
  rc = p->fam->fwd(p, (const QcTrig*)d->trig_dev, d->umat_dev, q.u ? q.u : q.ajets, q.qjets, q.B, q.nch, q.store, st);
  return rc ? rc : after_launch();
}

// forward half -> post -> circuit adjoint -> [amplitude adjoint] -> pre adjoint, on one stream
// `sys` (the system step): the K-row layout, and the system post stage on the pipeline's targets in place of post_impl
static int run_pipeline(const qc_step_desc* d, const QcPipe& q, hipStream_t st, const QcTarget& tg,
                        const qc_step_system* sys = nullptr) {
  const qc_program* p = d->prog;
  const int n = d->n, H = d->H;
  const QcTrig* trig = (const QcTrig*)d->trig_dev;
  float* part_theta = d->part_dev + qc_layout(H, n, d->n_theta, sys ? sys->K : 1, 0, prog_n_in(p)).oTh;
  if (!q.X || !q.ajets || !q.qjets || !q.qbar || !q.abar || (p->n_u4 > 0 && !d->umat_dev)) return QC_ERR_ARG;
  int rc;
  if ((rc = pipe_forward(d, q, st))) return rc;
  const float* cin = q.u ? q.u : q.ajets;
  float* cout = q.u ? q.ub : q.abar;
  // abar is written only by the adjoint sweep below: its head serves as per-point cotangent scratch here
  if (sys) {
    if ((rc = qc_post_system(d->params_dev, H, n, d->n_theta, sys, &d->pde, q.qjets,
                             q.nch == 6 ? sys->target_res_dev : sys->target_val_dev, q.qbar, d->part_dev, d->part_stride,
                             q.row0, q.B, q.nch, st))) return rc;
  } else if ((rc = post_impl(2, q.X, d->params_dev, H, n, d->n_theta, &d->pde, q.qjets, q.abar, q.nch == 6 ? q.abar + q.B : nullptr,
                             nullptr, nullptr, q.qbar, d->part_dev, d->part_stride, q.row0, q.B, q.nch, st, tg, prog_n_in(p)))) return rc;
  if ((rc = p->fam->bwd(p, trig, d->umat_dev, cin, q.qbar, cout, part_theta, d->part_stride, q.row0, q.B, q.nch, q.store, st)) ||
      (rc = after_launch())) return rc;
  if (q.u && (rc = qc_amp_backward(q.ajets, q.ub, q.abar, n, q.B, q.nch, st))) return rc;
  return prog_pre_backward(p, q.X, d->params_dev, H, n, d->n_theta, q.ajets, q.abar, d->part_dev, d->part_stride, q.row0, q.B,
                           q.nch, st);
}

// Everything the step entry points differ in, built by the entry that validated its records.  `tg`: where the post stage
// takes its targets and its operator from (a balancer comes with it); `src`: where QC_PHASE_SAMPLE takes the batches `b`
// from.  The dataset kinds gather rows and targets (and operator rows) AHEAD of the stages, in the merged form too (the
// merged pre stage then runs with its own draw off, so its instantiations are the analytic step's); nothing else in the
// step depends on the source.
// `sys` (the system step): K last-layer rows in the layout, the system post stage in both pipelines, always the two-stream
// form; `tg` is then not read.  `cz` (the causal step): the causal fold in place of the plain row fold.  `gn` (the
// gradient-norm step, never with a communicator): the class fold and the combination in place of both reduction levels; the
// optimiser launch then takes flat_dev.  `tt_data` and `tt_coef` (the seven-channel step, both or neither): the operator
// rows gathered behind the batches, tt_run_pipeline as the residual pipeline, the value pipeline without a store, always
// the two-stream form, nothing asked of the step workspace.
struct QcStepPlan {
  QcTarget tg;
  QcBatches b;
  QcSource src;
  const qc_step_system* sys = nullptr;
  const QcCausal* cz = nullptr;
  const QcGradnorm* gn = nullptr;
  const qc_step_data* tt_data = nullptr;
  const qc_step_coef_tt* tt_coef = nullptr;
};
// the seven-channel pieces of a step (behind their stages, below)
static int tt_gather_coef(const QcBatches& b, const qc_step_data* t, float* coef_res, const float* ds_coef, void* stream);
static int tt_run_pipeline(const qc_step_desc* d, const qc_step_data* t, const qc_step_coef_tt* cf, const QcLayout& L, hipStream_t st);

// The tail of every step: the partial rows of the stages -> flat_dev [gradient | 3 loss sums] -> the optimiser
static int step_tail(const qc_step_desc* d, const QcStepPlan& plan, const QcLayout& L, int64_t rows_res, int64_t rows_val,
                     int phases, hipStream_t st) {
  int rc;
  // the balanced step: the optimiser launch forms the balancer's three gradient entries from the reduced loss columns
  const QcBal* bal = !plan.sys && plan.tg.kind == QC_TARGET_BAL ? &plan.tg.bal : nullptr;
  if ((phases & QC_PHASE_GRADS) && plan.gn) {
    // value tile k wrote row rows_res + k in every stage and the IC points come first: the IC class ends on a tile boundary
    const int64_t rows_ic = plan.b.n_bc > 0 ? plan.b.n_ic / 64 : rows_val;
    qc_opt_gradnorm_fold(d->part_dev, rows_res, rows_ic, rows_val - rows_ic, d->part_stride, L.NP + 3, *plan.gn, d->flat_dev,
                         nullptr, st);
    if ((rc = after_launch())) return rc;
  } else if (phases & QC_PHASE_GRADS) {
    // the step owns its partial-row matrix, so the reduction folds it in place (two levels, fixed order);
    // with the update phase in the same call the second level rides in the optimiser launch
    const int64_t rows = rows_res + rows_val;
    const int RS = plan.cz ? qc_opt_causal_fold(d->part_dev, rows, rows_res, d->part_stride, L.NP + 3, *plan.cz, st)
                           : qc_opt_fold_rows(d->part_dev, rows, d->part_stride, L.NP + 3, st);
    if ((phases & QC_PHASE_UPDATE) && !d->comm) {
      QcOptHyper h;
      memcpy(&h, &d->hyper, sizeof(h));
      qc_opt_adam_fold(d->part_dev, d->part_stride, RS, d->flat_dev, L.NP, d->params_dev, d->m_dev, d->v_dev,
                       (QcOptState*)d->opt_state_dev, h, d->hist_dev, d->hist_cap, d->prog, L.oTh, (QcTrig*)d->trig_dev, st,
                       bal);
      return after_launch();
    }
    if ((rc = qc_reduce_rows(d->part_dev, RS, d->part_stride, L.NP + 3, d->flat_dev, st))) return rc;
    // data parallelism inside the library: sum the flat [gradient | 3 loss sums] vector over the ranks (RCCL, same stream)
    if (d->comm && (phases & QC_PHASE_UPDATE) && (rc = qc_comm_allreduce(d->flat_dev, L.NP + 3, d->comm, st))) return rc;
  }
  if (!(phases & QC_PHASE_UPDATE)) return QC_OK;
  return adam_step_impl(d->flat_dev, L.NP, d->params_dev, d->m_dev, d->v_dev, d->opt_state_dev, &d->hyper, d->hist_dev,
                        d->hist_cap, d->prog, L.oTh, d->trig_dev, st, bal);
}

// The step behind every step entry point: the plan's records are validated by its entry, the descriptor here.
static int fused_step(const qc_step_desc* d, const QcStepPlan& plan, int phases, void* stream) {
  const QcTarget& tg = plan.tg;
  const qc_step_system* sys = plan.sys;
  const bool tt = plan.tt_data != nullptr;
  if (!d->part_dev || !d->flat_dev || !plan.src.holds(plan.b)) return QC_ERR_ARG;
  if (!sys && ((tg.kind == QC_TARGET_ANALYTIC && !problem_ok(d->pde.problem)) || !tg.ok(2, 6, d->pde.problem))) return QC_ERR_ARG;
  int rc = check_step_desc(d, false, nullptr);
  if (rc) return rc;
  // no kernel family: n > 20 (refused above by the network's shape) or EMBED gates outside 2 <= n <= 5 (qc_program_create)
  if (!d->prog->fam) return QC_ERR_UNSUPPORTED;
  const int n = d->n, H = d->H;
  const QcLayout L = qc_layout(H, n, d->n_theta, sys ? sys->K : 1, sys ? 0 : tg.n_op(), prog_n_in(d->prog));
  const int64_t rows_res = d->B_res > 0 ? qc_ceil_div(d->B_res, 64) : 0;
  const int64_t rows_val = d->B_val > 0 ? qc_ceil_div(d->B_val, 64) : 0;
  const int64_t rows = rows_res + rows_val;
  if (rows <= 0 || rows > d->part_rows_cap || d->part_stride < L.NP + 3) return QC_ERR_ARG;
  if ((phases & QC_PHASE_UPDATE) && (!d->m_dev || !d->v_dev || !d->opt_state_dev)) return QC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  // seven channels: no kept final states, no amplitude encoding, nothing asked of the workspace
  const QcStepLayout ws = tt ? QcStepLayout{0, true} : step_layout(d->prog, d->B_res, d->B_val, d->circ_ws_dev, d->circ_ws_bytes);

  // (in the merged form below the first stage draws the points itself)
  const bool draw_in_stage = plan.src.kind == QC_SOURCE_DRAW && (phases & QC_PHASE_SAMPLE) && (phases & QC_PHASE_GRADS) && merged_ok(d);   // (never a system's)
  if ((phases & QC_PHASE_SAMPLE) && !draw_in_stage && (rc = fill_batches(plan.b, plan.src, st))) return rc;
  if ((phases & QC_PHASE_SAMPLE) && tt && (rc = tt_gather_coef(plan.b, plan.tt_data, plan.tt_coef->coef_res_dev, plan.tt_coef->ds_coef, st)))
    return rc;
  // register family, angle encoding, both pipelines present, final-state store available: every stage is ONE launch
  // over the value tiles and the residual tiles together (no side stream, 9 launches per step); QC_NO_MERGE=1 keeps
  // the two-stream form below
  const bool merged = !sys && !tt && (phases & QC_PHASE_GRADS) && merged_ok(d);
  if (merged) {
    for (int stage = 0; stage < QC_STAGE_COUNT; ++stage)
      if ((rc = merged_stage(d, stage, st, draw_in_stage && stage == QC_STAGE_PRE_FWD, tg))) return rc;
    if ((rc = after_launch())) return rc;
  }
  if ((phases & QC_PHASE_GRADS) && !merged) {
    if (!ws.fits) return QC_ERR_ARG;
    // the two pipelines are independent until the row reduction: fork the value pipeline onto a side
    // stream (not for the HBM family, where both may share the statevector workspace)
    QcSide* side = (d->B_res > 0 && d->B_val > 0 && d->prog->fam != &qc_family_hbm) ? side_stream() : nullptr;
    const hipStream_t sv = side_fork(side, st);
    const QcPipe val = {d->X_val_dev, d->ajets_val_dev, d->qjets_val_dev, d->qbar_val_dev, d->abar_val_dev, ws.u_val,
                        ws.ub_val, d->B_val, rows_res, 1, ws.val};
    const QcPipe res = {d->X_res_dev, d->ajets_res_dev, d->qjets_res_dev, d->qbar_res_dev, d->abar_res_dev, ws.u_res,
                        ws.ub_res, d->B_res, 0, 6, ws.res};
    if (d->B_val > 0 && (rc = run_pipeline(d, val, sv, tg.value_side(), sys))) return rc;
    if (d->B_res > 0 && (rc = tt ? tt_run_pipeline(d, plan.tt_data, plan.tt_coef, L, st) : run_pipeline(d, res, st, tg, sys)))
      return rc;
    if ((rc = side_join(side, st))) return rc;
  }
  return step_tail(d, plan, L, rows_res, rows_val, phases, st);
}

// the plan of the entry points that take the optional records of the public header: no data: analytic targets and the
// coordinate draw; data: tabulated targets and its dataset's rows; `cf`: with one operator row per residual point (no
// residual points: the plain tabulated step); `ad`: the residual rows from its CDF
static QcStepPlan plan_from(const qc_step_desc* d, const qc_step_data* t, const qc_step_coef* cf, const qc_step_adapt* ad) {
  const bool table = cf && d->B_res > 0;
  const QcTarget tg = !t      ? QcTarget{}
                      : table ? QcTarget::with_coef(t->target_res_dev, t->target_val_dev, cf->coef_res_dev)
                              : QcTarget::tabulated(t->target_res_dev, t->target_val_dev, t->c_u);
  return {tg, step_batches(d, t), make_source(t, cf, cf ? cf->coef_res_dev : nullptr, ad, d->sample_bc_face_points)};
}

int qc_fused_pinn_residual_step(const qc_step_desc* d, int phases, void* stream) {
  if (!d) return QC_ERR_ARG;
  return fused_step(d, plan_from(d, nullptr, nullptr, nullptr), phases, stream);
}

int qc_fused_pinn_data_step(const qc_step_desc* d, const qc_step_data* data, int phases, void* stream) {
  if (!data || !d) return QC_ERR_ARG;
  return fused_step(d, plan_from(d, data, nullptr, nullptr), phases, stream);
}

int qc_fused_pinn_coef_step(const qc_step_desc* d, const qc_step_data* data, const qc_step_coef* coef, int phases,
                            void* stream) {
  if (!data || !coef || !d) return QC_ERR_ARG;
  return fused_step(d, plan_from(d, data, coef, nullptr), phases, stream);
}

// the trainable operator, with or without residual points
int qc_fused_pinn_inverse_step(const qc_step_desc* d, const qc_step_data* data, const qc_step_learn* learn, int phases,
                               void* stream) {
  if (!data || !learn_ok(learn) || !d) return QC_ERR_ARG;
  QcStepPlan plan = plan_from(d, data, nullptr, nullptr);
  plan.tg = QcTarget::learned(data->target_res_dev, data->target_val_dev, to_learn(learn, d->opt_state_dev));
  return fused_step(d, plan, phases, stream);
}

// the tabulated step under balanced loss weights
int qc_fused_pinn_balanced_step(const qc_step_desc* d, const qc_step_data* data, const qc_step_balance* bal, int phases,
                                void* stream) {
  if (!data || !bal_ok(bal) || !d) return QC_ERR_ARG;
  QcStepPlan plan = plan_from(d, data, nullptr, nullptr);
  plan.tg = QcTarget::balanced(data->target_res_dev, data->target_val_dev, data->c_u, to_bal(bal));
  return fused_step(d, plan, phases, stream);
}

int qc_fused_pinn_adaptive_step(const qc_step_desc* d, const qc_step_data* data, const qc_step_coef* coef,
                                const qc_step_adapt* adapt, int phases, void* stream) {
  if (!d || !data || !adapt || d->B_res <= 0) return QC_ERR_ARG;
  return fused_step(d, plan_from(d, data, coef, adapt), phases, stream);
}

int qc_fused_pinn_system_step(const qc_step_desc* d, const qc_step_system* sys, int phases, void* stream) {
  if (!d || !sys_ok(sys) || (d->B_val > 0 && !sys->target_val_dev)) return QC_ERR_ARG;
  if (d->prog && d->prog->ff_m > 0) return QC_ERR_UNSUPPORTED;   // the system post stage lays W1 out as [H][3]
  const QcBatches b = {(float*)d->X_res_dev, sys->target_res_dev, d->B_res, d->sample_off_res, (float*)d->X_val_dev,
                       sys->target_val_dev, d->n_ic, d->sample_off_ic, d->B_val - d->n_ic, d->sample_off_bc, d->sample_seed,
                       d->sample_step};
  const QcSource src = system_source(sys);
  if ((phases & QC_PHASE_SAMPLE) && !src.ok(b)) return QC_ERR_ARG;   // ahead of everything the descriptor is asked
  if (d->H >= 1 && d->n >= 1 && d->n_theta >= 0 && d->part_stride < qc_layout(d->H, d->n, d->n_theta, sys->K).NP + 3)
    return QC_ERR_ARG;
  QcStepPlan plan = {QcTarget{}, b, src};
  plan.sys = sys;
  return fused_step(d, plan, phases, stream);
}

// ---- causal weighting of the residual slabs
static_assert(QC_CAUSAL_SLABS == QC_CAUSAL_MAX_SLABS && QC_CAUSAL_STATE_WORDS(1) == QC_CAUSAL_HEAD + 2, "causal record");
// THE validity rule of a causal record: slab count in range, an aligned state record, eps0 >= 0, growth, eps_max and delta
// finite and positive, a history buffer behind a positive capacity
static bool causal_ok(const qc_step_causal* c) {
  if (!c || c->n_slabs < 2 || c->n_slabs > QC_CAUSAL_MAX_SLABS || !c->state_dev || ((uintptr_t)c->state_dev & 3)) return false;
  if (!isfinite(c->eps0) || c->eps0 < 0.f || !pos_finite(c->eps_growth) || !pos_finite(c->eps_max) || !pos_finite(c->delta)) return false;
  return c->hist_cap >= 0 && (c->hist_cap == 0 || c->hist_dev);
}
static QcCausal to_causal(const qc_step_causal* c, int64_t tile_off) {
  QcCausal q;
  q.M = c->n_slabs;
  q.tile_off = (int)(tile_off % c->n_slabs);
  q.growth = c->eps_growth; q.eps_max = c->eps_max; q.delta = c->delta;
  q.rec = (float*)c->state_dev;
  const bool hist = c->hist_dev && c->hist_cap > 0;
  q.hist = hist ? c->hist_dev : nullptr;
  q.hist_cap = hist ? c->hist_cap : 0;
  return q;
}

int qc_causal_init(void* state_dev, const qc_step_causal* causal, void* stream) {
  if (!state_dev || ((uintptr_t)state_dev & 3) || !causal) return QC_ERR_ARG;
  qc_step_causal c = *causal;   // the rule asks for a record: the one being seeded serves
  c.state_dev = state_dev;
  if (!causal_ok(&c)) return QC_ERR_ARG;
  qc_opt_causal_init((float*)state_dev, causal->n_slabs, causal->eps0, (hipStream_t)stream);
  return after_launch();
}

int qc_sample_dataset_slabs(float* X_res, float* target_res, int64_t n_res, int64_t off_res, float* X_val, float* target_val,
                            int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, const qc_step_data* t, int n_slabs,
                            const int64_t* slab_lo, uint64_t seed, uint64_t step, void* stream) {
  if (!t) return QC_ERR_ARG;
  QcSource s = make_source(t, nullptr, nullptr, nullptr);
  s.kind = QC_SOURCE_SLABS;
  s.slab_lo = slab_lo;
  s.n_slabs = n_slabs;
  return fill_batches({X_res, target_res, n_res, off_res, X_val, target_val, n_ic, off_ic, n_bc, off_bc, seed, step}, s, stream);
}

int qc_causal_fold(float* part, int64_t rows, int64_t rows_res, int64_t stride, int ncols, const qc_step_causal* causal,
                   float* flat, void* stream) {
  if (!part || !flat || ncols < 3 || stride < ncols || rows < 1 || rows >= ((int64_t)1 << 31) || !causal_ok(causal)) return QC_ERR_ARG;
  if (rows_res < 1 || rows_res > rows || rows_res % causal->n_slabs != 0) return QC_ERR_ARG;
  const int RS = qc_opt_causal_fold(part, rows, rows_res, stride, ncols, to_causal(causal, 0), (hipStream_t)stream);
  int rc = after_launch();
  if (rc) return rc;
  return qc_reduce_rows(part, RS, stride, ncols, flat, stream);
}

int qc_fused_pinn_causal_step(const qc_step_desc* d, const qc_step_data* t, const qc_step_causal* causal, int phases,
                              void* stream) {
  if (!d || !t || !causal_ok(causal)) return QC_ERR_ARG;
  if (d->comm) return QC_ERR_UNSUPPORTED;   // the slab losses of the ranks would need a reduction of their own
  if (d->B_res <= 0 || d->B_res % (64 * (int64_t)causal->n_slabs) != 0 || d->sample_off_res < 0 || d->sample_off_res % 64 != 0)
    return QC_ERR_ARG;
  if (d->part_rows_cap >= ((int64_t)1 << 31)) return QC_ERR_ARG;
  QcSource s = make_source(t, nullptr, nullptr, nullptr, d->sample_bc_face_points);
  s.kind = QC_SOURCE_SLABS;
  s.slab_lo = causal->slab_lo_dev;
  s.n_slabs = causal->n_slabs;
  const QcCausal cz = to_causal(causal, d->sample_off_res / 64);
  QcStepPlan plan = {QcTarget::tabulated(t->target_res_dev, t->target_val_dev, t->c_u), step_batches(d, t), s};
  plan.cz = &cz;
  return fused_step(d, plan, phases, stream);
}

// ---- gradient-norm loss weights
static_assert(QC_GRADNORM_WORDS == QC_GRADNORM_STATE_WORDS && QC_GRADNORM_COLS == QC_GRADNORM_HIST_COLS, "gradient-norm record");
// THE validity rule of a gradient-norm record: an aligned state record, alpha in [0, 1], every >= 1, lam_max and the two
// starting weights finite and positive, a history buffer behind a positive capacity
static bool gradnorm_ok(const qc_step_gradnorm* g) {
  if (!g || !g->state_dev || ((uintptr_t)g->state_dev & 3)) return false;
  if (!(g->alpha >= 0.f && g->alpha <= 1.f) || g->every < 1) return false;
  if (!pos_finite(g->lam_max) || !pos_finite(g->lam0_bc) || !pos_finite(g->lam0_ic)) return false;
  return g->hist_cap >= 0 && (g->hist_cap == 0 || g->hist_dev);
}
static QcGradnorm to_gradnorm(const qc_step_gradnorm* g, float w_res, float w_bc, float w_ic) {
  QcGradnorm q;
  q.alpha = g->alpha; q.lam_max = g->lam_max; q.every = g->every;
  q.w[0] = w_res; q.w[1] = w_bc; q.w[2] = w_ic;
  q.rec = g->state_dev;
  const bool hist = g->hist_dev && g->hist_cap > 0;
  q.hist = hist ? g->hist_dev : nullptr;
  q.hist_cap = hist ? g->hist_cap : 0;
  return q;
}

int qc_gradnorm_init(float* state_dev, const qc_step_gradnorm* gn, void* stream) {
  if (!state_dev || ((uintptr_t)state_dev & 3) || !gn) return QC_ERR_ARG;
  qc_step_gradnorm g = *gn;   // the rule asks for a record: the one being seeded serves
  g.state_dev = state_dev;
  if (!gradnorm_ok(&g)) return QC_ERR_ARG;
  qc_opt_gradnorm_init(state_dev, gn->lam0_bc, gn->lam0_ic, (hipStream_t)stream);
  return after_launch();
}

int qc_gradnorm_fold(float* part, int64_t rows, int64_t rows_res, int64_t rows_ic, int64_t stride, int ncols,
                     const qc_step_gradnorm* gn, float* flat, float* class_out, void* stream) {
  if (!part || !flat || ncols < 4 || stride < ncols || rows < 1 || rows >= ((int64_t)1 << 31) || !gradnorm_ok(gn)) return QC_ERR_ARG;
  if (rows_res < 0 || rows_ic < 0 || rows_res > rows || rows_ic > rows - rows_res) return QC_ERR_ARG;
  qc_opt_gradnorm_fold(part, rows_res, rows_ic, rows - rows_res - rows_ic, stride, ncols, to_gradnorm(gn, 1.f, 1.f, 1.f), flat,
                       class_out, (hipStream_t)stream);
  return after_launch();
}

int qc_fused_pinn_gradnorm_step(const qc_step_desc* d, const qc_step_data* t, const qc_step_coef* cf, const qc_step_gradnorm* gn,
                                int phases, void* stream) {
  if (!d || !gradnorm_ok(gn) || (cf && !t)) return QC_ERR_ARG;
  if (d->comm) return QC_ERR_UNSUPPORTED;   // the class gradients of the ranks would need a reduction ahead of the ratio
  if (d->n_ic < 0 || d->B_val < d->n_ic) return QC_ERR_ARG;
  if (d->n_ic > 0 && d->B_val > d->n_ic && d->n_ic % 64 != 0) return QC_ERR_ARG;   // a value tile would mix IC and BC points
  if (d->part_rows_cap >= ((int64_t)1 << 31)) return QC_ERR_ARG;
  const QcGradnorm q = to_gradnorm(gn, d->hyper.w_res, d->hyper.w_bc, d->hyper.w_ic);
  QcStepPlan plan = plan_from(d, t, cf, nullptr);
  plan.gn = &q;
  return fused_step(d, plan, phases, stream);
}

// Scores of the dataset's residual rows [row0, row0 + rows): the forward half of the residual pipeline (pipe_forward, then
// qc_post mode 4) over chunks of at most B_res rows through the step's residual scratch, then |res - r| per row.  Between
// steps those buffers hold nothing that is read again.
int qc_dataset_scores(const qc_step_desc* d, const qc_step_data* t, const qc_step_coef* cf, int64_t row0, int64_t rows,
                      float* score, void* stream) {
  if (!d || !t || !score || d->B_res <= 0) return QC_ERR_ARG;
  if (!QcDsSeg{t->ds_X_res, t->ds_r, t->ds_n_res}.serves(1)) return QC_ERR_ARG;
  if (row0 < 0 || rows < 1 || row0 > t->ds_n_res || rows > t->ds_n_res - row0) return QC_ERR_ARG;
  if (cf && !cf->ds_coef) return QC_ERR_ARG;
  if (d->pde.problem != QC_PROBLEM_TABULATED) return QC_ERR_ARG;
  if (!d->ajets_res_dev || !d->qjets_res_dev || !d->qbar_res_dev) return QC_ERR_ARG;
  int rc = check_step_desc(d, true, [](const qc_step_desc* e) { return e->prog->fam != nullptr; });
  if (rc) return rc;
  const QcStepLayout ws = step_layout(d->prog, d->B_res, d->B_val, d->circ_ws_dev, d->circ_ws_bytes);
  if (!ws.fits) return QC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const QcPde pde = to_pde(&d->pde);
  float* uj = d->qbar_res_dev;   // [6][c]
  for (int64_t r = row0; r < row0 + rows; r += d->B_res) {
    const int64_t c = row0 + rows - r < d->B_res ? row0 + rows - r : d->B_res;
    // forward only: nothing is kept.  The HBM family runs a chunk in as many groups of tiles as its scratch holds (a
    // forward tile is never larger than the forward-and-adjoint tile the step sized it for), so no chunk needs shrinking
    const QcPipe q = {t->ds_X_res + 3 * r, d->ajets_res_dev, d->qjets_res_dev, nullptr, nullptr, ws.u_res, nullptr, c, 0, 6,
                      {ws.res.p, ws.res.bytes, false}};
    if ((rc = pipe_forward(d, q, st))) return rc;
    if ((rc = post_impl(4, q.X, d->params_dev, d->H, d->n, d->n_theta, &d->pde, q.qjets, uj, nullptr, nullptr, nullptr, nullptr,
                        nullptr, 0, 0, c, 6, st, QcTarget{}, prog_n_in(d->prog)))) return rc;
    qc_adapt_score_launch(uj, c, pde, t->c_u, cf ? cf->ds_coef + (size_t)QC_COEF_N * r : nullptr, t->ds_r + r, score + r, st);
    if ((rc = after_launch())) return rc;
  }
  return QC_OK;
}

// ---- seven derivative channels (channel 6 = d2/dt2): stages and the coefficient step for equations second order in time
static_assert(QC_NCH_TT_N == QC_NCH_TT && QC_COEF_TT_N == QC_COEF_TT_COLS && QC_COEF_TT_N == QC_COEF_N + 1, "seven-channel counts");
// THE rule of what the seven-channel stages serve: the register family's qubit counts (whatever QC_FORCE_WAVE says: they
// have their own kernels), no EMBED gates, angle encoding, plain inputs, no angle map
static bool tt_prog_ok(const qc_program* p) {
  return p->n_qubits >= 2 && p->n_qubits <= 5 && p->n_embed == 0 && !p->amplitude && p->ff_m == 0 &&
         p->angle_map == QC_ANGLE_MAP_NONE;
}
static int check_mlp_tt(int H, int n, int n_theta, int64_t B) {
  const int rc = check_mlp(H, n, n_theta, B, 6);
  if (rc) return rc;
  return (n >= 2 && n <= 5) ? QC_OK : QC_ERR_UNSUPPORTED;
}

int qc_pre_forward_tt(const float* X, const float* prm, int H, int n, int n_theta, float* ajets, int64_t B, void* stream) {
  if (!X || !prm || !ajets) return QC_ERR_ARG;
  int rc = check_mlp_tt(H, n, n_theta, B);
  if (rc) return rc;
  rc = qc_tt_pre_fwd(X, prm, make_layout(H, n, n_theta), ajets, B, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_pre_backward_tt(const float* X, const float* prm, int H, int n, int n_theta, const float* abar, float* part,
                       int64_t part_stride, int64_t row0, int64_t B, void* stream) {
  if (!X || !prm || !abar || !part || row0 < 0) return QC_ERR_ARG;
  int rc = check_mlp_tt(H, n, n_theta, B);
  if (rc) return rc;
  const QcLayout L = make_layout(H, n, n_theta);
  if (part_stride < L.NP) return QC_ERR_ARG;
  rc = qc_tt_pre_bwd(X, prm, L, abar, part, part_stride, row0, B, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_forward_jets_tt(const qc_program* p, const void* trig, const float* umat, const float* ajets, float* qjets, int64_t B,
                       void* stream) {
  if (!p || !trig || B <= 0 || !ajets || !qjets || (p->n_u4 > 0 && !umat)) return QC_ERR_ARG;
  if (!tt_prog_ok(p)) return QC_ERR_UNSUPPORTED;
  const int rc = qc_tt_circ_fwd(p, (const QcTrig*)trig, umat, ajets, qjets, B, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_backward_jets_tt(const qc_program* p, const void* trig, const float* umat, const float* ajets, const float* qbar,
                        float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B, void* stream) {
  if (!p || !trig || B <= 0 || !ajets || !qbar || !abar || !part || (p->n_u4 > 0 && !umat)) return QC_ERR_ARG;
  if (part_stride < p->n_params || row0 < 0) return QC_ERR_ARG;
  if (!tt_prog_ok(p)) return QC_ERR_UNSUPPORTED;
  const int rc = qc_tt_circ_bwd(p, (const QcTrig*)trig, umat, ajets, qbar, abar, part, part_stride, row0, B, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_post_coef_tt(const float* prm, int H, int n, int n_theta, const qc_pde* pde, const float* qjets, const float* target,
                    const float* coef, float* cot, float* qbar, float* part, int64_t part_stride, int64_t row0, int64_t B,
                    void* stream) {
  if (!prm || !pde || !qjets || !target || !coef || !cot || !qbar || !part || row0 < 0) return QC_ERR_ARG;
  if (pde->problem != QC_PROBLEM_TABULATED) return QC_ERR_ARG;
  int rc = check_mlp_tt(H, n, n_theta, B);
  if (rc) return rc;
  const QcLayout L = make_layout(H, n, n_theta);
  if (part_stride < L.NP + 3) return QC_ERR_ARG;
  rc = qc_tt_post(2, prm, L, to_pde(pde), qjets, target, coef, cot, qbar, part, part_stride, row0, B, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

int qc_post_jets_tt(int mode, const float* prm, int H, int n, int n_theta, const float* qjets, float* io, float* qbar,
                    float* part, int64_t part_stride, int64_t row0, int64_t B, void* stream) {
  if ((mode != 3 && mode != 4) || !prm || !qjets || !io) return QC_ERR_ARG;
  int rc = check_mlp_tt(H, n, n_theta, B);
  if (rc) return rc;
  const QcLayout L = make_layout(H, n, n_theta);
  if (mode == 3 && (!qbar || !part || row0 < 0 || part_stride < L.NP)) return QC_ERR_ARG;
  QcPde pde;
  memset(&pde, 0, sizeof(pde));   // not read by these modes
  rc = qc_tt_post(mode, prm, L, pde, qjets, nullptr, nullptr, io, qbar, part, part_stride, row0, B, (hipStream_t)stream);
  return rc ? rc : after_launch();
}

// the operator rows of the residual batch: the dataset gather once more, on the counters of the gather that filled the
// points (same row index), with the 8-column table as the residual segment's target rows
static int tt_gather_coef(const QcBatches& b, const qc_step_data* t, float* coef_res, const float* ds_coef, void* stream) {
  if (b.n_res <= 0) return QC_OK;
  if (!coef_res || !ds_coef) return QC_ERR_ARG;
  QcSource s;
  s.kind = QC_SOURCE_ROWS;
  s.res = {t->ds_X_res, ds_coef, t->ds_n_res};
  s.w_res = QC_COEF_TT_N;
  return fill_batches({b.X_res, coef_res, b.n_res, b.off_res, nullptr, nullptr, 0, 0, 0, 0, b.seed, b.step}, s, stream);
}

int qc_sample_dataset_coef_tt(float* X_res, float* target_res, int64_t n_res, int64_t off_res, float* X_val, float* target_val,
                              int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, float* coef_res, const qc_step_data* t,
                              const qc_step_coef_tt* cf, uint64_t seed, uint64_t step, void* stream) {
  if (!t || !cf) return QC_ERR_ARG;
  const QcBatches b = {X_res, target_res, n_res, off_res, X_val, target_val, n_ic, off_ic, n_bc, off_bc, seed, step};
  const QcSource src = make_source(t, nullptr, nullptr, nullptr);
  if (!src.ok(b) || (n_res > 0 && (!coef_res || !cf->ds_coef))) return QC_ERR_ARG;   // nothing is written on a refusal
  const int rc = fill_batches(b, src, stream);
  return rc ? rc : tt_gather_coef(b, t, coef_res, cf->ds_coef, stream);
}

// the residual pipeline of the seven-channel step, on one stream: pre -> circuit -> post (coefficient form) -> circuit
// adjoint -> pre adjoint.  The [7][B_res] channel cotangents are the head of abar_res_dev (written by the adjoint sweep only)
static int tt_run_pipeline(const qc_step_desc* d, const qc_step_data* t, const qc_step_coef_tt* cf, const QcLayout& L,
                           hipStream_t st) {
  const qc_program* p = d->prog;
  const QcTrig* trig = (const QcTrig*)d->trig_dev;
  const int64_t B = d->B_res;
  int rc;
  if ((rc = qc_tt_pre_fwd(d->X_res_dev, d->params_dev, L, d->ajets_res_dev, B, st))) return rc;
  if ((rc = qc_tt_circ_fwd(p, trig, d->umat_dev, d->ajets_res_dev, d->qjets_res_dev, B, st)) || (rc = after_launch())) return rc;
  if ((rc = qc_tt_post(2, d->params_dev, L, to_pde(&d->pde), d->qjets_res_dev, t->target_res_dev, cf->coef_res_dev, d->abar_res_dev,
                       d->qbar_res_dev, d->part_dev, d->part_stride, 0, B, st))) return rc;
  if ((rc = qc_tt_circ_bwd(p, trig, d->umat_dev, d->ajets_res_dev, d->qbar_res_dev, d->abar_res_dev, d->part_dev + L.oTh,
                           d->part_stride, 0, B, st)) || (rc = after_launch())) return rc;
  if ((rc = qc_tt_pre_bwd(d->X_res_dev, d->params_dev, L, d->abar_res_dev, d->part_dev, d->part_stride, 0, B, st))) return rc;
  return after_launch();
}

int qc_fused_pinn_coef_tt_step(const qc_step_desc* d, const qc_step_data* t, const qc_step_coef_tt* cf, int phases, void* stream) {
  if (!d || !t || !cf || !d->part_dev || !d->flat_dev) return QC_ERR_ARG;
  if (d->pde.problem != QC_PROBLEM_TABULATED) return QC_ERR_ARG;
  if (!d->prog || !d->trig_dev || !d->params_dev) return QC_ERR_ARG;
  if (!tt_prog_ok(d->prog)) return QC_ERR_UNSUPPORTED;
  QcStepPlan plan = plan_from(d, t, nullptr, nullptr);   // tabulated targets, the dataset's rows
  if (!plan.src.holds(plan.b)) return QC_ERR_ARG;
  // umat and the residual buffers are asked for whatever the phases, and the sampler's inputs ahead of rows and stride
  const int rc = check_step_desc(d, true, nullptr);
  if (rc) return rc;
  if (d->B_res > 0 && (!cf->coef_res_dev || !d->X_res_dev || !d->ajets_res_dev || !d->qjets_res_dev || !d->qbar_res_dev ||
                       !d->abar_res_dev))
    return QC_ERR_ARG;
  if ((phases & QC_PHASE_SAMPLE) && (!plan.src.ok(plan.b) || (d->B_res > 0 && !cf->ds_coef))) return QC_ERR_ARG;
  plan.tt_data = t;
  plan.tt_coef = cf;
  return fused_step(d, plan, phases, stream);
}

// ---- ensembles: M members per launch sequence (the merged form of the analytic step, every stage over all members' tiles)
static bool ens_supported(const qc_step_desc* d) {
  const qc_program* p = d->prog;
  return p->fam == &qc_family_reg && !p->amplitude && p->ff_m == 0 && p->n_embed == 0 &&
         (d->H < 1 || qc_mlp_ens_ok(qc_layout(d->H, d->n, d->n_theta)));
}

int qc_ensemble_strides(const qc_step_desc* d, int M, qc_step_ensemble* out) {
  if (!d || !out || !d->prog || M < 1 || d->B_res < 0 || d->B_val < 0 || d->H < 1 || d->n < 1 || d->n_theta < 0 || d->hist_cap < 0)
    return QC_ERR_ARG;
  const QcLayout L = qc_layout(d->H, d->n, d->n_theta, 1, 0, prog_n_in(d->prog));
  out->M = M;
  out->params_stride = L.NP;
  out->flat_stride = L.NP + 3;
  out->hist_stride = d->hist_cap;
  out->trig_stride = (int64_t)round256(qc_trig_bytes(d->prog));
  out->x_res_stride = 3 * d->B_res;
  out->x_val_stride = 3 * d->B_val;
  out->jets_res_stride = 6 * (int64_t)d->n * d->B_res;
  out->jets_val_stride = (int64_t)d->n * d->B_val;
  out->ws_stride = (int64_t)round256(qc_step_workspace_bytes(d->prog, d->B_res, d->B_val));
  out->pde_dev = nullptr;
  out->hyper_dev = nullptr;
  return QC_OK;
}

int qc_fused_pinn_ensemble_step(const qc_step_desc* d, const qc_step_ensemble* ens, int phases, void* stream) {
  if (!d || !ens || d->comm) return QC_ERR_ARG;
  if (ens->M < 1 || ens->M > 65535) return QC_ERR_ARG;
  if (!d->part_dev || !d->flat_dev) return QC_ERR_ARG;
  if (!problem_ok(d->pde.problem) || d->sample_bc_face_points < QC_BC_RANDOM_FACE) return QC_ERR_ARG;
  int rc = check_step_desc(d, false, ens_supported);
  if (rc) return rc;
  const qc_program* pg = d->prog;
  if (pg->n_u4 > 0 && !d->umat_dev) return QC_ERR_ARG;
  const QcLayout L = qc_layout(d->H, d->n, d->n_theta);
  const size_t store = qc_family_reg.store_bytes(pg, 6, d->B_res > 0 ? d->B_res : 0);
  if (d->B_res <= 0 || d->B_val <= 0 || d->n_ic < 0 || d->n_ic > d->B_val || !d->X_res_dev || !d->X_val_dev || !d->ajets_res_dev ||
      !d->qjets_res_dev || !d->qbar_res_dev || !d->abar_res_dev || !d->ajets_val_dev || !d->qjets_val_dev || !d->qbar_val_dev ||
      !d->abar_val_dev || !d->circ_ws_dev || d->circ_ws_bytes < store)
    return QC_ERR_ARG;
  const int64_t rows_res = qc_ceil_div(d->B_res, 64), rows_val = qc_ceil_div(d->B_val, 64), rows = rows_res + rows_val;
  if (rows > d->part_rows_cap || d->part_stride < L.NP + 3) return QC_ERR_ARG;
  if ((phases & QC_PHASE_UPDATE) && (!d->m_dev || !d->v_dev || !d->opt_state_dev)) return QC_ERR_ARG;
  if (ens->params_stride < L.NP || ens->flat_stride < L.NP + 3 || (d->hist_dev && ens->hist_stride < d->hist_cap) ||
      ens->trig_stride < (int64_t)qc_trig_bytes(pg) || (ens->trig_stride & 255) || ens->x_res_stride < 3 * d->B_res ||
      ens->x_val_stride < 3 * d->B_val || ens->jets_res_stride < 6 * (int64_t)d->n * d->B_res ||
      ens->jets_val_stride < (int64_t)d->n * d->B_val || ens->ws_stride < (int64_t)store || (ens->ws_stride & 255) ||
      ((uintptr_t)ens->pde_dev & 7) || ((uintptr_t)ens->hyper_dev & 7))
    return QC_ERR_ARG;
  const QcEns e = {ens->M, ens->params_stride, ens->flat_stride, ens->hist_stride, ens->trig_stride, ens->x_res_stride,
                   ens->x_val_stride, ens->jets_res_stride, ens->jets_val_stride, d->part_rows_cap * d->part_stride,
                   ens->ws_stride, (const QcPde*)ens->pde_dev, (const QcOptHyper*)ens->hyper_dev};
  hipStream_t st = (hipStream_t)stream;
  const QcTrig* trig = (const QcTrig*)d->trig_dev;
  float* chi_store = (float*)d->circ_ws_dev;
  const QcBatches b0 = step_batches(d, nullptr);
  if ((phases & QC_PHASE_SAMPLE) && !(phases & QC_PHASE_GRADS)) {
    // points alone: one draw per member, keyed seed + m (with the gradients the first stage draws them itself)
    QcSource src;
    src.face_pts = d->sample_bc_face_points;
    for (int m = 0; m < e.M; ++m) {
      QcBatches b = b0;
      b.X_res += m * e.X_res;
      b.X_val += m * e.X_val;
      b.seed += (uint64_t)m;
      if ((rc = fill_batches(b, src, st))) return rc;
    }
  }
  if (phases & QC_PHASE_GRADS) {
    QcPde pde;
    memcpy(&pde, &d->pde, sizeof(pde));
    if ((rc = qc_mlp_pre_fwd_ens(b0, (phases & QC_PHASE_SAMPLE) ? 1 : 0, d->sample_bc_face_points, d->params_dev, L,
                                 d->ajets_res_dev, d->ajets_val_dev, st, pg->angle_map, e)) ||
        (rc = qc_reg_circ_fwd_ens(pg, trig, d->umat_dev, d->ajets_res_dev, d->qjets_res_dev, d->B_res, chi_store,
                                  d->ajets_val_dev, d->qjets_val_dev, d->B_val, st, e)) ||
        (rc = qc_mlp_post_ens(d->params_dev, L, pde, d->X_res_dev, d->qjets_res_dev, d->abar_res_dev, d->abar_res_dev + d->B_res,
                              d->qbar_res_dev, 0, d->B_res, d->X_val_dev, d->qjets_val_dev, d->abar_val_dev, d->qbar_val_dev,
                              rows_res, d->B_val, d->part_dev, d->part_stride, st, e)) ||
        (rc = qc_reg_circ_bwd_ens(pg, trig, d->umat_dev, d->ajets_res_dev, d->qbar_res_dev, d->abar_res_dev, 0, d->B_res,
                                  chi_store, d->ajets_val_dev, d->qbar_val_dev, d->abar_val_dev, rows_res, d->B_val,
                                  d->part_dev + L.oTh, d->part_stride, st, e)) ||
        (rc = qc_mlp_pre_bwd_ens(d->X_res_dev, d->X_val_dev, d->params_dev, L, d->abar_res_dev, d->abar_val_dev, d->part_dev,
                                 d->part_stride, 0, rows_res, d->B_res, d->B_val, st, pg->angle_map, d->ajets_res_dev,
                                 d->ajets_val_dev, e)))
      return rc;
    if ((rc = after_launch())) return rc;
  }
  if (!(phases & (QC_PHASE_GRADS | QC_PHASE_UPDATE))) return QC_OK;
  QcOptHyper h;
  memcpy(&h, &d->hyper, sizeof(h));
  qc_opt_ens_tail(d->part_dev, (phases & QC_PHASE_GRADS) ? rows : 0, d->part_stride, d->flat_dev, L.NP, d->params_dev, d->m_dev,
                  d->v_dev, (QcOptState*)d->opt_state_dev, h, d->hist_dev, d->hist_cap, pg, L.oTh, (QcTrig*)d->trig_dev,
                  (phases & QC_PHASE_UPDATE) ? 1 : 0, e, st);
  return after_launch();
}

}  // extern "C"
