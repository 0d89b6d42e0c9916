// L-BFGS on the device: the second training phase (Adam, then L-BFGS on a fixed batch).  One single-block kernel behind the
// gradient reduction, the counterpart of k_adam_fast: it reads flat = [grad[NP] | L_r, L_bc, L_ic] evaluated at the current
// parameters, advances a state machine that lives in the caller's workspace (curvature pairs, line search, counters) and
// writes the NEXT point to evaluate into the parameters; no host read decides anything.  The rule is written out in
// include/qcpinn_hip.h (qc_lbfgs_step); tests/lbfgs_reference.py restates it in float64.
//
// Direction: the dot products the two-loop recursion needs (S.g, Y.g and the new pair against every kept one) come from
// ONE batched fixed-order reduction behind one barrier: wave w sweeps the rows w, w + 16, ... of [S | Y] once and forms
// that row's two or three products, so nothing is summed across waves.  The Gram entries S.Y and Y.Y of the kept pairs are
// carried in the workspace.  The recursion then runs on those scalars in one wave (lane j holds pair j) and yields
// d = sum_j cS_j s_j + cY_j y_j + cg g.  The scalars, the recursion and that combination are in double: the Gram form
// cancels large terms where the textbook loop works on a vector that has already become small, and in fp32 it missed the
// direction tolerance when the pairs are linearly dependent (NP < m); the stored vectors stay fp32.
#include "qc_internal.h"

namespace {

constexpr int LB_T = 1024, LB_WAVES = 16, LB_M = 32;   // == QC_LBFGS_MAX_HISTORY
constexpr int LB_EXTRA = 9;                            // scalars of the batch behind the 5 m pair products
constexpr int LB_NS = 5 * LB_M + LB_EXTRA;
enum { E_YS = 0, E_YY, E_GG, E_G1, E_NF, E_KK, E_K1, E_SG, E_YG };
enum { A_FIRST = 0, A_STEP, A_REJECT, A_RESET, A_STALL };

struct QcLbfgsArgs {
  const float* flat;
  int NP;
  float* prm;
  float* ws;
  QcLbfgsHyper hp;
  float* hist;
  int hist_cap;
  const QcGate* prog;
  int n_gates, theta_off, n_qubits;
  QcTrig* trig;
  QcDiagRuns runs;
};

template <int CTRL, int ROWS, bool BC>
__device__ __forceinline__ double lb_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xF, BC);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xF, BC);
  return __hiloint2double(hi, lo);
}

// sum over the wave in the fixed order of qc_wave_sum_to_lane63, the total in every lane
__device__ __forceinline__ double lb_wave_sum(double v) {
  v += lb_dpp<0xB1, 0xF, true>(v);
  v += lb_dpp<0x4E, 0xF, true>(v);
  v += lb_dpp<0x141, 0xF, true>(v);
  v += lb_dpp<0x140, 0xF, true>(v);
  v += lb_dpp<0x142, 0xA, false>(v);
  v += lb_dpp<0x143, 0xC, false>(v);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

__device__ __forceinline__ double lb_block_sum(double v, double* s_red) {
  v = lb_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < LB_WAVES; ++w) t += s_red[w];
  return t;
}

// the elements of this thread: i = tid, tid + 1024, ...; K > 0: at most K of them, their values cached in registers at [k]
template <int K, class F>
__device__ __forceinline__ void lb_each(int NP, int tid, F&& f) {
  if constexpr (K > 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = tid + k * LB_T;
      if (i < NP) f(i, k);
    }
  } else {
    for (int i = tid; i < NP; i += LB_T) f(i, 0);
  }
}

// (The trig buffer's tail, the per-gate entries and the diagonal-run tables from the NEW theta, is the one k_adam_fast
// runs: the gate stage of qc_common.h, loaded at kernel entry and read back from LDS behind the move.)

__device__ __forceinline__ float lb_first_t(float lr, float g1) { return lr * fminf(1.f, 1.f / g1); }

template <int K>
__global__ void __launch_bounds__(LB_T) k_lbfgs(QcLbfgsArgs a) {
  __shared__ double s_dot[LB_NS];
  __shared__ double s_SY[LB_M * LB_M], s_YY[LB_M * LB_M];
  __shared__ double s_cS[LB_M], s_cY[LB_M];
  __shared__ double s_red[LB_WAVES];
  // register path: g, g_k and s = t d of the call for the row sweeps, later the new theta for the tables
  __shared__ float s_v[K > 0 ? 3 * K * LB_T : 1];
  extern __shared__ __attribute__((aligned(16))) float s_stage[];   // the gate stage (qc_common.h)
  constexpr int KC = K > 0 ? K : 1;
  const int NP = a.NP, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const QcLbfgsHyper& hp = a.hp;
  const int m = hp.history;
  const QcLbfgsRec rec = *reinterpret_cast<const QcLbfgsRec*>(a.ws);
  const QcGateStage sg = qc_gate_stage_load(a.prog, a.n_gates, a.n_qubits, a.runs, s_stage, tid);
  float* const xk = a.ws + QC_LBFGS_REC_WORDS;
  float* const gk = xk + NP;
  float* const dd = gk + NP;
  float* const S = dd + NP;
  float* const Y = S + (size_t)m * NP;
  float* const rho = Y + (size_t)m * NP;
  float* const SY = rho + m;            // (high, low) float pairs: [m][m][2]
  float* const YY = SY + 2 * m * m;
  const float l_r = a.flat[NP], l_bc = a.flat[NP + 1], l_ic = a.flat[NP + 2];
  if (tid < m * m) {
    s_SY[tid] = (double)SY[2 * tid] + (double)SY[2 * tid + 1];
    s_YY[tid] = (double)YY[2 * tid] + (double)YY[2 * tid + 1];
  }
  float gv[KC], kv[KC], dv[KC], xv[KC], pv[KC];
  if constexpr (K > 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = tid + k * LB_T;
      gv[k] = kv[k] = dv[k] = xv[k] = pv[k] = 0.f;
      if (i < NP) {
        gv[k] = a.flat[i];
        kv[k] = gk[i];
        dv[k] = dd[i];
        xv[k] = xk[i];
        pv[k] = a.prm[i];
      }
    }
  }
  auto G = [&](int i, int k) { return K > 0 ? gv[k] : a.flat[i]; };
  auto GK = [&](int i, int k) { return K > 0 ? kv[k] : gk[i]; };
  auto D = [&](int i, int k) { return K > 0 ? dv[k] : dd[i]; };
  auto X = [&](int i, int k) { return K > 0 ? xv[k] : xk[i]; };
  auto P = [&](int i, int k) { return K > 0 ? pv[k] : a.prm[i]; };
  const float t_old = rec.t;

  // ---- the batch of dot products.  Row r of [S | Y] (wave r mod 16): S_j.g, S_j.y or Y_j.g, Y_j.y, s.Y_j  (s = t d,
  // y = g - g_k); the nine extras go to waves 15, 14, ...  Lane l sums elements l, l + 64, ... in double, then the wave.
  float *const vg = s_v, *const vk = s_v + K * LB_T, *const vs = s_v + 2 * K * LB_T;
  qc_gate_stage_store<LB_T>(sg, a.prog, a.n_gates, a.runs, tid);   // (published by the barriers below)
  if constexpr (K > 0) {
    lb_each<K>(NP, tid, [&](int i, int k) {
      vg[i] = gv[k];
      vk[i] = kv[k];
      vs[i] = t_old * dv[k];
    });
    __syncthreads();
  }
  auto VG = [&](int i) { return K > 0 ? vg[i] : a.flat[i]; };
  auto VK = [&](int i) { return K > 0 ? vk[i] : gk[i]; };
  auto VS = [&](int i) { return K > 0 ? vs[i] : t_old * dd[i]; };
  for (int r = wave; r < 2 * m; r += LB_WAVES) {
    const bool isY = r >= m;
    const int j = isY ? r - m : r;
    const float* row = (isY ? Y : S) + (size_t)j * NP;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = lane; i < NP; i += 64) {
      const float v = row[i], g = VG(i), y = g - VK(i);
      a0 += (double)v * (double)g;
      a1 += (double)v * (double)y;
      if (isY) a2 += (double)v * (double)VS(i);
    }
    a0 = lb_wave_sum(a0);
    a1 = lb_wave_sum(a1);
    if (isY) a2 = lb_wave_sum(a2);
    if (lane == 0) {
      s_dot[(isY ? 1 : 0) * m + j] = a0;
      s_dot[(isY ? 3 : 2) * m + j] = a1;
      if (isY) s_dot[4 * m + j] = a2;
    }
  }
  for (int q = LB_WAVES - 1 - wave; q < LB_EXTRA; q += LB_WAVES) {
    double acc = 0.0;
    for (int i = lane; i < NP; i += 64) {
      const float g = VG(i), gp = VK(i), sv = VS(i), y = g - gp;
      const float u = q == E_YS ? y : q == E_YY ? y : q == E_GG ? g : q == E_G1 ? fabsf(g) : q == E_NF ? (isfinite(g) ? 0.f : 1.f)
                      : q == E_KK ? gp : q == E_K1 ? fabsf(gp) : q == E_SG ? sv : y;
      const float w = q == E_YS ? sv : q == E_YY ? y : q == E_GG ? g : q == E_KK ? gp : (q == E_SG || q == E_YG) ? g : 1.f;
      acc += (double)u * (double)w;
    }
    acc = lb_wave_sum(acc);
    if (lane == 0) s_dot[5 * m + q] = acc;
  }
  __syncthreads();
  const double* ex = s_dot + 5 * m;
  const double ys_d = ex[E_YS], yy_d = ex[E_YY];
  const float ys = (float)ys_d, gg = (float)ex[E_GG], g1 = (float)ex[E_G1];

  // ---- the decision, the same in every thread
  const float f = hp.w_res * l_r + hp.w_bc * l_bc + hp.w_ic * l_ic;
  const bool finite = isfinite(f) && ex[E_NF] == 0.0;
  int act;
  if (rec.stalled) act = A_STALL;
  else if (rec.phase == 0) act = A_FIRST;
  else if (hp.line_search == 0) act = A_STEP;
  else if (finite && f <= rec.f0 + hp.c1 * t_old * rec.gtd0) act = A_STEP;
  else if (rec.ls_trials + 1 >= hp.max_ls) act = (rec.sd_failed && rec.n_pairs == 0) ? A_STALL : A_RESET;
  else act = A_REJECT;

  QcLbfgsRec o = rec;
  o.n_eval = rec.n_eval + 1;
  o.f = f;
  o.loss_parts[0] = l_r;
  o.loss_parts[1] = l_bc;
  o.loss_parts[2] = l_ic;
  o.accepted = (act == A_FIRST || act == A_STEP) ? 1 : 0;
  float t_new = t_old;
  bool reset_sd = false;   // A_STEP only: the new direction is no descent direction

  if (act == A_FIRST) {
    o.phase = 1;
    o.n_iter = rec.n_iter + 1;
    o.ls_trials = 0;
    o.sd_failed = 0;
    o.f0 = f;
    o.gtd0 = -gg;
    t_new = lb_first_t(hp.lr, g1);
    lb_each<K>(NP, tid, [&](int i, int k) {
      const float g = G(i, k), p = P(i, k), pn = p + t_new * (-g);
      xk[i] = p;
      gk[i] = g;
      dd[i] = -g;
      a.prm[i] = pn;
      if (K > 0) pv[k] = pn;
    });
  } else if (act == A_STEP) {
    const bool push = ys > hp.curv_eps;
    const int h = rec.head;
    const int np = push ? min(rec.n_pairs + 1, m) : rec.n_pairs;
    const int head = push ? (h + 1 == m ? 0 : h + 1) : h;
    const float gamma = push ? (float)(ys_d / yy_d) : rec.gamma;
    const bool sd = hp.line_search != 0 && np == 0;   // backtracking mode with an empty history: steepest descent
    if (wave == 0) {
      // the recursion on the scalars, lane j holding alpha_j and beta_j of pair j (oldest first): every inner sum is one
      // wave sum.  Gram entries by slot, the new pair's row and column taken from this call's batch
      auto sy = [&](int si, int sj) -> double {
        if (push && si == h) return sj == h ? ys_d : s_dot[4 * m + sj];
        if (push && sj == h) return s_dot[2 * m + si];
        return s_SY[si * m + sj];
      };
      auto yyf = [&](int si, int sj) -> double {
        if (push && (si == h || sj == h)) return (si == h && sj == h) ? yy_d : s_dot[3 * m + (si == h ? sj : si)];
        return s_YY[si * m + sj];
      };
      auto sg = [&](int sl) -> double { return (push && sl == h) ? ex[E_SG] : s_dot[sl]; };
      auto yg = [&](int sl) -> double { return (push && sl == h) ? ex[E_YG] : s_dot[m + sl]; };
      auto slot = [&](int k) { return (head - np + k + m) % m; };   // k = 0: the oldest pair
      const int j = lane;
      const bool live = j < np;
      const int sj = live ? slot(j) : 0;
      const double gam = (double)gamma;
      double al = 0.0, be = 0.0;
      for (int i = np - 1; i >= 0; --i) {
        const int si = slot(i);
        const double tot = lb_wave_sum((live && j > i) ? al * sy(si, sj) : 0.0);
        const double a_i = (sg(si) - tot) / sy(si, si);
        if (j == i) al = a_i;
      }
      for (int i = 0; i < np; ++i) {
        const int yi = slot(i);
        double term = 0.0;
        if (live) term = -gam * al * yyf(yi, sj) + (j < i ? (al - be) * sy(sj, yi) : 0.0);
        const double b_i = (gam * yg(yi) + lb_wave_sum(term)) / sy(yi, yi);
        if (j == i) be = b_i;
      }
      if (lane < m) s_cS[lane] = s_cY[lane] = 0.0;
      if (live) {
        s_cS[sj] = be - al;
        s_cY[sj] = gam * al;
      }
    }
    __syncthreads();
    const float cg = sd ? -1.f : -gamma;
    // new pair into its slot, x_k / g_k, the direction d = cg g + sum over the kept pairs (oldest first), and g.d
    double gd = 0.0;
    float dn[KC];
    lb_each<K>(NP, tid, [&](int i, int k) {
      const float g = G(i, k), p = P(i, k);
      if (push) {
        S[(size_t)h * NP + i] = t_old * D(i, k);
        Y[(size_t)h * NP + i] = g - GK(i, k);
      }
      double acc = (double)cg * (double)g;
      for (int q = 0; q < np; ++q) {
        const int j = (head - np + q + m) % m;
        acc += s_cS[j] * (double)S[(size_t)j * NP + i] + s_cY[j] * (double)Y[(size_t)j * NP + i];
      }
      const float d = (float)acc;
      xk[i] = p;
      gk[i] = g;
      dd[i] = d;
      if (K > 0) dn[k] = d;
      gd += (double)g * (double)d;
    });
    const float gtd = (float)lb_block_sum(gd, s_red);
    o.n_iter = rec.n_iter + 1;
    o.n_pairs = np;
    o.head = head;
    o.gamma = gamma;
    o.ls_trials = 0;
    o.sd_failed = 0;
    o.f0 = f;
    if (!push) o.n_skipped_pairs = rec.n_skipped_pairs + 1;
    bool move = true;
    if (hp.line_search == 0) {
      t_new = hp.lr;
      o.gtd0 = gtd;
      move = gtd < 0.f;
    } else if (sd) {
      t_new = lb_first_t(hp.lr, g1);
      o.gtd0 = -gg;
    } else if (!(gtd < 0.f)) {
      reset_sd = true;
      o.n_pairs = 0;
      o.head = 0;
      o.n_resets = rec.n_resets + 1;
      t_new = lb_first_t(hp.lr, g1);
      o.gtd0 = -gg;
    } else {
      t_new = hp.lr;
      o.gtd0 = gtd;
    }
    lb_each<K>(NP, tid, [&](int i, int k) {
      const float p = P(i, k);
      float d = K > 0 ? dn[k] : dd[i];
      if (reset_sd) {
        d = -G(i, k);
        dd[i] = d;
      }
      const float pn = move ? p + t_new * d : p;
      a.prm[i] = pn;
      if (K > 0) pv[k] = pn;
    });
    if (!move) t_new = 0.f;   // (kept below as the t that led to the next point; the record's t stays lr)
    if (push && tid < m) {
      const int j = tid;
      auto put = [](float* G2, int at, double v) {      // entry `at` as a (high, low) float pair
        const float hi = (float)v;
        G2[2 * at] = hi;
        G2[2 * at + 1] = (float)(v - (double)hi);
      };
      if (j == h) {
        put(SY, h * m + h, ys_d);
        put(YY, h * m + h, yy_d);
        rho[h] = 1.f / ys;
      } else {
        put(SY, h * m + j, s_dot[4 * m + j]);
        put(SY, j * m + h, s_dot[2 * m + j]);
        put(YY, h * m + j, s_dot[3 * m + j]);
        put(YY, j * m + h, s_dot[3 * m + j]);
      }
    }
  } else if (act == A_REJECT) {
    o.n_rejected = rec.n_rejected + 1;
    o.ls_trials = rec.ls_trials + 1;
    float tq = -rec.gtd0 * t_old * t_old / (2.f * (f - rec.f0 - rec.gtd0 * t_old));
    if (!isfinite(f) || !isfinite(tq)) tq = hp.shrink_hi * t_old;
    t_new = fminf(fmaxf(tq, hp.shrink_lo * t_old), hp.shrink_hi * t_old);
    lb_each<K>(NP, tid, [&](int i, int k) {
      const float pn = X(i, k) + t_new * D(i, k);
      a.prm[i] = pn;
      if (K > 0) pv[k] = pn;
    });
  } else if (act == A_RESET) {
    o.n_rejected = rec.n_rejected + 1;
    o.n_resets = rec.n_resets + 1;
    o.ls_trials = 0;
    o.sd_failed = 1;
    o.n_pairs = 0;
    o.head = 0;
    o.gtd0 = -(float)ex[E_KK];
    t_new = lb_first_t(hp.lr, (float)ex[E_K1]);
    lb_each<K>(NP, tid, [&](int i, int k) {
      const float d = -GK(i, k), pn = X(i, k) + t_new * d;
      dd[i] = d;
      a.prm[i] = pn;
      if (K > 0) pv[k] = pn;
    });
  } else {   // stalled: back to (or staying at) the last accepted point
    if (!rec.stalled) o.n_rejected = rec.n_rejected + 1;
    o.stalled = 1;
    t_new = 0.f;
    lb_each<K>(NP, tid, [&](int i, int k) {
      const float pn = X(i, k);
      a.prm[i] = pn;
      if (K > 0) pv[k] = pn;
    });
  }

  // ---- trig and diagonal-run tables from the new theta, as the Adam tail does (register path: theta reaches the table
  // through LDS, in the space of the row sweeps' vectors; strided path: through the parameters)
  if (a.prog != nullptr) {
    const int n_theta = NP - a.theta_off;
    if constexpr (K > 0) {
      __syncthreads();
      lb_each<K>(NP, tid, [&](int i, int k) {
        if (i >= a.theta_off) s_v[i - a.theta_off] = pv[k];
      });
    }
    __syncthreads();
    qc_gate_stage_tables<LB_T>(sg, a.prog, a.n_gates, a.n_qubits, n_theta, a.trig, a.runs, K > 0 ? s_v : a.prm + a.theta_off, tid);
  }
  if (tid == 0) {
    const int e = rec.n_eval;
    if (a.hist != nullptr && e >= 0 && e < a.hist_cap) {
      a.hist[3 * e] = f;
      a.hist[3 * e + 1] = rec.t_led;
      a.hist[3 * e + 2] = (float)o.accepted;
    }
    o.t_led = t_new;
    o.t = (act == A_STEP && hp.line_search == 0) ? hp.lr : t_new;
    if (act == A_STALL) o.t = t_old;
    o.NP = NP;
    o.history = m;
    *reinterpret_cast<QcLbfgsRec*>(a.ws) = o;
  }
}

__global__ void __launch_bounds__(256) k_lbfgs_init(float* ws, size_t words, int NP, int m) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
    float v = 0.f;
    if (i == offsetof(QcLbfgsRec, gamma) / 4) v = 1.f;
    if (i == offsetof(QcLbfgsRec, NP) / 4) v = __int_as_float(NP);
    if (i == offsetof(QcLbfgsRec, history) / 4) v = __int_as_float(m);
    ws[i] = v;
  }
}

__global__ void k_lbfgs_restart(QcLbfgsRec* r, int keep) {
  if (threadIdx.x != 0) return;
  QcLbfgsRec o = *r;
  o.phase = 0;
  o.ls_trials = 0;
  o.stalled = 0;
  o.sd_failed = 0;
  o.t_led = 0.f;
  if (!keep) {
    o.n_pairs = 0;
    o.head = 0;
    o.gamma = 1.f;
  }
  *r = o;
}

}  // namespace

size_t qc_lbfgs_words(int NP, int m) {
  return (size_t)QC_LBFGS_REC_WORDS + 3 * (size_t)NP + 2 * (size_t)m * NP + (size_t)m + 4 * (size_t)m * m;
}

int qc_lbfgs_init_launch(void* ws, int NP, int m, hipStream_t st) {
  const size_t words = qc_lbfgs_words(NP, m);
  const int blocks = (int)(words / 256 + 1 < 1024 ? words / 256 + 1 : 1024);
  hipLaunchKernelGGL(k_lbfgs_init, dim3(blocks), dim3(256), 0, st, (float*)ws, words, NP, m);
  return QC_OK;
}

int qc_lbfgs_restart_launch(void* ws, int keep, hipStream_t st) {
  hipLaunchKernelGGL(k_lbfgs_restart, dim3(1), dim3(64), 0, st, (QcLbfgsRec*)ws, keep);
  return QC_OK;
}

int qc_lbfgs_step_launch(const float* flat, int NP, float* prm, void* ws, QcLbfgsHyper hp, float* hist, int hist_cap,
                         const qc_program* pg, int theta_off, QcTrig* trig, hipStream_t st) {
  QcLbfgsArgs a;
  a.flat = flat; a.NP = NP; a.prm = prm; a.ws = (float*)ws; a.hp = hp; a.hist = hist; a.hist_cap = hist_cap;
  a.prog = pg ? pg->d_gates : nullptr; a.n_gates = pg ? pg->n_gates : 0; a.theta_off = theta_off; a.trig = trig;
  a.n_qubits = pg ? pg->n_qubits : 0;
  a.runs = qc_diag_runs_of(pg);
  const size_t lds = sizeof(float) * qc_gate_stage_words(pg);
  if (NP + 3 <= 3 * LB_T)
    hipLaunchKernelGGL((k_lbfgs<3>), dim3(1), dim3(LB_T), lds, st, a);
  else
    hipLaunchKernelGGL((k_lbfgs<0>), dim3(1), dim3(LB_T), lds, st, a);
  return QC_OK;
}
