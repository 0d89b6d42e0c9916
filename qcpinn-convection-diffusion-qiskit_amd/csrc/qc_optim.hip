// Gradient-row reduction, gradient clipping, Adam and the plateau scheduler, all on device so a
// training step never synchronises with the host.
//
// Mirrors the optimiser block of the reference step (trainer/diffusion_train.py:81-90):
//   clip_grad_norm_(max_norm=1) -> Adam(lr) -> ReduceLROnPlateau(min, factor 0.9, patience 1000)
// as configured in nn/DVPDESolver.py:59-64 (torch defaults otherwise: betas (0.9, 0.999),
// eps 1e-8, threshold 1e-4 relative, cooldown 0, min_lr 0, scheduler eps 1e-8).
#include "qc_internal.h"

namespace {

// Fixed-order column sums of the partial-row matrix: out[c] = sum_r part[r][c].
// grid.x = ceil(ncols/64); 16 waves per block, wave w takes rows w, w+16, ...
__global__ void __launch_bounds__(1024) k_reduce_rows(const float* __restrict__ part, int64_t rows,
                                                      int64_t stride, int ncols, float* __restrict__ out) {
  __shared__ float s[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (col < ncols) {
    int64_t r = wave;
    for (; r + 48 < rows; r += 64) {
      a0 += part[r * stride + col];
      a1 += part[(r + 16) * stride + col];
      a2 += part[(r + 32) * stride + col];
      a3 += part[(r + 48) * stride + col];
    }
    for (; r < rows; r += 16) a0 += part[r * stride + col];
  }
  s[wave][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (wave == 0 && col < ncols) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += s[w][lane];
    out[col] = t;
  }
}

// beta^step by repeated squaring in double (<= 31 dependent multiplies; the generic pow() costs ~1 us of a one-block
// kernel's latency chain); agrees with pow() to a few ulp of double, far below the float it is converted to
__device__ __forceinline__ double qc_ipow(double b, int e) {
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

__device__ __forceinline__ float block_sum_1024(float v, float* s_red) {
  v = qc_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_red[w];
  return t;
}

// the same sum where the block is known to be 16 waves (k_adam_fast): the wave count is not fetched from the dispatch
// packet behind the second barrier
__device__ __forceinline__ float block_sum_16_waves(float v, float* s_red) {
  v = qc_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) t += s_red[w];
  return t;
}

// One block.  flat = [grad[NP] | L_r, L_bc, L_ic].  Updates prm/m/v in place, advances the
// scheduler, appends the loss to hist[step], and rebuilds the gate trig table from the NEW theta.
struct QcAdamArgs {
  float* flat;
  int NP;
  float *prm, *m, *v;
  QcOptState* st;
  QcOptHyper hp;
  float* hist;
  int hist_cap;
  const QcGate* prog;
  int n_gates, theta_off, n_qubits;
  QcTrig* trig;
  QcDiagRuns runs;
};

// The balancer's share of an optimiser launch (BAL below), on the thread that owns entry NP_B - 3 + k, from the entry's
// value p BEFORE the update and the reduced loss column Lk: the effective weight w_k e_k (stored to row `hi` of the weight
// history), the term w_k e_k L_k + s_k of F (to s_term[k], read by thread 0 behind the next barrier), and the gradient
// entry scale_k (1 - w_k e_k L_k), exactly 0 for a frozen term.
__device__ __forceinline__ float bal_entry(const int k, const float p, const float Lk, const QcOptHyper& hp, const QcBal& bl,
                                           const int hi, float* s_term) {
  const float sc = k == 0 ? bl.scale[0] : (k == 1 ? bl.scale[1] : bl.scale[2]);
  const float w = (k == 0 ? hp.w_res : (k == 1 ? hp.w_bc : hp.w_ic)) * qc_bal_factor(sc, p);
  if (bl.hist != nullptr && hi >= 0 && hi < bl.hist_cap) bl.hist[(int64_t)hi * QC_BAL_N + k] = w;
  s_term[k] = fmaf(w, Lk, sc * p);
  return sc == 0.f ? 0.f : sc * (1.f - w * Lk);
}

// BAL (the balanced step): the last QC_BAL_N of the NP entries are the balancer's.  Their gradients are formed here
// (bal_entry) whatever flat holds in their slots, they stay out of the clip's norm and are not scaled by its factor, and
// the scheduler, the history and last_loss see F; loss_parts stay the raw columns.
template <bool BAL = false>
__device__ __forceinline__ void adam_block(const QcAdamArgs& a, float* s_red, const QcBal* bl = nullptr,
                                           float* s_term = nullptr) {
  float* __restrict__ flat = a.flat;
  const int NP = a.NP;
  const int NPn = BAL ? NP - QC_BAL_N : NP;   // the clipped (network) entries
  float *__restrict__ prm = a.prm, *__restrict__ m = a.m, *__restrict__ v = a.v;
  QcOptState* __restrict__ st = a.st;
  const QcOptHyper& hp = a.hp;
  float* __restrict__ hist = a.hist;
  const int hist_cap = a.hist_cap, n_gates = a.n_gates, theta_off = a.theta_off;
  const QcGate* __restrict__ prog = a.prog;
  QcTrig* __restrict__ trig = a.trig;
  float ss = 0.f;
  for (int i = threadIdx.x; i < NPn; i += blockDim.x) ss += flat[i] * flat[i];
  const float norm = sqrtf(block_sum_1024(ss, s_red));
  float coef = hp.max_norm / (norm + 1e-6f);           // torch.nn.utils.clip_grad_norm_
  coef = coef > 1.f ? 1.f : coef;

  const int step = st->step + 1;
  const float lr = st->lr;
  const float b1 = (float)hp.beta1, b2 = (float)hp.beta2;
  const double bc1 = 1.0 - qc_ipow(hp.beta1, step);
  const float bc2s = (float)sqrt(1.0 - qc_ipow(hp.beta2, step));
  const float step_size = (float)((double)lr / bc1);
  for (int i = threadIdx.x; i < NP; i += blockDim.x) {
    float g = flat[i] * coef;
    if constexpr (BAL)
      if (i >= NPn) g = bal_entry(i - NPn, prm[i], flat[NP + i - NPn], hp, *bl, step - 1 - st->hist_base, s_term);
    flat[i] = g;                                       // leave the clipped gradient visible
    const float mi = m[i] + (1.f - b1) * (g - m[i]);       // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = b2 * v[i] + (1.f - b2) * g * g;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2s + hp.eps;
    prm[i] -= step_size * (mi / denom);
  }
  __syncthreads();
  if (prog != nullptr) {
    for (int g = threadIdx.x; g < n_gates; g += blockDim.x) {
      const QcGate gt = prog[g];
      QcTrig tr = {1.f, 0.f, 0.f, 0.f};
      if (gt.op != QC_U4 && gt.slot >= 0) {
        tr.th = prm[theta_off + gt.slot];
        sincosf(0.5f * tr.th, &tr.s, &tr.c);
      }
      trig[g] = tr;
    }
    __syncthreads();
    qc_fill_diag_tables(prog, n_gates, a.n_qubits, trig, threadIdx.x, a.runs);
  }
  if (threadIdx.x == 0) {
    const float lr_ = flat[NP], lb = flat[NP + 1], li = flat[NP + 2];
    float loss = hp.w_res * lr_ + hp.w_bc * lb + hp.w_ic * li;
    if constexpr (BAL) loss = (s_term[0] + s_term[1]) + s_term[2];
    // ReduceLROnPlateau.step(loss), mode "min", threshold_mode "rel", cooldown 0
    float best = st->best;
    int bad = st->num_bad;
    float new_lr = lr;
    if (loss < best * (1.f - hp.sched_threshold)) {
      best = loss;
      bad = 0;
    } else {
      bad += 1;
    }
    if (bad > hp.sched_patience) {
      const float cand = fmaxf(lr * hp.sched_factor, hp.sched_min_lr);
      if (lr - cand > hp.sched_eps) new_lr = cand;
      bad = 0;
    }
    st->lr = new_lr;
    st->best = best;
    st->num_bad = bad;
    st->step = step;
    st->last_loss = loss;
    st->last_norm = norm;
    st->loss_parts[0] = lr_;
    st->loss_parts[1] = lb;
    st->loss_parts[2] = li;
    const int hi = step - 1 - st->hist_base;
    if (hist != nullptr && hi >= 0 && hi < hist_cap) hist[hi] = loss;
  }
}

__global__ void __launch_bounds__(1024) k_adam(QcAdamArgs a) {
  __shared__ float s_red[16];
  adam_block(a, s_red);
}

// First level of the step's own row reduction, in place: block (cb, rs) folds rows rs, rs + RS,
// rs + 2 RS, ... of column block cb into row rs (only that block ever touches row rs of those columns).
// The RS = gridDim.y surviving rows are added, in order, by k_adam_fold (same call) or k_reduce_rows.
// 1 700 rows become ~7 dependent loads per wave on 384 blocks instead of ~27 on 12.
// CW = (QcCausalRows) (the causal step): residual row r < rows_res is scaled by the weight of its slab, W[(r + tile_off) mod M],
// as it is loaded; value rows are not scaled; the order of the sums is the plain fold's.  (A trailing pack, as k_adam_fast
// takes its balancer: the plain instantiation carries no argument for it and keeps its code.)
struct QcCausalRows {
  const float* W;   // [M], written by k_causal_weights ahead of this launch
  int rows_res, M, tile_off;
};
__device__ __forceinline__ float qc_causal_w(const int64_t r, const QcCausalRows& c) {
  return r < c.rows_res ? c.W[(uint32_t)((int)r + c.tile_off) % (uint32_t)c.M] : 1.f;
}
// CW = (QcClassRows) (the gradient-norm step): three folds in one launch, the class in blockIdx.z.  Class c owns rows
// [lo_c, lo_c + n_c); block (cb, rs, c) folds rows lo_c + rs, lo_c + rs + RS_c, ... into row lo_c + rs, RS_c = min(n_c, 32),
// exactly as the plain fold would fold the class's rows alone; blocks with rs >= RS_c (an empty class: all of them) return.
struct QcClassRows {
  int lo_ic, lo_bc;          // first row of the IC and of the BC class (the residual class starts at row 0)
  int n_res, n_ic, n_bc;
};
constexpr int QC_RED_WAVES = 8;
template <class... CW>
__global__ void __launch_bounds__(64 * QC_RED_WAVES) k_fold_rows(float* __restrict__ part, int64_t rows, int64_t stride,
                                                                 int ncols, CW... cw) {
  static_assert(sizeof...(CW) == 0 ||
                    (sizeof...(CW) == 1 && ((std::is_same_v<CW, QcCausalRows> || std::is_same_v<CW, QcClassRows>) && ...)),
                "(), (QcCausalRows) or (QcClassRows)");
  constexpr bool CAUSAL = (std::is_same_v<CW, QcCausalRows> || ...);
  constexpr bool CLASSES = (std::is_same_v<CW, QcClassRows> || ...);
  __shared__ float s[QC_RED_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const int rs = blockIdx.y;
  int RS = gridDim.y;
  if constexpr (CLASSES) {
    const QcClassRows& c = std::get<0>(std::tie(cw...));
    const int z = blockIdx.z;
    const int lo = z == 0 ? 0 : (z == 1 ? c.lo_ic : c.lo_bc), n = z == 0 ? c.n_res : (z == 1 ? c.n_ic : c.n_bc);
    RS = n < 32 ? n : 32;
    if (rs >= RS) return;   // (the whole block: nobody waits at the barrier below)
    part += (int64_t)lo * stride;
    rows = n;
  }
  // rows r, r + hop, r + 2 hop, ... of this wave: the first EIGHT are requested together (config 2 has ~7 per wave: one
  // memory round trip instead of four dependent ones), then summed in the same fixed order as a two-chain loop
  float a0 = 0.f, a1 = 0.f;
  if (col < ncols) {
    const int64_t r0 = rs + (int64_t)RS * wave;
    const int64_t hop = (int64_t)RS * QC_RED_WAVES;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t r = r0 + k * hop;
      v[k] = r < rows ? part[r * stride + col] : 0.f;
      if constexpr (CAUSAL) v[k] *= qc_causal_w(r, cw...);
    }
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      a0 += v[k];
      a1 += v[k + 1];
    }
    for (int64_t r = r0 + 8 * hop; r < rows; r += 2 * hop) {
      if constexpr (CAUSAL) {
        a0 += part[r * stride + col] * qc_causal_w(r, cw...);
        if (r + hop < rows) a1 += part[(r + hop) * stride + col] * qc_causal_w(r + hop, cw...);
      } else {
        a0 += part[r * stride + col];
        if (r + hop < rows) a1 += part[(r + hop) * stride + col];
      }
    }
  }
  s[wave][lane] = a0 + a1;
  __syncthreads();
  if (wave == 0 && col < ncols) {
    float t = s[0][lane];
#pragma unroll
    for (int w = 1; w < QC_RED_WAVES; ++w) t += s[w][lane];
    part[(int64_t)rs * stride + col] = t;
  }
}
// implicit instantiations are emitted in order of first use: the plain fold is named here so that it keeps its place in the
// code object, ahead of the optimiser kernels
constexpr auto k_fold_rows_plain = k_fold_rows<>;

// The optimiser update with everything it reads fetched in ONE round trip (state record, gradient or the
// RS folded rows of it, moments, parameters, and the gate records and run list the tables need: qc_common.h), for
// NP + 3 <= 3 * 1024: a single-block kernel is a chain of memory latencies, so the loads are issued together up front
// and the new theta reaches the trig table through LDS instead of a store -> load of global memory.  What depends on
// the state record alone (the bias corrections) is computed under those loads' latency, and the record is written by a
// thread of the last wave as soon as the loss is known; behind the update nothing is loaded from global memory and no
// store is waited for.  Arithmetic identical to adam_block.
// FOLD: flat[c] = part[0][c] + ... + part[RS-1][c] (second reduction level, fixed order) is formed here.
// BL = (QcBal): BAL as in adam_block; the owner of a balancer entry holds its value in a register and finds the loss
// columns in LDS.  (A trailing pack, as the post kernels take their target kinds: the plain instantiations carry no
// argument for it.)
constexpr int QC_ADAM_K = 3;
template <bool FOLD, class... BL>
__global__ void __launch_bounds__(1024) k_adam_fast(QcAdamArgs a, const float* __restrict__ part, int64_t stride, int RS,
                                                    BL... bl) {
  static_assert(sizeof...(BL) == 0 || (sizeof...(BL) == 1 && (std::is_same_v<BL, QcBal> && ...)), "() or (QcBal)");
  constexpr bool BAL = sizeof...(BL) == 1;
  __shared__ float s_red[16];
  __shared__ float s_loss[BAL ? 3 + QC_BAL_N : 3];   // BAL: the terms of F behind the loss columns
  [[maybe_unused]] float* s_term = s_loss + 3;
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];   // the gate stage (qc_common.h), then theta [n_theta]
  const int NP = a.NP, tid = threadIdx.x;
  const int NPn = BAL ? NP - QC_BAL_N : NP;   // the clipped (network) entries
  const QcOptHyper& hp = a.hp;
  const int step = a.st->step + 1;
  const float lr = a.st->lr;
  float best = a.st->best;
  int bad = a.st->num_bad;
  const int hist_base = a.st->hist_base;
  // every argument the requests below need, fetched from the argument segment in one round trip (left alone the compiler
  // fetches each where it is first used: five dependent scalar waits ahead of the last request).  Behind the reads of
  // the record: a uniform load that follows an asm statement is no longer a scalar load
  asm volatile("" ::"s"(a.NP), "s"(a.m), "s"(a.v), "s"(a.prm), "s"(a.flat), "s"(a.prog), "s"(a.n_gates), "s"(a.n_qubits),
               "s"(a.runs.n), "s"(a.runs.list), "s"(part), "s"(stride), "s"(RS));
  const int n_theta = NPn - a.theta_off;
  const QcGateStage sg = qc_gate_stage_load(a.prog, a.n_gates, a.n_qubits, a.runs, s_dyn, tid);
  float* s_theta = s_dyn + sg.words;
  float g[QC_ADAM_K], mi[QC_ADAM_K], vi[QC_ADAM_K], pi[QC_ADAM_K];
  [[maybe_unused]] float x[QC_ADAM_K][32];   // FOLD: the (<= 32) folded rows of each column block
  // all (<= 32) folded rows of every live column block requested together, unconditionally: one memory round trip.
  // RS < 32: the rows past RS - 1 load row RS - 1 again and are replaced by +0.f below
  const bool full = RS >= 32;
  auto request = [&](const int k) {
    const int i = tid + k * 1024;
    g[k] = mi[k] = vi[k] = pi[k] = 0.f;
    if (i < NP) {
      mi[k] = a.m[i];
      vi[k] = a.v[i];
      pi[k] = a.prm[i];
    }
    if (i < NP + 3) {
      if constexpr (FOLD) {
        // (the row pointer walks in scalar registers, pinned there and read as the global pointer it is: one lane offset
        // serves all 32 loads, where 32 per-lane 64-bit addresses did not fit beside the values in flight)
        const float* row = part;
        if (full) {
#pragma unroll
          for (int j = 0; j < 32; ++j) {
            x[k][j] = ((const __attribute__((address_space(1))) float*)row)[i];
            if (j < 31) row += stride;
            asm volatile("" : "+s"(row));
          }
        } else if (RS > 0) {
#pragma unroll
          for (int j = 0; j < 32; ++j) {
            x[k][j] = ((const __attribute__((address_space(1))) float*)row)[i];
            if (j + 1 < RS) row += stride;
            asm volatile("" : "+s"(row));
          }
        }
      } else {
        g[k] = a.flat[i];
      }
    }
  };
  request(0);
  request(1);
  // under the latency of those loads: what needs the state record alone (pinned: sunk behind the norm's barriers otherwise)
  const float b1 = (float)hp.beta1, b2 = (float)hp.beta2;
  const double bc1 = 1.0 - qc_ipow(hp.beta1, step);
  float bc2s = (float)sqrt(1.0 - qc_ipow(hp.beta2, step));
  float step_size = (float)((double)lr / bc1);
  asm volatile("" : "+v"(bc2s), "+v"(step_size));
  // the third column block (NP + 3 > 2048) behind that arithmetic, still ahead of the first wait: 96 rows in flight
  // beside the double-precision temporaries are more than the 128 registers of a 1024-thread block
  request(2);
  if constexpr (FOLD) {
#pragma unroll
    for (int k = 0; k < QC_ADAM_K; ++k) {
      const int i = tid + k * 1024;
      if (i < NP + 3) {
        float t = 0.f;
        if (full) {
#pragma unroll
          for (int j = 0; j < 32; ++j) t += x[k][j];      // the same left-to-right sum
        } else if (RS > 0) {
#pragma unroll
          for (int j = 0; j < 32; ++j) t += j < RS ? x[k][j] : 0.f;   // (rows >= RS add +0.f: the sum is unchanged)
        }
        for (int q = 32; q < RS; ++q) t += part[(int64_t)q * stride + i];
        g[k] = t;
      }
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < QC_ADAM_K; ++k) {
    const int i = tid + k * 1024;
    if (i < NPn) ss += g[k] * g[k];
    else if ((!BAL || i >= NP) && i < NP + 3) s_loss[i - NP] = g[k];
  }
  qc_gate_stage_store<1024>(sg, a.prog, a.n_gates, a.runs, tid);
  const float norm = sqrtf(block_sum_16_waves(ss, s_red));   // (its barriers also publish s_loss and the gate stage)
  float coef = hp.max_norm / (norm + 1e-6f);
  coef = coef > 1.f ? 1.f : coef;
  // the scheduler, the state record and the history entry: one thread of the last wave (the first waves have the gates),
  // as soon as the loss is known.  (Every thread's reads of the record lie ahead of the norm's barriers.)
  auto write_state = [&]() {
    const float lr_ = s_loss[0], lb = s_loss[1], li = s_loss[2];
    float loss = hp.w_res * lr_ + hp.w_bc * lb + hp.w_ic * li;
    if constexpr (BAL) loss = (s_term[0] + s_term[1]) + s_term[2];
    float new_lr = lr;
    if (loss < best * (1.f - hp.sched_threshold)) {
      best = loss;
      bad = 0;
    } else {
      bad += 1;
    }
    if (bad > hp.sched_patience) {
      const float cand = fmaxf(lr * hp.sched_factor, hp.sched_min_lr);
      if (lr - cand > hp.sched_eps) new_lr = cand;
      bad = 0;
    }
    QcOptState o;
    o.lr = new_lr;
    o.best = best;
    o.num_bad = bad;
    o.step = step;
    o.last_loss = loss;
    o.last_norm = norm;
    o.loss_parts[0] = lr_;
    o.loss_parts[1] = lb;
    o.loss_parts[2] = li;
    o.hist_base = hist_base;
#pragma unroll
    for (int k = 0; k < 6; ++k) o.pad[k] = 0;
    *a.st = o;
    const int hi = step - 1 - hist_base;
    if (a.hist != nullptr && hi >= 0 && hi < a.hist_cap) a.hist[hi] = loss;
  };
  if constexpr (!BAL)
    if (tid == 1023) write_state();
#pragma unroll
  for (int k = 0; k < QC_ADAM_K; ++k) {
    const int i = tid + k * 1024;
    if (i < NP) {
      float gc = g[k] * coef;
      if constexpr (BAL)
        if (i >= NPn) gc = bal_entry(i - NPn, pi[k], s_loss[i - NPn], hp, bl..., step - 1 - hist_base, s_term);
      const float mn = mi[k] + (1.f - b1) * (gc - mi[k]);
      const float vn = b2 * vi[k] + (1.f - b2) * gc * gc;
      const float denom = sqrtf(vn) / bc2s + hp.eps;
      const float pn = pi[k] - step_size * (mn / denom);
      a.flat[i] = gc;
      a.m[i] = mn;
      a.v[i] = vn;
      a.prm[i] = pn;
      if (a.prog != nullptr && i >= a.theta_off && (!BAL || i < NPn)) s_theta[i - a.theta_off] = pn;
    } else if (FOLD && i < NP + 3) {
      a.flat[i] = g[k];
    }
  }
  if (a.prog == nullptr && !BAL) return;
  qc_lds_barrier();   // theta (and BAL: the terms of F) through LDS
  if constexpr (BAL)
    if (tid == 1023) write_state();
  if (a.prog != nullptr) qc_gate_stage_tables<1024>(sg, a.prog, a.n_gates, a.n_qubits, n_theta, a.trig, a.runs, s_theta, tid);
}

// one block: per-gate (cos, sin, theta) entries, then the phase tables of the fused diagonal runs
__global__ void __launch_bounds__(256) k_prep_trig(const QcGate* __restrict__ prog, int n_gates, int n_qubits,
                                                   const float* __restrict__ theta, QcTrig* __restrict__ trig,
                                                   QcDiagRuns runs) {
  for (int g = threadIdx.x; g < n_gates; g += 256) {
    const QcGate gt = prog[g];
    QcTrig tr = {1.f, 0.f, 0.f, 0.f};
    if (gt.op != QC_U4 && gt.slot >= 0) {
      tr.th = theta[gt.slot];
      sincosf(0.5f * tr.th, &tr.s, &tr.c);
    }
    trig[g] = tr;
  }
  __syncthreads();
  qc_fill_diag_tables(prog, n_gates, n_qubits, trig, threadIdx.x, runs);
}

}  // namespace

int qc_opt_reduce_rows(const float* part, int64_t rows, int64_t stride, int ncols, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_reduce_rows, dim3(qc_ceil_div(ncols, 64)), dim3(1024), 0, st, part, rows, stride, ncols, out);
  return QC_OK;
}

static QcAdamArgs adam_args(float* flat, int NP, float* prm, float* m, float* v, QcOptState* state, QcOptHyper hp,
                            float* hist, int hist_cap, const qc_program* pg, int theta_off, QcTrig* trig) {
  QcAdamArgs a;
  a.flat = flat; a.NP = NP; a.prm = prm; a.m = m; a.v = v; a.st = state; a.hp = hp; a.hist = hist; a.hist_cap = hist_cap;
  a.prog = pg ? pg->d_gates : nullptr; a.n_gates = pg ? pg->n_gates : 0; a.theta_off = theta_off; a.trig = trig;
  a.n_qubits = pg ? pg->n_qubits : 0;
  a.runs = qc_diag_runs_of(pg);
  return a;
}

static bool adam_fast_ok(int NP) { return NP + 3 <= QC_ADAM_K * 1024; }
// dynamic LDS of a k_adam_fast launch: the gate stage, then theta
static size_t adam_fast_lds(const qc_program* pg, int NP, int theta_off) {
  return pg ? sizeof(float) * (qc_gate_stage_words(pg) + (size_t)(NP - theta_off)) : 0;
}

// the balanced launches of both entry points below: defined at the end of this file, so that their kernels lie behind
// every other kernel of the code object
static void adam_bal_launch(const QcAdamArgs& a, bool fold, const float* part, int64_t stride, int RS, size_t lds,
                            const QcBal& bal, hipStream_t st);

int qc_opt_adam(float* flat, int NP, float* prm, float* m, float* v, QcOptState* state, QcOptHyper hp,
                float* hist, int hist_cap, const qc_program* pg, int theta_off, QcTrig* trig, hipStream_t st,
                const QcBal* bal) {
  const QcAdamArgs a = adam_args(flat, NP, prm, m, v, state, hp, hist, hist_cap, pg, theta_off, trig);
  if (bal)
    adam_bal_launch(a, false, nullptr, 0, 0, adam_fast_lds(pg, NP, theta_off), *bal, st);
  else if (adam_fast_ok(NP))
    hipLaunchKernelGGL((k_adam_fast<false>), dim3(1), dim3(1024), adam_fast_lds(pg, NP, theta_off), st, a,
                       (const float*)nullptr, (int64_t)0, 0);
  else
    hipLaunchKernelGGL(k_adam, dim3(1), dim3(1024), 0, st, a);
  return QC_OK;
}

// In-place first level over the step's own partial-row matrix; returns the number of surviving rows.
int qc_opt_fold_rows(float* part, int64_t rows, int64_t stride, int ncols, hipStream_t st) {
  const int RS = (int)(rows < 32 ? rows : 32);
  hipLaunchKernelGGL(k_fold_rows_plain, dim3(qc_ceil_div(ncols, 64), RS), dim3(64 * QC_RED_WAVES), 0, st, part, rows, stride, ncols);
  return RS;
}

// Second level + optimiser update (flat = [grad | 3 loss parts] is written as well).
int qc_opt_adam_fold(const float* part, int64_t stride, int RS, float* flat, int NP, float* prm, float* m, float* v,
                     QcOptState* state, QcOptHyper hp, float* hist, int hist_cap, const qc_program* pg, int theta_off,
                     QcTrig* trig, hipStream_t st, const QcBal* bal) {
  if (adam_fast_ok(NP)) {
    const size_t lds = adam_fast_lds(pg, NP, theta_off);
    const QcAdamArgs a = adam_args(flat, NP, prm, m, v, state, hp, hist, hist_cap, pg, theta_off, trig);
    if (bal) adam_bal_launch(a, true, part, stride, RS, lds, *bal, st);
    else hipLaunchKernelGGL((k_adam_fast<true>), dim3(1), dim3(1024), lds, st, a, part, stride, RS);
    return QC_OK;
  }
  qc_opt_reduce_rows(part, RS, stride, NP + 3, flat, st);
  return qc_opt_adam(flat, NP, prm, m, v, state, hp, hist, hist_cap, pg, theta_off, trig, st, bal);
}

int qc_opt_prep_trig(const qc_program* pg, const float* theta, QcTrig* trig, hipStream_t st) {
  hipLaunchKernelGGL(k_prep_trig, dim3(1), dim3(256), 0, st, pg->d_gates, pg->n_gates, pg->n_qubits, theta, trig,
                     qc_diag_runs_of(pg));
  return QC_OK;
}

// ------------------------------------------------------------------ the balanced update (the balanced step)
// adam_block with BAL set (the fast sizes: k_adam_fast<FOLD, QcBal>): one launch, nothing read back.  a.NP counts the
// balancer's three entries.
namespace {

__global__ void __launch_bounds__(1024) k_adam_bal(QcAdamArgs a, QcBal bal) {
  __shared__ float s_red[16];
  __shared__ float s_term[QC_BAL_N];
  adam_block<true>(a, s_red, &bal, s_term);
}

}  // namespace

// fold: the second reduction level rides in the launch (fast sizes only: the caller reduces first otherwise)
static void adam_bal_launch(const QcAdamArgs& a, bool fold, const float* part, int64_t stride, int RS, size_t lds,
                            const QcBal& bal, hipStream_t st) {
  if (!adam_fast_ok(a.NP)) hipLaunchKernelGGL(k_adam_bal, dim3(1), dim3(1024), 0, st, a, bal);
  else if (fold) hipLaunchKernelGGL((k_adam_fast<true, QcBal>), dim3(1), dim3(1024), lds, st, a, part, stride, RS, bal);
  else hipLaunchKernelGGL((k_adam_fast<false, QcBal>), dim3(1), dim3(1024), lds, st, a, (const float*)nullptr, (int64_t)0, 0, bal);
}

// ------------------------------------------------------------------ causal weighting of the residual rows (the causal step)
// One launch ahead of the weighted fold, kept apart from it: every fold block would otherwise redo the M slab sums.
namespace {

// One block.  Slab i owns the residual rows r with (r + tile_off) mod M = i.  Wave i mod 16 sums its L_r entries: lane l
// adds the slab's rows l, l + 64, ... (ascending) in double, then the 64 lane sums meet in a butterfly over lane distances
// 32, 16, .. 1 (every lane ends with the same bits); L_i = M * that sum.  Thread i < M then adds L_0 .. L_{i-1} in ascending
// order (double) and forms W_i = exp(-eps * sum) in double, rounded to float.  Thread M - 1 holds the smallest weight and
// anneals eps for the next launch.  Everything of the record that is read is read ahead of the barrier, written behind it.
__global__ void __launch_bounds__(1024) k_causal_weights(const float* __restrict__ part, int64_t stride, int col, int rows_res,
                                                         QcCausal c) {
  __shared__ double s_L[QC_CAUSAL_SLABS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, M = c.M;
  int* irec = reinterpret_cast<int*>(c.rec);
  const double eps = (double)c.rec[0];
  const int n_raised = irec[1], n_steps = irec[2], hist_base = irec[3];
  for (int s = wave; s < M; s += 16) {
    const int first = (s - c.tile_off + M) % M;   // tile_off in [0, M)
    double acc = 0.0;
    for (int r = first + lane * M; r < rows_res; r += 64 * M) acc += (double)part[(int64_t)r * stride + col];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) s_L[s] = acc * (double)M;
  }
  __syncthreads();
  if ((int)threadIdx.x < M) {
    const int i = threadIdx.x;
    double cum = 0.0;
    for (int k = 0; k < i; ++k) cum += s_L[k];
    const float W = (float)exp(-eps * cum);
    const float Li = (float)s_L[i];
    c.rec[QC_CAUSAL_HEAD + i] = W;
    c.rec[QC_CAUSAL_HEAD + M + i] = Li;
    const int hi = n_steps - hist_base;
    float* row = (c.hist != nullptr && hi >= 0 && hi < c.hist_cap) ? c.hist + (int64_t)hi * (1 + 2 * M) : nullptr;
    if (row != nullptr) {
      row[1 + i] = W;
      row[1 + M + i] = Li;
    }
    if (i == M - 1) {
      if (row != nullptr) row[0] = (float)eps;
      irec[2] = n_steps + 1;
      if (W > c.delta && (float)eps < c.eps_max) {
        c.rec[0] = (float)fmin(eps * (double)c.growth, (double)c.eps_max);
        irec[1] = n_raised + 1;
      }
    }
  }
}

__global__ void __launch_bounds__(2 * QC_CAUSAL_SLABS) k_causal_init(float* __restrict__ rec, int M, float eps0) {
  const int i = threadIdx.x;
  if (i < 2 * M) rec[QC_CAUSAL_HEAD + i] = i < M ? 1.f : 0.f;
  if (i == 0) {
    int* irec = reinterpret_cast<int*>(rec);
    rec[0] = eps0;
    irec[1] = irec[2] = irec[3] = 0;
  }
}

}  // namespace

int qc_opt_causal_init(float* rec, int M, float eps0, hipStream_t st) {
  hipLaunchKernelGGL(k_causal_init, dim3(1), dim3(2 * QC_CAUSAL_SLABS), 0, st, rec, M, eps0);
  return QC_OK;
}

// In-place first level like qc_opt_fold_rows, under the weights of this call; returns the number of surviving rows.
int qc_opt_causal_fold(float* part, int64_t rows, int64_t rows_res, int64_t stride, int ncols, const QcCausal& cz, hipStream_t st) {
  hipLaunchKernelGGL(k_causal_weights, dim3(1), dim3(1024), 0, st, (const float*)part, stride, ncols - 3, (int)rows_res, cz);
  const int RS = (int)(rows < 32 ? rows : 32);
  const QcCausalRows cw = {cz.rec + QC_CAUSAL_HEAD, (int)rows_res, cz.M, cz.tile_off};
  hipLaunchKernelGGL((k_fold_rows<QcCausalRows>), dim3(qc_ceil_div(ncols, 64), RS), dim3(64 * QC_RED_WAVES), 0, st, part, rows,
                     stride, ncols, cw);
  return RS;
}

// ------------------------------------------------------------------ gradient-norm loss weights (the gradient-norm step)
// Wang, Teng, Perdikaris 2021, Algorithm 1.  The rows of a tile belong to one loss class, so the class fold above leaves
// the three per-class gradients in at most 32 rows each; one single-block launch adds them, moves the weights and writes
// the combined gradient the unchanged optimiser launch then takes.
namespace {

struct QcClassSurv {   // the surviving rows of the class fold: class c in rows [lo_c, lo_c + RS_c), lo_res = 0
  int lo_ic, lo_bc;
  int RS_res, RS_ic, RS_bc;
  int n_ic, n_bc;        // rows of the value classes before the fold (0: an empty class keeps its weight)
};

// The three class sums of columns i0, i0 + 1024, .. (K of them) of one thread: G_c[i] = the left-to-right sum of the class's
// RS_c <= 32 surviving rows.  R rows of all 3 K streams are requested together (a single-block kernel is a chain of
// memory latencies: the small batches take one round trip, 32 rows per class 32 / R); a row a class does not have adds +0.f.
template <int K>
__device__ __forceinline__ void qc_class_sums(const float* __restrict__ part, const int64_t stride, const QcClassSurv& sv,
                                              const int ncols, const int i0, float (&gr)[K], float (&gi)[K], float (&gb)[K]) {
  const float* p_ic = part + (int64_t)sv.lo_ic * stride;
  const float* p_bc = part + (int64_t)sv.lo_bc * stride;
  const int RS = sv.RS_res > sv.RS_ic ? (sv.RS_res > sv.RS_bc ? sv.RS_res : sv.RS_bc) : (sv.RS_ic > sv.RS_bc ? sv.RS_ic : sv.RS_bc);
#pragma unroll
  for (int k = 0; k < K; ++k) gr[k] = gi[k] = gb[k] = 0.f;
  constexpr int R = K > 1 ? 4 : 8;   // 36 or 24 loads in flight: what the 128 registers of a 1024-thread block hold
  for (int j = 0; j < RS; j += R) {
    float xr[K][R], xi[K][R], xb[K][R];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = i0 + k * 1024;
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int64_t o = (int64_t)(j + q) * stride + i;
        xr[k][q] = (i < ncols && j + q < sv.RS_res) ? part[o] : 0.f;
        xi[k][q] = (i < ncols && j + q < sv.RS_ic) ? p_ic[o] : 0.f;
        xb[k][q] = (i < ncols && j + q < sv.RS_bc) ? p_bc[o] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int q = 0; q < R; ++q) {
        gr[k] += xr[k][q];
        gi[k] += xi[k][q];
        gb[k] += xb[k][q];
      }
  }
}
// max that keeps a NaN once it has seen one (fmaxf would drop it, and a NaN must stop the update)
__device__ __forceinline__ float qc_max_nan(const float m, const float x) { return (x > m || x != x) ? x : m; }

// One block.  FAST (ncols <= 3 * 1024): thread t owns columns t, t + 1024, t + 2048 and keeps their three class sums in
// registers; else it strides over the columns and forms the sums a second time behind the barrier (same order, same
// bits).  With n_steps % every == 0 the statistics m_r = max |G_res|, a_k = mean |G_k| over the NP gradient columns: one
// value per thread (columns ascending, sums in double), a butterfly over lane distances 32 .. 1, then the 16 wave values
// in ascending order on every thread; lam_k = min(lam_max, (1 - alpha) lam_k + alpha m_r / a_k) in double, stored as
// float, unless class k is empty, a_k is 0 or m_r or a_k is not finite.  Everything of the record that is read is read
// ahead of the barrier, written behind it.
template <bool FAST>
__global__ void __launch_bounds__(1024) k_gradnorm_combine(const float* __restrict__ part, int64_t stride, int ncols,
                                                           QcClassSurv sv, QcGradnorm g, float* __restrict__ flat,
                                                           float* __restrict__ class_out) {
  __shared__ float s_m[16];
  __shared__ double s_a[2][16];
  __shared__ float s_loss[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NP = ncols - 3;
  int* irec = reinterpret_cast<int*>(g.rec);
  const float lam_bc0 = g.rec[0], lam_ic0 = g.rec[1];
  const int n_steps = irec[2], hist_base = irec[3], n_updates = irec[4];
  float m_r = g.rec[5], a_bc = g.rec[6], a_ic = g.rec[7], hat_bc = g.rec[8], hat_ic = g.rec[9];
  const bool update = n_steps % g.every == 0;
  constexpr int K = FAST ? QC_ADAM_K : 1;
  float gr[K], gi[K], gb[K];
  float mx = 0.f;
  double sb = 0.0, si = 0.0;
  for (int i0 = tid; i0 < ncols; i0 += K * 1024) {   // FAST: one pass
    qc_class_sums<K>(part, stride, sv, ncols, i0, gr, gi, gb);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = i0 + k * 1024;
      if (i < NP) {
        mx = qc_max_nan(mx, fabsf(gr[k]));
        sb += (double)fabsf(gb[k]);
        si += (double)fabsf(gi[k]);
      } else if (i < ncols) {
        s_loss[i - NP] = (gr[k] + gi[k]) + gb[k];
      }
    }
  }
  if (update) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mx = qc_max_nan(mx, __shfl_xor(mx, o));
      sb += __shfl_xor(sb, o);
      si += __shfl_xor(si, o);
    }
    if (lane == 0) {
      s_m[wave] = mx;
      s_a[0][wave] = sb;
      s_a[1][wave] = si;
    }
  }
  __syncthreads();
  float lam_bc = lam_bc0, lam_ic = lam_ic0;
  if (update) {
    float m = s_m[0];
    double b = s_a[0][0], c = s_a[1][0];
    for (int w = 1; w < 16; ++w) {
      m = qc_max_nan(m, s_m[w]);
      b += s_a[0][w];
      c += s_a[1][w];
    }
    const double mr = (double)m, ab = b / (double)NP, ai = c / (double)NP, al = (double)g.alpha;
    const bool ok_bc = sv.n_bc > 0 && isfinite(mr) && isfinite(ab) && ab > 0.0;
    const bool ok_ic = sv.n_ic > 0 && isfinite(mr) && isfinite(ai) && ai > 0.0;
    const double hb = ok_bc ? mr / ab : 0.0, hi_ = ok_ic ? mr / ai : 0.0;
    if (ok_bc) lam_bc = (float)fmin((double)g.lam_max, (1.0 - al) * (double)lam_bc0 + al * hb);
    if (ok_ic) lam_ic = (float)fmin((double)g.lam_max, (1.0 - al) * (double)lam_ic0 + al * hi_);
    m_r = m;
    a_bc = (float)ab;
    a_ic = (float)ai;
    hat_bc = (float)hb;
    hat_ic = (float)hi_;
  }
  for (int i0 = tid; i0 < ncols; i0 += K * 1024) {
    if constexpr (!FAST) qc_class_sums<K>(part, stride, sv, ncols, i0, gr, gi, gb);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = i0 + k * 1024;
      if (i >= ncols) continue;
      flat[i] = i < NP ? fmaf(lam_ic, gi[k], fmaf(lam_bc, gb[k], gr[k])) : s_loss[i - NP];
      if (class_out != nullptr) {
        class_out[i] = gr[k];
        class_out[(int64_t)ncols + i] = gi[k];
        class_out[2 * (int64_t)ncols + i] = gb[k];
      }
    }
  }
  if (tid == 0) {
    const float wl = fmaf(lam_ic * g.w[2], s_loss[2], fmaf(lam_bc * g.w[1], s_loss[1], g.w[0] * s_loss[0]));
    g.rec[0] = lam_bc;
    g.rec[1] = lam_ic;
    irec[2] = n_steps + 1;
    if (update) {
      irec[4] = n_updates + 1;
      g.rec[5] = m_r;
      g.rec[6] = a_bc;
      g.rec[7] = a_ic;
      g.rec[8] = hat_bc;
      g.rec[9] = hat_ic;
    }
    const int hi = n_steps - hist_base;
    if (g.hist != nullptr && hi >= 0 && hi < g.hist_cap) {
      float* row = g.hist + (int64_t)hi * QC_GRADNORM_COLS;
      row[0] = lam_bc;
      row[1] = lam_ic;
      row[2] = m_r;
      row[3] = a_bc;
      row[4] = a_ic;
      row[5] = wl;
      row[6] = update ? 1.f : 0.f;
    }
  }
}

__global__ void __launch_bounds__(64) k_gradnorm_init(float* __restrict__ rec, float lam_bc, float lam_ic) {
  const int i = threadIdx.x;
  if (i < QC_GRADNORM_WORDS) rec[i] = i == 0 ? lam_bc : (i == 1 ? lam_ic : 0.f);   // (0.f: the zero word of the counters too)
}

}  // namespace

int qc_opt_gradnorm_init(float* rec, float lam_bc, float lam_ic, hipStream_t st) {
  hipLaunchKernelGGL(k_gradnorm_init, dim3(1), dim3(64), 0, st, rec, lam_bc, lam_ic);
  return QC_OK;
}

int qc_opt_gradnorm_fold(float* part, int64_t n_res, int64_t n_ic, int64_t n_bc, int64_t stride, int ncols, const QcGradnorm& gn,
                         float* flat, float* class_out, hipStream_t st) {
  const auto surv = [](int64_t n) { return (int)(n < 32 ? n : 32); };
  const QcClassSurv sv = {(int)n_res, (int)(n_res + n_ic), surv(n_res), surv(n_ic), surv(n_bc), (int)n_ic, (int)n_bc};
  const int RS = sv.RS_res > sv.RS_ic ? (sv.RS_res > sv.RS_bc ? sv.RS_res : sv.RS_bc) : (sv.RS_ic > sv.RS_bc ? sv.RS_ic : sv.RS_bc);
  if (RS > 0) {
    const QcClassRows cr = {sv.lo_ic, sv.lo_bc, (int)n_res, (int)n_ic, (int)n_bc};
    hipLaunchKernelGGL((k_fold_rows<QcClassRows>), dim3(qc_ceil_div(ncols, 64), RS, 3), dim3(64 * QC_RED_WAVES), 0, st, part,
                       n_res + n_ic + n_bc, stride, ncols, cr);
  }
  if (ncols <= QC_ADAM_K * 1024)
    hipLaunchKernelGGL((k_gradnorm_combine<true>), dim3(1), dim3(1024), 0, st, (const float*)part, stride, ncols, sv, gn, flat, class_out);
  else
    hipLaunchKernelGGL((k_gradnorm_combine<false>), dim3(1), dim3(1024), 0, st, (const float*)part, stride, ncols, sv, gn, flat, class_out);
  return QC_OK;
}

// ------------------------------------------------------------------ ensembles: the tail, one block per member
// Member blockIdx.y's partial rows -> its flat vector -> (UPDATE) adam_block on its slices, its state record and its own
// trig buffer, with its own hyper-parameter record when there is a table.  The sums have the single-model step's order:
// more than 32 rows are first folded in place as k_fold_rows folds them (k_fold_rows_ens, the member in blockIdx.z; up to
// 32 rows that fold copies every row onto itself and is not launched), then the surviving rows are added left to right,
// as k_adam_fast<true> adds them.
namespace {

__global__ void __launch_bounds__(64 * QC_RED_WAVES) k_fold_rows_ens(float* __restrict__ part, int64_t rows, int64_t stride,
                                                                     int ncols, int64_t member_stride) {
  __shared__ float s[QC_RED_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const int rs = blockIdx.y, RS = gridDim.y;
  part += (int64_t)blockIdx.z * member_stride;
  float a0 = 0.f, a1 = 0.f;
  if (col < ncols) {
    const int64_t r0 = rs + (int64_t)RS * wave;
    const int64_t hop = (int64_t)RS * QC_RED_WAVES;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t r = r0 + k * hop;
      v[k] = r < rows ? part[r * stride + col] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      a0 += v[k];
      a1 += v[k + 1];
    }
    for (int64_t r = r0 + 8 * hop; r < rows; r += 2 * hop) {
      a0 += part[r * stride + col];
      if (r + hop < rows) a1 += part[(r + hop) * stride + col];
    }
  }
  s[wave][lane] = a0 + a1;
  __syncthreads();
  if (wave == 0 && col < ncols) {
    float t = s[0][lane];
#pragma unroll
    for (int w = 1; w < QC_RED_WAVES; ++w) t += s[w][lane];
    part[(int64_t)rs * stride + col] = t;
  }
}

template <bool UPDATE>
__global__ void __launch_bounds__(1024) k_ens_tail(QcAdamArgs a, const float* __restrict__ part, int64_t stride, int RS, QcEns e) {
  __shared__ float s_red[16];
  const int64_t m = blockIdx.y;
  part += m * e.part;
  float* __restrict__ flat = a.flat + m * e.flat;
  for (int i = threadIdx.x; RS > 0 && i < a.NP + 3; i += 1024) {   // (RS = 0: the flat vector is given)
    float t = 0.f;
    for (int j = 0; j < RS; ++j) t += part[(int64_t)j * stride + i];
    flat[i] = t;
  }
  if constexpr (UPDATE) {
    // the member's argument record, in LDS: adam_block indexes the run list in it (a private copy would live in scratch)
    __shared__ QcAdamArgs s_a;
    if (threadIdx.x == 0) {
      s_a = a;
      s_a.flat = flat;
      s_a.prm = a.prm + m * e.prm;
      s_a.m = a.m + m * e.prm;
      s_a.v = a.v + m * e.prm;
      s_a.st = a.st + m;
      if (a.hist != nullptr) s_a.hist = a.hist + m * e.hist;
      s_a.trig = (QcTrig*)((char*)a.trig + m * e.trig);
      if (e.hyper != nullptr) s_a.hp = qc_ens_record(e.hyper, (int)blockIdx.y);
    }
    __syncthreads();   // the record, and the flat vector, written above by other threads than read below
    adam_block(s_a, s_red);
  }
}

}  // namespace

int qc_opt_ens_tail(float* part, int64_t rows, int64_t stride, float* flat, int NP, float* prm, float* m, float* v,
                    QcOptState* state, QcOptHyper hp, float* hist, int hist_cap, const qc_program* pg, int theta_off,
                    QcTrig* trig, int update, const QcEns& e, hipStream_t st) {
  const int RS = (int)(rows < 32 ? rows : 32);
  if (rows > 32)
    hipLaunchKernelGGL(k_fold_rows_ens, dim3(qc_ceil_div(NP + 3, 64), RS, e.M), dim3(64 * QC_RED_WAVES), 0, st, part, rows, stride,
                       NP + 3, e.part);
  const QcAdamArgs a = adam_args(flat, NP, prm, m, v, state, hp, hist, hist_cap, pg, theta_off, trig);
  if (update) hipLaunchKernelGGL((k_ens_tail<true>), dim3(1, e.M), dim3(1024), 0, st, a, (const float*)part, stride, RS, e);
  else hipLaunchKernelGGL((k_ens_tail<false>), dim3(1, e.M), dim3(1024), 0, st, a, (const float*)part, stride, RS, e);
  return QC_OK;
}
