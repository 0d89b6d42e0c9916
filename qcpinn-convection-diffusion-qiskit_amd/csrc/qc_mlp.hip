// Classical pre/post networks of DVPDESolver with forward-mode derivative channels, the PDE
// residual, the weighted MSE loss and their reverse pass.
//
// Replaces, for the fused path, what the reference runs as torch modules + 5 autograd.grad calls
// + loss.backward():
//   pre  : Linear(3,H) -> Tanh -> Linear(H,n)      nn/DVPDESolver.py:37-43
//   post : Linear(n,H) -> Tanh -> Linear(H,1)      nn/DVPDESolver.py:45-51
//   residual = u_t/s_t + v_x u_x/s_x + v_y u_y/s_y - D (u_xx/s_x^2 + u_yy/s_y^2)    nn/pde.py:53-72
//            = c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy) with the coefficients of QcPde
//   targets u(t,x,y), r(t,x,y) (incl. the -400 constant)           data/diffusion_dataset.py:20-38
//   loss parts = MSE(residual, r), MSE(u_bc, u), MSE(u_ic, u)      trainer/diffusion_train.py:44-47
//
// Parameters live in ONE flat fp32 buffer in torch's model.parameters() order:
//   W1[H][3] b1[H] W2[n][H] b2[n] | W3[H][n] b3[H] W4[H] b4 | theta[L*P]
// Gradients leave every kernel as one "partial row" per block ([rows][stride] buffer, same column
// order, 3 extra columns for the loss sums); qc_optim.hip reduces rows in a fixed order, so the
// result is bit-reproducible (no float atomics).
//
// NCH = 6 : residual points, channels {value, d/dt, d/dx, d/dy, d2/dx2, d2/dy2};
// NCH = 1 : boundary / initial-condition points, value channel only.
#include "qc_internal.h"
#include "qc_philox.h"
#include <tuple>

namespace {

// tanh(x) = 1 - 2/(exp(2x)+1) on the hardware exp/rcp units (abs. error ~1e-7; saturates cleanly
// to +-1 for |x| large, where exp overflows to inf or underflows to 0).
// (__frcp_rn is a correctly rounded division on this target: ten instructions with v_div_scale / v_div_fmas / v_div_fixup;
// the hardware reciprocal is 1 ulp, far inside the 1e-7 of the exp approximation.)
__device__ __forceinline__ float qc_tanh(float x) {
  const float e = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// register pairs for the contraction blocks of the six-channel kernels: two derivative channels per 64-bit register,
// v_pk_fma_f32 with a broadcast scalar weight (two multiply-adds per instruction; csrc/qc_gates.h has the issue rates)
typedef float mf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ mf2 m_dup(const float a) { return (mf2){a, a}; }
__device__ __forceinline__ mf2 m_fma(const mf2 a, const mf2 b, const mf2 c) { return __builtin_elementwise_fma(a, b, c); }

// analytic solution and forcing term, data/diffusion_dataset.py:20-38
__device__ __forceinline__ float analytic_u(float t, float x, float y) {
  const float dx = x - 0.5f, dy = y - 0.5f;
  return expf(-100.f * (dx * dx + dy * dy)) * expf(-t);
}
__device__ __forceinline__ float analytic_r(float t, float x, float y, float D, float vx, float vy) {
  const float u = analytic_u(t, x, y);
  const float dx = x - 0.5f, dy = y - 0.5f;
  const float ut = -u, ux = -200.f * dx * u, uy = -200.f * dy * u;
  const float uxx = (40000.f * dx * dx - 400.f) * u;  // the reference's constant (:31-34)
  const float uyy = (40000.f * dy * dy - 400.f) * u;
  return ut + vx * ux + vy * uy - D * (uxx + uyy);
}

// second workload (train_hybrid_qpinn.py:116-131): u = sin(pi x) sin(pi y) exp(-2 pi^2 D t); its PDE
// u_t = D (u_xx + u_yy) has no forcing term, and u vanishes on the four boundary faces
__device__ __forceinline__ float analytic_u_diffusion(float t, float x, float y, float D) {
  const float pi = 3.14159265358979323846f;
  return sinf(pi * x) * sinf(pi * y) * expf(-2.f * pi * pi * D * t);
}

// targets of mode 2 by qc_pde.problem.  Residual: the forcing term r of problem 0, zero for problem 1 (pure diffusion) and
// problem 2 (Gaussian pulse, trainer/train.py:62-93).  Value: the Gaussian pulse (analytic_u, the same function as
// train.py:55-60) on every point of problems 0 and 2; problem 1 takes the diffusion mode on IC points, 0 on the faces.
__device__ __forceinline__ float residual_target(const QcPde& pde, float t, float x, float y) {
  return pde.problem != QC_PB_CONVECTION_DIFFUSION ? 0.f : analytic_r(t, x, y, pde.D, pde.vx, pde.vy);
}
__device__ __forceinline__ float value_target(const QcPde& pde, bool seg_a, float t, float x, float y) {
  return pde.problem == QC_PB_PURE_DIFFUSION ? (seg_a ? analytic_u_diffusion(t, x, y, pde.D) : 0.f) : analytic_u(t, x, y);
}

// ================================================================== output map of the pre network
// MAP = 1 (QC_ANGLE_MAP_TANH_PI): the third workload's encoder ends in Tanh and its circuit embeds RX(pi tanh v_i)
// (trainer/train.py:150-155, :206), so the pre stage emits the jets of a = pi tanh(v) and its reverse pass pulls the angle
// cotangents back through that map first.  MAP = 0 is the identity of the other workloads (same code as before).
constexpr float QC_PI_F = 3.14159265358979323846f;

// forward epilogue of one wire: network output jets v -> angle jets a, with tau = tanh v0 and s = 1 - tau^2:
//   a0 = pi tau,  a_k = pi s v_k (k = t, x, y),  a_kk = pi s (v_kk - 2 tau v_k^2) (k = x, y)
template <int NCH>
__device__ __forceinline__ void angle_map_fwd(const float (&v)[NCH], float (&a)[NCH]) {
  const float tau = qc_tanh(v[0]);
  const float ps = QC_PI_F * (1.f - tau * tau);
  a[0] = QC_PI_F * tau;
  if constexpr (NCH == 6) {
    a[1] = ps * v[1];
    a[2] = ps * v[2];
    a[3] = ps * v[3];
    a[4] = ps * (v[4] - 2.f * tau * v[2] * v[2]);
    a[5] = ps * (v[5] - 2.f * tau * v[3] * v[3]);
  }
}

// reverse prologue of one wire: angle cotangents ab and the stored angle jets a -> cotangents vb of v.  It reads tau from
// a0 / pi and never divides by s, so it stays finite where tanh saturates:
//   vb_kk = pi s ab_kk,  vb_k = pi s ab_k - 4 tau a_k ab_kk (k = x, y),  vb_t = pi s ab_t,
//   vb0 = pi s ab0 - 2 tau sum_{t,x,y} a_k ab_k - sum_{x,y} (2 tau a_kk + 2 a_k^2 / pi) ab_kk
template <int NCH>
__device__ __forceinline__ void angle_map_bwd(const float (&ab)[NCH], const float (&a)[NCH], float (&vb)[NCH]) {
  const float tau = a[0] * (1.f / QC_PI_F);
  const float ps = QC_PI_F * (1.f - tau * tau);
  vb[0] = ps * ab[0];
  if constexpr (NCH == 6) {
    const float tt = 2.f * tau;
    vb[1] = ps * ab[1];
    vb[2] = ps * ab[2] - 2.f * tt * a[2] * ab[4];
    vb[3] = ps * ab[3] - 2.f * tt * a[3] * ab[5];
    vb[4] = ps * ab[4];
    vb[5] = ps * ab[5];
    vb[0] -= tt * (a[1] * ab[1] + a[2] * ab[2] + a[3] * ab[3]) +
             (tt * a[4] + 2.f * a[2] * a[2] * (1.f / QC_PI_F)) * ab[4] +
             (tt * a[5] + 2.f * a[3] * a[3] * (1.f / QC_PI_F)) * ab[5];
  }
}

// ================================================================== pre network, forward jets
// Block = 4 waves on ONE 64-point tile: lane = collocation point, wave w takes a quarter of the
// hidden units (wave-uniform weights -> scalar loads); the four partial angle jets meet in LDS.
// Four waves per tile (instead of one) keep >= 4 waves per SIMD in flight at B = 65 536.
constexpr int QC_MS = 4;

// ------------------------------------------------------------------ hidden-unit blocks of the lane = point kernels
// A wave's hidden units m0 .. m1 - 1 are walked in compile-time blocks of UB units (then one block of 2 and one of 1
// for the remainder).  A block's wave-uniform weights are fetched into one register set at its top: contiguous runs,
// so a few wide scalar loads and ONE wait per block instead of a scalar-memory round trip or two per hidden unit.  With
// PF the next full block's weights are requested before the current block's arithmetic starts and are only waited for
// when it is done.  Fam::Blk<K> is the register set of K units, load(w, m) fills it for units m .. m + K - 1,
// apply(w, m) does their arithmetic: every accumulator still takes its terms one hidden unit at a time in ascending m.
template <class Fam, int UB, bool PF, class Load, class Apply>
__device__ __forceinline__ void qc_unit_blocks(const int m0, const int m1, Load&& load, Apply&& apply) {
  static_assert(UB == 1 || UB == 2 || UB == 4, "remainder blocks: 2, then 1");
  int m = m0;
  const int nblk = m1 > m0 ? (m1 - m0) / UB : 0;
  if constexpr (PF) {
    if (nblk > 0) {
      typename Fam::template Blk<UB> cur;
      load(cur, m);
      for (int b = 1; b <= nblk; ++b) {
        typename Fam::template Blk<UB> nxt;
        load(nxt, b < nblk ? m + UB : m);   // the last pass re-reads its own block: in bounds, never used
        apply(cur, m);
        cur = nxt;
        m += UB;
      }
    }
  } else {
    for (int b = 0; b < nblk; ++b, m += UB) {
      typename Fam::template Blk<UB> w;
      load(w, m);
      apply(w, m);
    }
  }
  if constexpr (UB > 2) {
    if (m + 2 <= m1) {
      typename Fam::template Blk<2> w;
      load(w, m);
      apply(w, m);
      m += 2;
    }
  }
  if constexpr (UB > 1) {
    if (m < m1) {
      typename Fam::template Blk<1> w;
      load(w, m);
      apply(w, m);
    }
  }
}

// block sizes by wire count: the register sets are 3 K + K + N K (pre) and N K + 2 K (post) scalar registers
constexpr int qc_pre_ub(int n) { return n <= 4 ? 4 : (n <= 8 ? 2 : 1); }

template <int N>
struct QcPreW {
  template <int K>
  struct Blk { static constexpr int count = K; float w1[3 * K], b1[K], w2[N][K]; };
};

template <int N, int K>
__device__ __forceinline__ void pre_blk_load(typename QcPreW<N>::template Blk<K>& w, const float* __restrict__ W1,
                                             const float* __restrict__ b1, const float* __restrict__ W2, const int H,
                                             const int m) {
  const float* __restrict__ p1 = W1 + 3 * m;   // one base per run: constant offsets merge into wide loads
  const float* __restrict__ pb = b1 + m;
#pragma unroll
  for (int j = 0; j < 3 * K; ++j) w.w1[j] = p1[j];
#pragma unroll
  for (int j = 0; j < K; ++j) w.b1[j] = pb[j];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float* __restrict__ p2 = W2 + (i * H + m);
#pragma unroll
    for (int j = 0; j < K; ++j) w.w2[i][j] = p2[j];
  }
}

// K hidden units of the pre network on one point: the K tanh chains first (independent, quarter-rate exp / rcp), then
// the multiply-adds unit by unit
template <int N, int NCH, int K>
__device__ __forceinline__ void pre_blk_apply(const typename QcPreW<N>::template Blk<K>& w, const float t, const float x,
                                              const float y, mf2 (&acc2)[NCH == 6 ? 3 : 1][N]) {
  float z[K];
#pragma unroll
  for (int j = 0; j < K; ++j)
    z[j] = qc_tanh(fmaf(w.w1[3 * j], t, fmaf(w.w1[3 * j + 1], x, fmaf(w.w1[3 * j + 2], y, w.b1[j]))));
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if constexpr (NCH == 6) {
      const float w0 = w.w1[3 * j], w1 = w.w1[3 * j + 1], w2 = w.w1[3 * j + 2];
      const float d1 = 1.f - z[j] * z[j], d2 = -2.f * z[j] * d1;
      const mf2 zc2[3] = {(mf2){z[j], d1 * w0}, (mf2){d1 * w1, d1 * w2}, (mf2){d2 * w1 * w1, d2 * w2 * w2}};
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const mf2 wi = m_dup(w.w2[i][j]);
#pragma unroll
        for (int cp = 0; cp < 3; ++cp) acc2[cp][i] = m_fma(wi, zc2[cp], acc2[cp][i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) acc2[0][i].x = fmaf(w.w2[i][j], z[j], acc2[0][i].x);
    }
  }
}

// hidden units m0 .. m1 - 1 of the pre network accumulated into acc2
template <int N, int NCH>
__device__ __forceinline__ void pre_fwd_units(const float* __restrict__ W1, const float* __restrict__ b1,
                                              const float* __restrict__ W2, const int H, const int m0, const int m1,
                                              const float t, const float x, const float y,
                                              mf2 (&acc2)[NCH == 6 ? 3 : 1][N]) {
  constexpr int UB = qc_pre_ub(N);
  qc_unit_blocks<QcPreW<N>, UB, (UB > 1)>(
      m0, m1,
      [&](auto& w, const int m) {
        constexpr int K = std::remove_reference_t<decltype(w)>::count;
        pre_blk_load<N, K>(w, W1, b1, W2, H, m);
      },
      [&](const auto& w, const int) {
        constexpr int K = std::remove_reference_t<decltype(w)>::count;
        pre_blk_apply<N, NCH, K>(w, t, x, y, acc2);
      });
}

template <int N, int NCH, int MAP = 0, bool RF = false>
__device__ __forceinline__ void k_pre_fwd_body(const int64_t bid, const float* __restrict__ X, const float* __restrict__ prm,
                                                 QcLayout L, float* __restrict__ ajets, int64_t B,
                                                 const QcDraw* __restrict__ draw = nullptr, float* __restrict__ Xout = nullptr) {
  __shared__ float s_part[QC_MS][NCH * N][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p = (int64_t)bid * 64 + lane;
  const int64_t pc = p < B ? p : B - 1;
  float t, x, y;
  if (draw != nullptr && draw->enabled) {
    // the step's sampler folded into its first stage: this tile draws its own points (same Philox counters as
    // k_sample) and wave 0 leaves them in X for the later stages
    if (NCH == 6) qc_draw_point(0, draw->off_res + pc, 0, draw->seed, draw->step, t, x, y);
    else if (pc < draw->n_ic) qc_draw_point(1, draw->off_ic + pc, 0, draw->seed, draw->step, t, x, y);
    else qc_draw_point<RF>(2, draw->off_bc + (pc - draw->n_ic), draw->face_pts, draw->seed, draw->step, t, x, y);
    if (wave == 0 && p < B) {
      Xout[p * 3 + 0] = t;
      Xout[p * 3 + 1] = x;
      Xout[p * 3 + 2] = y;
    }
  } else {
    t = X[pc * 3 + 0];
    x = X[pc * 3 + 1];
    y = X[pc * 3 + 2];
  }
  // six channels: the accumulators of channels (0,1), (2,3), (4,5) share a register pair (packed multiply-adds)
  constexpr int NP2 = NCH == 6 ? 3 : 1;
  mf2 acc2[NP2][N];
#pragma unroll
  for (int cp = 0; cp < NP2; ++cp)
#pragma unroll
    for (int i = 0; i < N; ++i) acc2[cp][i] = (mf2){0.f, 0.f};
  const float* W1 = prm + L.oW1;
  const float* b1 = prm + L.ob1;
  const float* W2 = prm + L.oW2;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  const int m0 = wave * hq, m1 = (m0 + hq) < L.H ? (m0 + hq) : L.H;
  pre_fwd_units<N, NCH>(W1, b1, W2, L.H, m0, m1, t, x, y, acc2);
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) s_part[wave][c * N + i][lane] = (c & 1) ? acc2[c >> 1][i].y : acc2[c >> 1][i].x;
  __syncthreads();
  if (p < B) {
    if constexpr (MAP == 0) {
      // compile-time trip count (n <= 8): every LDS read of the wave's rows is in flight before the first sum
      constexpr int NF = (NCH * N + QC_MS - 1) / QC_MS;
      if constexpr (NF <= 12) {
        float v[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          const int f = wave + QC_MS * j, fc = f < NCH * N ? f : 0;
          v[j] = (s_part[0][fc][lane] + s_part[1][fc][lane]) + (s_part[2][fc][lane] + s_part[3][fc][lane]);
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          const int f = wave + QC_MS * j;
          if (f < NCH * N) {
            if (f < N) v[j] += prm[L.ob2 + f];
            qc_store_wt(&ajets[(int64_t)f * B + p], v[j]);
          }
        }
      } else {
        for (int f = wave; f < NCH * N; f += QC_MS) {
          float v = (s_part[0][f][lane] + s_part[1][f][lane]) + (s_part[2][f][lane] + s_part[3][f][lane]);
          if (f < N) v += prm[L.ob2 + f];
          qc_store_wt(&ajets[(int64_t)f * B + p], v);
        }
      }
    } else {
      // the map mixes the channels of one wire: a wave finishes whole wires
      for (int i = wave; i < N; i += QC_MS) {
        float v[NCH], a[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int f = c * N + i;
          v[c] = (s_part[0][f][lane] + s_part[1][f][lane]) + (s_part[2][f][lane] + s_part[3][f][lane]);
        }
        v[0] += prm[L.ob2 + i];
        angle_map_fwd<NCH>(v, a);
#pragma unroll
        for (int c = 0; c < NCH; ++c) qc_store_wt(&ajets[(int64_t)(c * N + i) * B + p], a[c]);
      }
    }
  }
}

template <int N, int NCH, int MAP>
__global__ void __launch_bounds__(256) k_pre_fwd(const float* __restrict__ X, const float* __restrict__ prm,
                                                 QcLayout L, float* __restrict__ ajets, int64_t B) {
  k_pre_fwd_body<N, NCH, MAP>(blockIdx.x, X, prm, L, ajets, B);
}

// ================================================================== pre network, reverse pass
// ------------------------------------------------------------------ tile staging and group sums of these kernels
// Staging: a wave fetches whole 64-point rows of the tile, wave w the rows w, w + nw, ... of the block's nw waves, so a
// row's address is wave-uniform (scalar base) and the lane is the point.  The requests of one chunk of rows, together
// with everything else the block reads from memory (its X values, a thread's weights), are written ahead of the first
// LDS store: ONE memory round trip where a loop of run-time stride made one per row.  A chunk serves every block of
// 192 threads or more; a chunk loop takes the rest of a narrower block's rows.  Lanes at or past cnt read the tile's
// last live point (never memory past the batch) and stage 0.
// Two things the compiler does otherwise: it folds the lane's offset into the row address first and
// then holds one 64-bit vector address per row (sixteen registers a chunk), and it sinks a request into the branch that
// stores its value, where the request waits alone.  So the row address passes through an empty asm as one scalar pair
// (the load's scalar-base form), and qc_pin, placed behind the last request, keeps every request in front of it.
__device__ __forceinline__ float qc_row_load(const float* __restrict__ row, const unsigned lane_off) {
#if defined(__HIP_DEVICE_COMPILE__)
  using G = const __attribute__((address_space(1))) char*;   // (the asm hides that the address is global memory)
  G b = (G)row;
  asm("" : "+s"(b));
  return *(const __attribute__((address_space(1))) float*)(b + (size_t)(lane_off * 4u));
#else
  return row[lane_off];
#endif
}
__device__ __forceinline__ void qc_pin(float& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#endif
}
template <int A, int B2>
__device__ __forceinline__ void qc_pin(float (&v)[A][B2]) {
#pragma unroll
  for (int a = 0; a < A; ++a)
#pragma unroll
    for (int b = 0; b < B2; ++b) qc_pin(v[a][b]);
}
template <int A>
__device__ __forceinline__ void qc_pin(float (&v)[A]) {
#pragma unroll
  for (int a = 0; a < A; ++a) qc_pin(v[a]);
}

// The sums over the PS point groups of hidden unit m's K accumulators (s_acc = [PS][K][HB]), ascending in the group like
// the plain loop.  The reads of GC groups (about forty registers) are all requested before the first add; a group past PS
// reads the last one and adds +0.f instead: a sum that starts at +0.f is never -0.f, so the bits are the plain loop's.
template <int K>
__device__ __forceinline__ void qc_group_sums(const float* s_acc, const int PS, const int HB, const int m, float (&tot)[K]) {
  constexpr int GC = K >= 40 ? 1 : 40 / K;
#pragma unroll
  for (int k = 0; k < K; ++k) tot[k] = 0.f;
  for (int g0 = 0; g0 < PS; g0 += GC) {
    float v[GC][K];
#pragma unroll
    for (int j = 0; j < GC; ++j) {
      const int gc = (g0 + j) < PS ? (g0 + j) : PS - 1;
#pragma unroll
      for (int k = 0; k < K; ++k) v[j][k] = s_acc[((size_t)gc * K + k) * HB + m];
    }
#pragma unroll
    for (int j = 0; j < GC; ++j)
#pragma unroll
      for (int k = 0; k < K; ++k) tot[k] += (g0 + j) < PS ? v[j][k] : 0.f;
  }
}

// For n <= 8.  Above (the circuit is then nine tenths of a step and more) these kernels sit at register limits the batch
// would cross (a wave per SIMD at n = 9, 12, 15, 16, scratch at n = 14 .. 16): they keep the plain loops.
constexpr bool qc_stage_batched(const int n) { return n <= 8; }

// lane = hidden unit (each lane owns one row of W1 / column of W2, so weight gradients need no
// cross-lane reduction).  The block's 64-point tile is staged in LDS and split over PS groups of HB
// threads (16 points each, read as LDS broadcasts); the groups' accumulators meet in LDS.
template <int N, int NCH, int MAP = 0>
__device__ __forceinline__ void k_pre_bwd_body(const int64_t bid, const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                          const float* __restrict__ abar, float* __restrict__ part, int64_t part_stride,
                          int64_t row0, int64_t B, int HB, int PS, const float* __restrict__ aj = nullptr) {
  // six channels: the cotangents of channels (0,1), (2,3), (4,5) of one wire sit side by side in LDS (one 64-bit
  // broadcast read) and ride through the two contraction blocks as register pairs (packed multiply-adds)
  constexpr int NP2 = NCH == 6 ? 3 : 1;
  __shared__ float sX[3][64];
  __shared__ mf2 sA2[NP2 * N][64];   // [cp * N + i][point] = (abar of channel 2 cp, channel 2 cp + 1) (NCH = 1: .x only)
  extern __shared__ float s_acc[];  // [PS][4 + N][HB]
  const int64_t base = (int64_t)bid * 64;
  const int cnt = (int)((B - base) < 64 ? (B - base) : 64);
  int grp, m;   // group and hidden unit of the thread; threads past HB * PS (block rounded up to waves) idle
  float w0, w1, w2, bb, w2c[N];
  constexpr bool BATCH = qc_stage_batched(N);
  if constexpr (BATCH) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const bool live = lane < cnt;
    const unsigned pc = live ? lane : cnt - 1;
    // MAP = 0: a staged row is a row of sA2 (a wire's channel pair: two loads, one 64-bit store; NCH = 1: one and .x).
    // MAP = 1: a staged row is a wire, all its channels of abar and of the angle jets aj: the angle cotangents are pulled
    // back through a = pi tanh(v) on load (angle_map_bwd); the rest of the pass is the MAP = 0 pass on the cotangents of v.
    constexpr int NR = MAP == 0 ? NP2 * N : N;                      // rows to stage
    constexpr int NV = MAP == 0 ? (NCH == 6 ? 2 : 1) : 2 * NCH;     // loads per row
    constexpr int CH = NV == 12 ? 1 : 8 / NV;                       // rows per chunk: 8 loads (12 for a six-channel wire)
    auto request = [&](const int r0, float (&v)[CH][NV]) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int r = r0 + j * nw, rc = r < NR ? r : 0;
        if constexpr (MAP == 0) {
          const int cp = rc / N, w = rc % N;
#pragma unroll
          for (int q = 0; q < NV; ++q) v[j][q] = qc_row_load(abar + ((int64_t)((2 * cp + q) * N + w) * B + base), pc);
        } else {
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int64_t o = (int64_t)(c * N + rc) * B + base;
            v[j][c] = qc_row_load(abar + o, pc);
            v[j][NCH + c] = qc_row_load(aj + o, pc);
          }
        }
      }
    };
    auto put = [&](const int r0, const float (&v)[CH][NV]) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int r = r0 + j * nw;
        if (r < NR) {
          if constexpr (MAP == 0) {
            if constexpr (NCH == 6) sA2[r][lane] = (mf2){live ? v[j][0] : 0.f, live ? v[j][1] : 0.f};
            else sA2[r][lane].x = live ? v[j][0] : 0.f;
          } else {
            float ab[NCH], a[NCH], vb[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
              ab[c] = live ? v[j][c] : 0.f;
              a[c] = live ? v[j][NCH + c] : 0.f;
            }
            angle_map_bwd<NCH>(ab, a, vb);
            if constexpr (NCH == 6) {
#pragma unroll
              for (int cp = 0; cp < 3; ++cp) sA2[cp * N + r][lane] = (mf2){vb[2 * cp], vb[2 * cp + 1]};
            } else {
              sA2[r][lane].x = vb[0];
            }
          }
        }
      }
    };
    // the requests: the wave's first chunk of cotangent rows, its row of the tile's 192 X values, the thread's weights
    float stg[CH][NV];
    request(wave, stg);
    const int xi = (wave < 3 ? wave : 0) * 64 + lane;
    float xv = qc_row_load(X + base * 3, xi < 3 * cnt ? xi : 3 * cnt - 1);
    grp = threadIdx.x / HB, m = threadIdx.x % HB;
    const int mc = m < L.H ? m : L.H - 1;      // (a thread without a hidden unit reads the last one's)
    w0 = prm[L.oW1 + 3 * mc], w1 = prm[L.oW1 + 3 * mc + 1], w2 = prm[L.oW1 + 3 * mc + 2];
    bb = prm[L.ob1 + mc];
#pragma unroll
    for (int i = 0; i < N; ++i) w2c[i] = prm[L.oW2 + i * L.H + mc];
    // one wait, then the LDS stores
    qc_pin(stg);
    qc_pin(xv);
    qc_pin(w0);
    qc_pin(w1);
    qc_pin(w2);
    qc_pin(bb);
    qc_pin(w2c);
    if (wave < 3) sX[xi % 3][xi / 3] = xi < 3 * cnt ? xv : 0.f;
    put(wave, stg);
    // blocks of fewer than three waves, or of fewer waves than a chunk covers: the rows left
    for (int r = wave + nw; r < 3; r += nw) {
      const int i = r * 64 + lane;
      sX[i % 3][i / 3] = i < 3 * cnt ? X[base * 3 + i] : 0.f;
    }
    for (int r0 = wave + CH * nw; r0 < NR; r0 += CH * nw) {
      request(r0, stg);
      qc_pin(stg);
      put(r0, stg);
    }
  } else {
    for (int i = threadIdx.x; i < 64 * 3; i += blockDim.x) {
      const int pp = i / 3, k = i % 3;
      sX[k][pp] = pp < cnt ? X[(base + pp) * 3 + k] : 0.f;
    }
    if constexpr (MAP == 0) {
      for (int i = threadIdx.x; i < NCH * N * 64; i += blockDim.x) {
        const int f = i >> 6, pp = i & 63;      // f = c * N + i
        const int c = f / N, w = f % N;
        const float v = pp < cnt ? abar[(int64_t)f * B + base + pp] : 0.f;
        if (c & 1) sA2[(c >> 1) * N + w][pp].y = v;
        else sA2[(c >> 1) * N + w][pp].x = v;
      }
    } else {
      for (int i = threadIdx.x; i < N * 64; i += blockDim.x) {
        const int w = i >> 6, pp = i & 63;
        float ab[NCH], a[NCH], vb[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int64_t o = (int64_t)(c * N + w) * B + base + pp;
          ab[c] = pp < cnt ? abar[o] : 0.f;
          a[c] = pp < cnt ? aj[o] : 0.f;
        }
        angle_map_bwd<NCH>(ab, a, vb);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          if (c & 1) sA2[(c >> 1) * N + w][pp].y = vb[c];
          else sA2[(c >> 1) * N + w][pp].x = vb[c];
        }
      }
    }
  }
  __syncthreads();

  if constexpr (!BATCH) grp = threadIdx.x / HB, m = threadIdx.x % HB;
  const int per = (64 + PS - 1) / PS;
  const int p0 = grp * per, p1 = (p0 + per) < cnt ? (p0 + per) : cnt;
  float gW1[3] = {0.f, 0.f, 0.f}, gb1 = 0.f;
  mf2 gW2p[N];
#pragma unroll
  for (int i = 0; i < N; ++i) gW2p[i] = (mf2){0.f, 0.f};
  if (grp < PS && m < L.H) {
    if constexpr (!BATCH) {
      w0 = prm[L.oW1 + 3 * m], w1 = prm[L.oW1 + 3 * m + 1], w2 = prm[L.oW1 + 3 * m + 2];
      bb = prm[L.ob1 + m];
#pragma unroll
      for (int i = 0; i < N; ++i) w2c[i] = prm[L.oW2 + i * L.H + m];
    }
    for (int pp = p0; pp < p1; ++pp) {
      const float t = sX[0][pp], x = sX[1][pp], y = sX[2][pp];
      const float h = fmaf(w0, t, fmaf(w1, x, fmaf(w2, y, bb)));
      const float z = qc_tanh(h);
      const float d1 = 1.f - z * z;
      if constexpr (NCH == 6) {
        mf2 a2[3][N], zb2[3];
#pragma unroll
        for (int cp = 0; cp < 3; ++cp) {
          zb2[cp] = (mf2){0.f, 0.f};
#pragma unroll
          for (int i = 0; i < N; ++i) {
            a2[cp][i] = sA2[cp * N + i][pp];
            zb2[cp] = m_fma(m_dup(w2c[i]), a2[cp][i], zb2[cp]);
          }
        }
        const float d2 = -2.f * z * d1;
        const float d3 = -2.f * (d1 * d1 + z * d2);
        const mf2 zc2[3] = {(mf2){z, d1 * w0}, (mf2){d1 * w1, d1 * w2}, (mf2){d2 * w1 * w1, d2 * w2 * w2}};
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
          for (int cp = 0; cp < 3; ++cp) gW2p[i] = m_fma(a2[cp][i], zc2[cp], gW2p[i]);
        const float zb[6] = {zb2[0].x, zb2[0].y, zb2[1].x, zb2[1].y, zb2[2].x, zb2[2].y};
        const float hb = zb[0] * d1 + (zb[1] * w0 + zb[2] * w1 + zb[3] * w2) * d2 +
                         (zb[4] * w1 * w1 + zb[5] * w2 * w2) * d3;
        gW1[0] += hb * t + zb[1] * d1;
        gW1[1] += hb * x + zb[2] * d1 + 2.f * zb[4] * d2 * w1;
        gW1[2] += hb * y + zb[3] * d1 + 2.f * zb[5] * d2 * w2;
        gb1 += hb;
      } else {
        float zb0 = 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const float a = sA2[i][pp].x;
          zb0 = fmaf(w2c[i], a, zb0);
          gW2p[i].x = fmaf(a, z, gW2p[i].x);
        }
        const float hb = zb0 * d1;
        gW1[0] += hb * t;
        gW1[1] += hb * x;
        gW1[2] += hb * y;
        gb1 += hb;
      }
    }
  }
  if (grp < PS) {
    float* mine = s_acc + (size_t)grp * (4 + N) * HB;
    mine[0 * HB + m] = gW1[0];
    mine[1 * HB + m] = gW1[1];
    mine[2 * HB + m] = gW1[2];
    mine[3 * HB + m] = gb1;
#pragma unroll
    for (int i = 0; i < N; ++i) mine[(4 + i) * HB + m] = gW2p[i].x + gW2p[i].y;
  }
  __syncthreads();
  float* row = part + (row0 + bid) * part_stride;
  if (grp == 0 && m < L.H) {
    float tot[4 + N];
    if constexpr (BATCH) {
      qc_group_sums<4 + N>(s_acc, PS, HB, m, tot);
    } else {
#pragma unroll
      for (int k = 0; k < 4 + N; ++k) {
        float sum = 0.f;
        for (int g2 = 0; g2 < PS; ++g2) sum += s_acc[((size_t)g2 * (4 + N) + k) * HB + m];
        tot[k] = sum;
      }
    }
    row[L.oW1 + 3 * m] = tot[0];
    row[L.oW1 + 3 * m + 1] = tot[1];
    row[L.oW1 + 3 * m + 2] = tot[2];
    row[L.ob1 + m] = tot[3];
#pragma unroll
    for (int i = 0; i < N; ++i) row[L.oW2 + i * L.H + m] = tot[4 + i];
  }
  if (threadIdx.x < N) {  // b2 only feeds the value channel
    float sum = 0.f;
    for (int pp = 0; pp < cnt; ++pp) sum += sA2[threadIdx.x][pp].x;
    row[L.ob2 + threadIdx.x] = sum;
  }
}

template <int N, int NCH, int MAP>
__global__ void k_pre_bwd(const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                          const float* __restrict__ abar, float* __restrict__ part, int64_t part_stride,
                          int64_t row0, int64_t B, int HB, int PS, const float* __restrict__ aj) {
  k_pre_bwd_body<N, NCH, MAP>(blockIdx.x, X, prm, L, abar, part, part_stride, row0, B, HB, PS, aj);
}

// ================================================================== post network + PDE + loss
// Point kernel: lane = collocation point (scalar weights), 4 tiles per block.
// MODE 0: forward only  -> u, residual
// MODE 1: reverse only: cotangents (ubar, rbar) come from memory (autograd path) -> qbar
// MODE 2: forward + analytic targets + squared error (loss sums into the tile's partial row)
//         + reverse -> qbar; the per-point cotangents (ubar, rbar-scale) are left in ub_out[2][B]
// MODE 3: reverse only, GENERAL cotangents: in_ubar = [6][B], one per derivative channel of u (operators that are not
//         linear in the channels, e.g. Navier-Stokes' u u_x) -> qbar
// MODE 4: forward only, all six channels of u -> out_u[6][B] (value, d/dt, d/dx, d/dy, d2/dx2, d2/dy2)
// The weight gradients of W3/b3/W4/b4 are NOT formed here (they would need ~300 cross-lane
// reductions per wave): k_post_wg below forms them with lane = hidden unit.
template <int N, int NCH>
__device__ __forceinline__ void post_cotangents(float (&gb)[NCH], float& gw4, const float (&g)[NCH],
                                                const float (&ub)[NCH], const float z, const float w4) {
  const float d1 = 1.f - z * z;
  gw4 = ub[0] * z;
  gb[0] = ub[0] * d1;
  if constexpr (NCH == 6) {
    const float d2 = -2.f * z * d1;
    const float d3 = -2.f * (d1 * d1 + z * d2);
    const float gx2 = g[2] * g[2], gy2 = g[3] * g[3];
    const float lin = ub[1] * g[1] + ub[2] * g[2] + ub[3] * g[3];
    gw4 += d1 * lin + ub[4] * (d2 * gx2 + d1 * g[4]) + ub[5] * (d2 * gy2 + d1 * g[5]);
    gb[0] += d2 * lin + ub[4] * (d3 * gx2 + d2 * g[4]) + ub[5] * (d3 * gy2 + d2 * g[5]);
    gb[1] = ub[1] * d1;
    gb[2] = ub[2] * d1 + 2.f * ub[4] * d2 * g[2];
    gb[3] = ub[3] * d1 + 2.f * ub[5] * d2 * g[3];
    gb[4] = ub[4] * d1;
    gb[5] = ub[5] * d1;
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) gb[c] *= w4;
}

template <int NCH>
__device__ __forceinline__ void expand_ub(float (&ub)[NCH], float ub0, float gsc, const QcPde& pde) {
  ub[0] = ub0;
  if constexpr (NCH == 6) {
    ub[1] = gsc * pde.c_t;
    ub[2] = gsc * pde.c_x;
    ub[3] = gsc * pde.c_y;
    ub[4] = -pde.d_xx * gsc;
    ub[5] = -pde.d_yy * gsc;
  }
}

// The N + 1 sums of one hidden unit of the K-output kernels (dW3[m][0..N), db3[m]) after qc_wave_sum_merged: sum r is in
// its home lane and register (csrc/qc_common.h), and that lane stores its column of the tile row: one store per chunk of
// sixteen sums; a chunk of one or two is unmerged and stored from lane 63.
template <int N, int C = 0>
__device__ __forceinline__ void post_store_w3b3(float* __restrict__ row, const QcLayout& L, const float (&wg)[N + 1], const int m,
                                                const int lane) {
  if constexpr (C * 16 < N + 1) {
    if constexpr (qc_ws_merged(N + 1, C * 16)) {
      const int r = C * 16 + qc_wave_sum_home_index(lane);
      if (qc_wave_sum_is_home(lane) && r <= N) row[r < N ? L.oW3 + m * N + r : L.ob3 + m] = wg[C * 16];
    } else if (lane == 63) {
#pragma unroll
      for (int r = C * 16; r <= N; ++r) row[r < N ? L.oW3 + m * N + r : L.ob3 + m] = wg[r];
    }
    post_store_w3b3<N, C + 1>(row, L, wg, m, lane);
  }
}

// LEARN (the inverse step): the operator is global and trainable.  The seven c_k = fmaf(scale_k, p_k, base_k) are formed once
// per wave from the wave-uniform p = prm[NP_L - 7 ..] (L.NP counts them) and take the place of a coefficient row.
__device__ __forceinline__ void learn_coefs(float (&cf)[QC_COEF_N], const float* __restrict__ prm, const QcLayout& L,
                                            const float (&base)[QC_COEF_N], const float (&scale)[QC_COEF_N]) {
  const float* __restrict__ pk = prm + (L.NP - QC_COEF_N);
#pragma unroll
  for (int k = 0; k < QC_COEF_N; ++k) cf[k] = fmaf(scale[k], pk[k], base[k]);
}
// Their gradient columns in the tile's row (wave 0): d loss / d c_k = sum over the tile's points of gsc times the term c_k
// multiplies (dead lanes: gsc = 0), in fixed order, scaled by scale_k; exactly 0 for a frozen entry.  Tile 0 of a launch
// with a history buffer also stores the c_k it used, in the row of the step the optimiser record is in.
// `z`: 0, or the opaque zero of learn_late().
__device__ __forceinline__ void learn_columns(float* __restrict__ row, const QcLayout& L, const QcLearn* lr, const int z,
                                              const float (&scale)[QC_COEF_N], const float (&cf)[QC_COEF_N], const float gsc,
                                              const float (&u)[6], const int lane, const bool tile0) {
  float gv[QC_COEF_N] = {gsc * u[0], gsc * u[1], gsc * u[2], gsc * u[3], -gsc * u[4], -gsc * u[5], gsc * (u[0] * u[0] * u[0])};
  // (unmerged: a per-lane pick of scale[k] for the home lanes costs these kernels scratch, and wave 0 runs this once per tile)
  qc_wave_sum_multi_to_lane63<QC_COEF_N>(gv);
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < QC_COEF_N; ++k) row[L.NP - QC_COEF_N + k] = scale[k] == 0.f ? 0.f : scale[k] * gv[k];
    if (tile0) {
      float* hist = (&lr->hist)[z];
      const QcOptState* st = (&lr->st)[z];
      if (hist != nullptr && st != nullptr) {
        const int hi = st->step - st->hist_base;
        if (hi >= 0 && hi < (&lr->hist_cap)[z]) {
#pragma unroll
          for (int k = 0; k < QC_COEF_N; ++k) hist[(int64_t)hi * QC_COEF_N + k] = cf[k];
        }
      }
    }
  }
}
// The record is a kernel argument, and its fields would be fetched at the kernel's entry: eighteen more scalar registers
// through phase A cost the fused kernels a resident wave (n = 2) or scalar spills (n = 4, 8).  Indexed with a zero the
// compiler cannot see through, they are scalar loads where they are first needed, behind the tile's first barrier.
__device__ __forceinline__ int learn_late() {
  int z = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(z));
#endif
  return z;
}
__device__ __forceinline__ void learn_read(const QcLearn* lr, const int z, float (&base)[QC_COEF_N], float (&scale)[QC_COEF_N]) {
#pragma unroll
  for (int k = 0; k < QC_COEF_N; ++k) {
    base[k] = lr->base[k + z];
    scale[k] = lr->scale[k + z];
  }
}
// a value tile's row: the seven columns are zero (the partial rows are scratch, and the fold sums every row)
__device__ __forceinline__ void learn_zero_columns(float* __restrict__ row, const QcLayout& L) {
#pragma unroll
  for (int k = 0; k < QC_COEF_N; ++k) row[L.NP - QC_COEF_N + k] = 0.f;
}

// BAL (the balanced step, with DATA): the cotangent scale of a tile's class is pde.w_* e_k, e_k = qc_bal_factor(scale_k, p_k)
// with p = prm[NP_B - 3 ..] (order residual, BC, IC; L.NP counts them; segment a = IC, b = BC).  p and scale are
// wave-uniform, read like the learned operator's p[7]; the product is formed once per wave, where the error is first needed,
// and handed back to a scalar register, so the per-point code is the tabulated kind's with a different scalar.  A residual
// tile needs one factor, a value tile two.
template <int NCH>
__device__ __forceinline__ void bal_weights(QcPde& pde, const float* __restrict__ prm, const QcLayout& L, const QcBal* bl) {
  const float* __restrict__ pk = prm + (L.NP - QC_BAL_N);
  auto uniform = [](const float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
  };
  if constexpr (NCH == 6) {
    pde.w_res = uniform(pde.w_res * qc_bal_factor(bl->scale[0], pk[0]));
  } else {
    pde.w_val_b = uniform(pde.w_val_b * qc_bal_factor(bl->scale[1], pk[1]));
    pde.w_val_a = uniform(pde.w_val_a * qc_bal_factor(bl->scale[2], pk[2]));
  }
}
// every tile's row: the three columns are zero (their gradient is a function of the reduced loss columns and is formed in
// the optimiser launch; the partial rows are scratch, and the fold sums every row)
__device__ __forceinline__ void bal_zero_columns(float* __restrict__ row, const QcLayout& L) {
#pragma unroll
  for (int k = 0; k < QC_BAL_N; ++k) row[L.NP - QC_BAL_N + k] = 0.f;
}

// DATA (MODE 2 only, QC_PB_TABULATED): the point's target is tg[p] instead of the analytic function of X, and the residual
// carries the zeroth-order term c_u u, whose cotangent on u is c_u gsc.  DATA = false is the code as it was.
// COEF (with DATA, residual points only): the operator is the point's own row coef[k][p], k = c_u, c_t, c_x, c_y, d_xx,
// d_yy, c_3 (QC_COEF_N), with the cubic term c_3 u^3; pde.c_* / d_* and c_u are not read.  The unit cotangent of the
// reverse pass is then per lane, and the cubic term adds a second direction, the unit cotangent of u alone (N more
// accumulators): its weight 3 c_3 u^2 is only known after the loop.  out_u receives all six channel cotangents [6][B]
// (the weight-gradient kernel runs in its gen mode on them); out_res is not written.
// LEARN (with DATA): residual points run the COEF arithmetic on the uniform c_k of `lr` and wave 0 adds their gradient
// columns; value points only zero those columns.  OPC below: either of the two.
// BAL (with DATA): see bal_weights; every tile zeroes the three columns of its row.
template <int N, int NCH, int MODE, bool DATA = false, bool COEF = false, bool LEARN = false, bool BAL = false>
__device__ __forceinline__ void k_post_body(const int64_t bid, const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                                              QcPde pde, const float* __restrict__ qjets,
                                              float* __restrict__ out_u, float* __restrict__ out_res,
                                              const float* __restrict__ in_ubar, const float* __restrict__ in_rbar,
                                              float* __restrict__ qbar, float* __restrict__ part,
                                              int64_t part_stride, int64_t row0, int64_t B,
                                              const float* __restrict__ tg = nullptr, const float c_u = 0.f,
                                              const float* __restrict__ coef = nullptr, const QcLearn* lr = nullptr,
                                              const QcBal* bl = nullptr) {
  static_assert(!DATA || MODE == 2, "tabulated targets: the fused mode only");
  static_assert(!COEF || (DATA && NCH == 6), "per-point operators: tabulated residual points only");
  static_assert(!LEARN || (DATA && !COEF), "learned operators: tabulated targets, no table");
  static_assert(!BAL || (DATA && !COEF && !LEARN), "balanced weights: the tabulated kind's operator");
  constexpr bool OPC = COEF || (LEARN && NCH == 6);
  // block = 4 waves on one 64-point tile; wave w owns a quarter of the hidden units
  __shared__ float s_buf[QC_MS][NCH * N][64];   // partial u jets first (NCH rows), partial qbar later
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = bid;
  const int64_t p = tile * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  float q[NCH][N];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) q[c][i] = qjets[((int64_t)c * N + i) * B + pc];
  float cf[OPC ? QC_COEF_N : 1];
  if constexpr (COEF) {
#pragma unroll
    for (int k = 0; k < QC_COEF_N; ++k) cf[k] = coef[(int64_t)k * B + pc];
  }
  float lbase[LEARN && NCH == 6 ? QC_COEF_N : 1], lscale[LEARN && NCH == 6 ? QC_COEF_N : 1];
  if constexpr (LEARN && NCH == 6) {
    learn_read(lr, 0, lbase, lscale);
    learn_coefs(cf, prm, L, lbase, lscale);
  }
  const float* W3 = prm + L.oW3;
  const float* b3 = prm + L.ob3;
  const float* W4 = prm + L.oW4;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  const int m0 = wave * hq, m1 = (m0 + hq) < L.H ? (m0 + hq) : L.H;

  float ub0 = 0.f, gsc = 0.f;  // cotangent of u, and of the residual
  float k3 = 0.f;              // COEF: 3 c_3 u^2, the weight of the second direction
  float qbu0[OPC ? N : 1];     // COEF: reverse pass of the unit cotangent of u alone
  if constexpr (OPC) {
#pragma unroll
    for (int i = 0; i < N; ++i) qbu0[i] = 0.f;
  }
  // MODE 2: the reverse pass is linear in its single non-zero cotangent (the residual's for residual points,
  // u's for value points), so it is accumulated for a UNIT cotangent inside the forward loop and scaled
  // afterwards - the pre-activations and tanh are formed once per hidden unit, not twice.
  float qbu[MODE == 2 ? NCH : 1][N];
  if constexpr (MODE == 2) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < N; ++i) qbu[c][i] = 0.f;
  }
  if constexpr (MODE == 0 || MODE == 2 || MODE == 4) {
    float u[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) u[c] = 0.f;
    float ub_unit[NCH];
    if constexpr (OPC) {
      ub_unit[0] = cf[0]; ub_unit[1] = cf[1]; ub_unit[2] = cf[2]; ub_unit[3] = cf[3]; ub_unit[4] = -cf[4]; ub_unit[5] = -cf[5];
    } else {
      expand_ub<NCH>(ub_unit, NCH == 6 ? (DATA ? c_u : 0.f) : 1.f, NCH == 6 ? 1.f : 0.f, pde);
    }
    for (int m = m0; m < m1; ++m) {
      float g[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        float sum = (c == 0) ? b3[m] : 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) sum = fmaf(W3[m * N + i], q[c][i], sum);
        g[c] = sum;
      }
      const float z = qc_tanh(g[0]);
      const float w4 = W4[m];
      u[0] = fmaf(w4, z, u[0]);
      if constexpr (NCH == 6) {
        const float d1 = 1.f - z * z, d2 = -2.f * z * d1;
        u[1] = fmaf(w4, d1 * g[1], u[1]);
        u[2] = fmaf(w4, d1 * g[2], u[2]);
        u[3] = fmaf(w4, d1 * g[3], u[3]);
        u[4] = fmaf(w4, d2 * g[2] * g[2] + d1 * g[4], u[4]);
        u[5] = fmaf(w4, d2 * g[3] * g[3] + d1 * g[5], u[5]);
      }
      if constexpr (MODE == 2) {
        float gb[NCH], gw4;
        post_cotangents<N, NCH>(gb, gw4, g, ub_unit, z, w4);
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const float w3 = W3[m * N + i];
#pragma unroll
          for (int c = 0; c < NCH; ++c) qbu[c][i] = fmaf(w3, gb[c], qbu[c][i]);
        }
        if constexpr (OPC) {   // post_cotangents of ub = (1, 0, ..): gb[0] = w4 d1 and nothing else
          const float g0 = w4 * (1.f - z * z);
#pragma unroll
          for (int i = 0; i < N; ++i) qbu0[i] = fmaf(W3[m * N + i], g0, qbu0[i]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) s_buf[wave][c][lane] = u[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      u[c] = (s_buf[0][c][lane] + s_buf[1][c][lane]) + (s_buf[2][c][lane] + s_buf[3][c][lane]);
    __syncthreads();   // s_buf is reused for the qbar partials below
    u[0] += prm[L.ob4];
    if constexpr (MODE == 4) {
      if (live && wave == 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) out_u[(int64_t)c * B + p] = u[c];
      }
      return;
    }
    float res = 0.f;
    if constexpr (OPC) {
      res = cf[1] * u[1] + cf[2] * u[2] + cf[3] * u[3] - (cf[4] * u[4] + cf[5] * u[5]);
      res = fmaf(fmaf(cf[6] * u[0], u[0], cf[0]), u[0], res);
      k3 = 3.f * cf[6] * u[0] * u[0];
    } else if constexpr (NCH == 6) {
      res = pde.c_t * u[1] + pde.c_x * u[2] + pde.c_y * u[3] - (pde.d_xx * u[4] + pde.d_yy * u[5]);
    }
    if constexpr (NCH == 6 && DATA && !OPC) res = fmaf(c_u, u[0], res);
    if constexpr (MODE == 0) {
      if (live && wave == 0) {
        if (out_u) out_u[p] = u[0];
        if constexpr (NCH == 6)
          if (out_res) out_res[p] = res;
      }
      return;
    } else {
      float t = 0.f, x = 0.f, y = 0.f, tgp = 0.f;
      if constexpr (DATA) {
        tgp = tg[pc];
      } else {
        t = X[pc * 3 + 0]; x = X[pc * 3 + 1]; y = X[pc * 3 + 2];
      }
      float* row = part + (row0 + tile) * part_stride;
      if constexpr (BAL) bal_weights<NCH>(pde, prm, L, bl);
      if constexpr (NCH == 6) {
        const float target = DATA ? tgp : residual_target(pde, t, x, y);
        const float e = live ? res - target : 0.f;
        gsc = pde.w_res * e;
        if constexpr (OPC) ub0 = (cf[0] + k3) * gsc;
        else if constexpr (DATA) ub0 = c_u * gsc;   // reaches k_post_wg through out_u (W4 / b4 / hidden-layer gradients)
        if (wave == 0) {
          const float ls = qc_wave_sum_to_lane63(e * e * pde.inv_n_res);
          if (lane == 63) {
            row[L.NP + 0] = ls;
            row[L.NP + 1] = 0.f;
            row[L.NP + 2] = 0.f;
            if constexpr (BAL) bal_zero_columns(row, L);
          }
          if constexpr (LEARN) learn_columns(row, L, lr, 0, lscale, cf, gsc, u, lane, tile == 0);
        }
      } else {
        const bool seg_a = p < pde.n_seg_a;
        const float target = DATA ? tgp : value_target(pde, seg_a, t, x, y);
        const float e = live ? u[0] - target : 0.f;
        ub0 = (seg_a ? pde.w_val_a : pde.w_val_b) * e;
        if (wave == 0) {
          const float la = qc_wave_sum_to_lane63(seg_a ? e * e * pde.inv_n_a : 0.f);
          const float lb = qc_wave_sum_to_lane63(seg_a ? 0.f : e * e * pde.inv_n_b);
          if (lane == 63) {
            row[L.NP + 0] = 0.f;
            row[L.NP + 1] = lb;  // column order: residual, BC, IC; segment a = IC, b = BC
            row[L.NP + 2] = la;
            if constexpr (LEARN) learn_zero_columns(row, L);
            if constexpr (BAL) bal_zero_columns(row, L);
          }
        }
      }
      if constexpr (OPC) {
        if (live && wave == 0) {  // the six channel cotangents, for k_post_wg in its gen mode
          out_u[p] = ub0;
          out_u[B + p] = gsc * cf[1];
          out_u[2 * B + p] = gsc * cf[2];
          out_u[3 * B + p] = gsc * cf[3];
          out_u[4 * B + p] = -cf[4] * gsc;
          out_u[5 * B + p] = -cf[5] * gsc;
        }
      } else if (live && wave == 0) {  // hand the per-point cotangents to k_post_wg
        out_u[p] = ub0;
        if constexpr (NCH == 6) out_res[p] = gsc;
      }
    }
  }
  if constexpr (MODE == 1) {
    ub0 = (live && in_ubar) ? in_ubar[pc] : 0.f;
    if constexpr (NCH == 6) gsc = (live && in_rbar) ? in_rbar[pc] : 0.f;
  }
  if constexpr (MODE == 2) {
    const float scale = NCH == 6 ? gsc : ub0;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if constexpr (OPC) s_buf[wave][c * N + i][lane] = scale * (c == 0 ? fmaf(k3, qbu0[i], qbu[c][i]) : qbu[c][i]);
        else s_buf[wave][c * N + i][lane] = scale * qbu[c][i];
      }
    __syncthreads();
    if (live) {
      for (int f = wave; f < NCH * N; f += QC_MS)
        qbar[(int64_t)f * B + p] = (s_buf[0][f][lane] + s_buf[1][f][lane]) + (s_buf[2][f][lane] + s_buf[3][f][lane]);
    }
  }
  if constexpr (MODE == 1 || MODE == 3) {
    float ub[NCH];
    if constexpr (MODE == 3) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) ub[c] = live ? in_ubar[(int64_t)c * B + pc] : 0.f;
    } else {
      expand_ub<NCH>(ub, ub0, gsc, pde);
    }
    float qb[NCH][N];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < N; ++i) qb[c][i] = 0.f;
    for (int m = m0; m < m1; ++m) {
      float g[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        float sum = (c == 0) ? b3[m] : 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) sum = fmaf(W3[m * N + i], q[c][i], sum);
        g[c] = sum;
      }
      const float z = qc_tanh(g[0]);
      float gb[NCH], gw4;
      post_cotangents<N, NCH>(gb, gw4, g, ub, z, W4[m]);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float w3 = W3[m * N + i];
#pragma unroll
        for (int c = 0; c < NCH; ++c) qb[c][i] = fmaf(w3, gb[c], qb[c][i]);
      }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < N; ++i) s_buf[wave][c * N + i][lane] = qb[c][i];
    __syncthreads();
    if (live) {
      for (int f = wave; f < NCH * N; f += QC_MS)
        qbar[(int64_t)f * B + p] = (s_buf[0][f][lane] + s_buf[1][f][lane]) + (s_buf[2][f][lane] + s_buf[3][f][lane]);
    }
  }
}

// Target kind of a mode-2 point kernel = its TRAILING arguments: none (analytic targets, computed from X), a QcTab
// (qc_post_data, the data step), or a QcTab and the coefficient table (qc_post_coef, the coefficient step).  One kernel
// template per launch shape takes them as a pack, so the analytic instantiations carry no argument for them.  QcKind
// names the DATA / COEF flags of the bodies and picks what the bodies take out of the pack, where they take it: null /
// zero for what the kind does not have or does not read (c_u beside a coefficient table).
// (QcTab, QcLearn): the inverse step, the trainable global operator by value; its residual bodies take no table.
// (QcTab, QcBal): the balanced step, the tabulated kind (c_u is read) with the balancer's record by value.
template <class... TG>
struct QcKind {
  static_assert(sizeof...(TG) <= 2, "(), (QcTab), (QcTab, const float*), (QcTab, QcLearn) or (QcTab, QcBal)");
  static constexpr bool data = sizeof...(TG) >= 1;
  static constexpr bool learn = (std::is_same_v<TG, QcLearn> || ...);
  static constexpr bool bal = (std::is_same_v<TG, QcBal> || ...);
  static constexpr bool coef = sizeof...(TG) == 2 && !learn && !bal;
  static __device__ __forceinline__ const float* tg_res(const TG&... t) {
    if constexpr (data) return std::get<0>(std::tie(t...)).tg_res; else return nullptr;
  }
  static __device__ __forceinline__ const float* tg_val(const TG&... t) {
    if constexpr (data) return std::get<0>(std::tie(t...)).tg_val; else return nullptr;
  }
  static __device__ __forceinline__ float c_u(const TG&... t) {
    if constexpr (data && !coef && !learn) return std::get<0>(std::tie(t...)).c_u; else return 0.f;
  }
  static __device__ __forceinline__ const QcLearn* op(const TG&... t) {
    if constexpr (learn) return &std::get<1>(std::tie(t...)); else return nullptr;
  }
  static __device__ __forceinline__ const QcBal* weights(const TG&... t) {
    if constexpr (bal) return &std::get<1>(std::tie(t...)); else return nullptr;
  }
  static __device__ __forceinline__ const float* table(const TG&... t) {
    if constexpr (coef) return std::get<1>(std::tie(t...)); else return nullptr;
  }
};

// With target arguments (MODE 2 only) X, in_ubar and in_rbar are not read; with a coefficient table (six channels only)
// out_u is the [6][B] cotangent scratch and out_res is not written.
template <int N, int NCH, int MODE, class... TG>
__global__ void __launch_bounds__(256) k_post(const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                                              QcPde pde, const float* __restrict__ qjets,
                                              float* __restrict__ out_u, float* __restrict__ out_res,
                                              const float* __restrict__ in_ubar, const float* __restrict__ in_rbar,
                                              float* __restrict__ qbar, float* __restrict__ part,
                                              int64_t part_stride, int64_t row0, int64_t B, TG... tg) {
  using K = QcKind<TG...>;
  k_post_body<N, NCH, MODE, K::data, K::coef, K::learn, K::bal>(blockIdx.x, X, prm, L, pde, qjets, out_u, out_res, in_ubar, in_rbar,
                                                                qbar, part, part_stride, row0, B,
                                                                NCH == 6 ? K::tg_res(tg...) : K::tg_val(tg...), K::c_u(tg...),
                                                                K::table(tg...), K::op(tg...), K::weights(tg...));
}

// Weight gradients of the post network: lane = hidden unit m (owns row m of W3, b3[m], W4[m]); the
// block walks its 64-point tile, reading the tile's <Z> jets and per-point cotangents from LDS as
// broadcasts.  No cross-lane reduction; one partial row per tile.
template <int N, int NCH>
__device__ __forceinline__ void k_post_wg_body(const int64_t bid, const float* __restrict__ prm, QcLayout L, QcPde pde, const float* __restrict__ qjets,
                          const float* __restrict__ ubar, const float* __restrict__ rbar,
                          float* __restrict__ part, int64_t part_stride, int64_t row0, int64_t B, int HB, int PS,
                          int gen = 0) {
  __shared__ float sQ[NCH * N][64];
  __shared__ float sU[NCH == 6 ? 6 : 2][64];   // rows 0, 1: (ubar, rbar); gen: one row per derivative channel of u
  extern __shared__ float s_acc[];  // [PS][N + 2][HB]
  const int64_t base = (int64_t)bid * 64;
  const int cnt = (int)((B - base) < 64 ? (B - base) : 64);
  int grp, m;   // group and hidden unit of the thread; threads past HB * PS (block rounded up to waves) idle
  float w3[N], b3m, w4;
  constexpr bool BATCH = qc_stage_batched(N);
  if constexpr (BATCH) {
    // staged by whole rows, the first chunk's requests and the thread's weights ahead of the first LDS store (see
    // qc_row_load): eight rows of <Z> jets and two cotangent rows per wave
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const bool live = lane < cnt;
    const unsigned pc = live ? lane : cnt - 1;
    constexpr int NRQ = NCH * N, CHQ = 8, CHU = 2;
    const int NRU = (NCH == 6 && gen) ? 6 : 2;   // gen: one row per channel of ubar; else (ubar, rbar), either may be absent
    auto request_q = [&](const int r0, float (&v)[CHQ]) {
#pragma unroll
      for (int j = 0; j < CHQ; ++j) {
        const int r = r0 + j * nw, rc = r < NRQ ? r : 0;
        v[j] = qc_row_load(qjets + ((int64_t)rc * B + base), pc);
      }
    };
    auto put_q = [&](const int r0, const float (&v)[CHQ]) {
#pragma unroll
      for (int j = 0; j < CHQ; ++j) {
        const int r = r0 + j * nw;
        if (r < NRQ) sQ[r][lane] = live ? v[j] : 0.f;
      }
    };
    auto source_u = [&](const int r) -> const float* {   // nullptr: the row stages zeros
      if (r >= NRU) return nullptr;
      if (NCH == 6 && gen) return ubar + ((int64_t)r * B + base);
      const float* src = r == 0 ? ubar : rbar;
      return src != nullptr ? src + base : nullptr;
    };
    auto request_u = [&](const int r0, float (&v)[CHU]) {
#pragma unroll
      for (int j = 0; j < CHU; ++j) {
        const float* src = source_u(r0 + j * nw);
        v[j] = qc_row_load(src != nullptr ? src : qjets + base, pc);
      }
    };
    auto put_u = [&](const int r0, const float (&v)[CHU]) {
#pragma unroll
      for (int j = 0; j < CHU; ++j) {
        const int r = r0 + j * nw;
        if (r < NRU) sU[r][lane] = (live && source_u(r) != nullptr) ? v[j] : 0.f;
      }
    };
    // (ubar, rbar) of a six-channel tile keep their loop, one trip of half the block at 128 threads or more: with these two
    // rows in the batch the merged kernel of n = 4 holds 71 vector registers against 63 and loses its eighth wave
    const bool batch_u = NCH == 1 || gen;
    float stq[CHQ], stu[CHU];
    request_q(wave, stq);
    if (batch_u) request_u(wave, stu);
    grp = threadIdx.x / HB, m = threadIdx.x % HB;
    const int mc = m < L.H ? m : L.H - 1;      // (a thread without a hidden unit reads the last one's)
#pragma unroll
    for (int i = 0; i < N; ++i) w3[i] = prm[L.oW3 + mc * N + i];
    b3m = prm[L.ob3 + mc], w4 = prm[L.oW4 + mc];
    qc_pin(stq);
    if (batch_u) qc_pin(stu);
    qc_pin(w3);
    qc_pin(b3m);
    qc_pin(w4);
    put_q(wave, stq);
    if (batch_u) put_u(wave, stu);
    for (int r0 = wave + CHQ * nw; r0 < NRQ; r0 += CHQ * nw) {
      request_q(r0, stq);
      qc_pin(stq);
      put_q(r0, stq);
    }
    if (batch_u) {
      for (int r0 = wave + CHU * nw; r0 < NRU; r0 += CHU * nw) {
        request_u(r0, stu);
        qc_pin(stu);
        put_u(r0, stu);
      }
    } else {
      for (int i = threadIdx.x; i < 128; i += blockDim.x) {
        const int k = i >> 6, pp = i & 63;
        const float* src = k == 0 ? ubar : rbar;
        sU[k][pp] = (pp < cnt && src != nullptr) ? src[base + pp] : 0.f;
      }
    }
  } else {
    for (int i = threadIdx.x; i < NCH * N * 64; i += blockDim.x) {
      const int f = i >> 6, pp = i & 63;
      sQ[f][pp] = pp < cnt ? qjets[(int64_t)f * B + base + pp] : 0.f;
    }
    if (NCH == 6 && gen) {
      for (int i = threadIdx.x; i < 6 * 64; i += blockDim.x) {
        const int k = i >> 6, pp = i & 63;
        sU[k][pp] = pp < cnt ? ubar[(int64_t)k * B + base + pp] : 0.f;
      }
    } else {
      for (int i = threadIdx.x; i < 128; i += blockDim.x) {
        const int k = i >> 6, pp = i & 63;
        const float* src = k == 0 ? ubar : rbar;
        sU[k][pp] = (pp < cnt && src != nullptr) ? src[base + pp] : 0.f;
      }
    }
  }
  __syncthreads();
  if constexpr (!BATCH) grp = threadIdx.x / HB, m = threadIdx.x % HB;
  const int per = (64 + PS - 1) / PS;
  const int p0 = grp * per, p1 = (p0 + per) < cnt ? (p0 + per) : cnt;
  float gW3[N], gb3 = 0.f, gW4 = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) gW3[i] = 0.f;
  if (grp < PS && m < L.H) {
    if constexpr (!BATCH) {
#pragma unroll
      for (int i = 0; i < N; ++i) w3[i] = prm[L.oW3 + m * N + i];
      b3m = prm[L.ob3 + m], w4 = prm[L.oW4 + m];
    }
    for (int pp = p0; pp < p1; ++pp) {
      float g[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        float sum = (c == 0) ? b3m : 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) sum = fmaf(w3[i], sQ[c * N + i][pp], sum);
        g[c] = sum;
      }
      const float z = qc_tanh(g[0]);
      float ub[NCH];
      if (NCH == 6 && gen) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) ub[c] = sU[c < (NCH == 6 ? 6 : 2) ? c : 0][pp];
      } else {
        expand_ub<NCH>(ub, sU[0][pp], sU[1][pp], pde);
      }
      float gb[NCH], gw4;
      post_cotangents<N, NCH>(gb, gw4, g, ub, z, w4);
      gW4 += gw4;
      gb3 += gb[0];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float sum = gW3[i];
#pragma unroll
        for (int c = 0; c < NCH; ++c) sum = fmaf(gb[c], sQ[c * N + i][pp], sum);
        gW3[i] = sum;
      }
    }
  }
  if (grp < PS) {
    float* mine = s_acc + (size_t)grp * (N + 2) * HB;
#pragma unroll
    for (int i = 0; i < N; ++i) mine[i * HB + m] = gW3[i];
    mine[N * HB + m] = gb3;
    mine[(N + 1) * HB + m] = gW4;
  }
  __syncthreads();
  float* row = part + (row0 + bid) * part_stride;
  if (grp == 0 && m < L.H) {
    float tot[N + 2];
    if constexpr (BATCH) {
      qc_group_sums<N + 2>(s_acc, PS, HB, m, tot);
    } else {
#pragma unroll
      for (int k = 0; k < N + 2; ++k) {
        float sum = 0.f;
        for (int g2 = 0; g2 < PS; ++g2) sum += s_acc[((size_t)g2 * (N + 2) + k) * HB + m];
        tot[k] = sum;
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) row[L.oW3 + m * N + i] = tot[i];
    row[L.ob3 + m] = tot[N];
    row[L.oW4 + m] = tot[N + 1];
  }
  if (threadIdx.x == 0) {
    float sum = 0.f;
    for (int pp = 0; pp < cnt; ++pp) sum += sU[0][pp];
    row[L.ob4] = sum;
  }
}

template <int N, int NCH>
__global__ void k_post_wg(const float* __restrict__ prm, QcLayout L, QcPde pde, const float* __restrict__ qjets,
                          const float* __restrict__ ubar, const float* __restrict__ rbar,
                          float* __restrict__ part, int64_t part_stride, int64_t row0, int64_t B, int HB, int PS, int gen) {
  k_post_wg_body<N, NCH>(blockIdx.x, prm, L, pde, qjets, ubar, rbar, part, part_stride, row0, B, HB, PS, gen);
}

// ================================================================== value tiles, one wave per tile
// In the merged launches a value tile (64 boundary / initial points, value channel only) is too little work to
// split four ways with two LDS round trips: here each of a block's 4 waves owns one whole tile (all hidden units,
// scalar weights, no LDS, no barrier).  Same arithmetic as the NCH = 1 instances of the kernels above; the four
// per-quarter partial sums are still formed and added as (p0 + p1) + (p2 + p3) (same association as the m-split form).
template <int N, int MAP = 0, bool RF = false>
__device__ __forceinline__ void k_pre_fwd_value4(const int64_t bid, const float* __restrict__ X, const float* __restrict__ prm,
                                                 QcLayout L, float* __restrict__ ajets, int64_t B,
                                                 const QcDraw* __restrict__ draw, float* __restrict__ Xout) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = bid * 4 + wave;
  if (tile * 64 >= B) return;
  const int64_t p = tile * 64 + lane;
  const int64_t pc = p < B ? p : B - 1;
  float t, x, y;
  if (draw != nullptr && draw->enabled) {
    if (pc < draw->n_ic) qc_draw_point(1, draw->off_ic + pc, 0, draw->seed, draw->step, t, x, y);
    else qc_draw_point<RF>(2, draw->off_bc + (pc - draw->n_ic), draw->face_pts, draw->seed, draw->step, t, x, y);
    if (p < B) {
      Xout[p * 3 + 0] = t;
      Xout[p * 3 + 1] = x;
      Xout[p * 3 + 2] = y;
    }
  } else {
    t = X[pc * 3 + 0];
    x = X[pc * 3 + 1];
    y = X[pc * 3 + 2];
  }
  const float* W1 = prm + L.oW1;
  const float* b1 = prm + L.ob1;
  const float* W2 = prm + L.oW2;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  float part[QC_MS][N];
#pragma unroll
  for (int k = 0; k < QC_MS; ++k) {
    mf2 acc[1][N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[0][i] = (mf2){0.f, 0.f};
    const int m0 = k * hq, m1 = (m0 + hq) < L.H ? (m0 + hq) : L.H;
    pre_fwd_units<N, 1>(W1, b1, W2, L.H, m0, m1, t, x, y, acc);
#pragma unroll
    for (int i = 0; i < N; ++i) part[k][i] = acc[0][i].x;
  }
  if (p < B) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float v = ((part[0][i] + part[1][i]) + (part[2][i] + part[3][i])) + prm[L.ob2 + i];
      if constexpr (MAP == 0) {
        qc_store_wt(&ajets[(int64_t)i * B + p], v);
      } else {
        const float vv[1] = {v};
        float a[1];
        angle_map_fwd<1>(vv, a);
        qc_store_wt(&ajets[(int64_t)i * B + p], a[0]);
      }
    }
  }
}

// fused (mode 2) post stage of a value tile: u, squared error against the analytic target, cotangent of <Z>
template <int N, bool DATA = false, bool LEARN = false, bool BAL = false>
__device__ __forceinline__ void k_post_value4(const int64_t bid, const float* __restrict__ X, const float* __restrict__ prm,
                                              QcLayout L, QcPde pde, const float* __restrict__ qjets,
                                              float* __restrict__ out_u, float* __restrict__ qbar, float* __restrict__ part,
                                              int64_t part_stride, int64_t row0, int64_t B,
                                              const float* __restrict__ tg = nullptr, const QcBal* bl = nullptr) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = bid * 4 + wave;
  if (tile * 64 >= B) return;
  const int64_t p = tile * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  float q[N];
#pragma unroll
  for (int i = 0; i < N; ++i) q[i] = qjets[(int64_t)i * B + pc];
  const float* W3 = prm + L.oW3;
  const float* b3 = prm + L.ob3;
  const float* W4 = prm + L.oW4;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  float up[QC_MS], qbu[QC_MS][N];
#pragma unroll
  for (int k = 0; k < QC_MS; ++k) {
    up[k] = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) qbu[k][i] = 0.f;
    const int m0 = k * hq, m1 = (m0 + hq) < L.H ? (m0 + hq) : L.H;
    for (int m = m0; m < m1; ++m) {
      float g = b3[m];
#pragma unroll
      for (int i = 0; i < N; ++i) g = fmaf(W3[m * N + i], q[i], g);
      const float z = qc_tanh(g);
      const float w4 = W4[m];
      up[k] = fmaf(w4, z, up[k]);
      const float gb = (1.f - z * z) * w4;          // post_cotangents<N, 1> for a unit cotangent of u
#pragma unroll
      for (int i = 0; i < N; ++i) qbu[k][i] = fmaf(W3[m * N + i], gb, qbu[k][i]);
    }
  }
  const float u = ((up[0] + up[1]) + (up[2] + up[3])) + prm[L.ob4];
  const bool seg_a = p < pde.n_seg_a;
  float target;
  if constexpr (DATA) {
    target = tg[pc];
  } else {
    const float t = X[pc * 3 + 0], x = X[pc * 3 + 1], y = X[pc * 3 + 2];
    target = value_target(pde, seg_a, t, x, y);
  }
  if constexpr (BAL) bal_weights<1>(pde, prm, L, bl);
  const float e = live ? u - target : 0.f;
  const float ub0 = (seg_a ? pde.w_val_a : pde.w_val_b) * e;
  const float la = qc_wave_sum_to_lane63(seg_a ? e * e * pde.inv_n_a : 0.f);
  const float lb = qc_wave_sum_to_lane63(seg_a ? 0.f : e * e * pde.inv_n_b);
  if (lane == 63) {
    float* row = part + (row0 + tile) * part_stride;
    row[L.NP + 0] = 0.f;
    row[L.NP + 1] = lb;  // column order: residual, BC, IC; segment a = IC, b = BC
    row[L.NP + 2] = la;
    if constexpr (LEARN) learn_zero_columns(row, L);
    if constexpr (BAL) bal_zero_columns(row, L);
  }
  if (live) {
    out_u[p] = ub0;
#pragma unroll
    for (int i = 0; i < N; ++i)
      qbar[(int64_t)i * B + p] = (ub0 * qbu[0][i] + ub0 * qbu[1][i]) + (ub0 * qbu[2][i] + ub0 * qbu[3][i]);
  }
}

// ================================================================== post stage of the training step in ONE kernel
// (MODE 2 of k_post + k_post_wg).  lane = collocation point throughout, weights are scalar operands:
//   phase A  u jets of the tile (pre-activations, tanh once per (point, hidden unit); the tanh values of a residual tile
//            are parked in LDS), residual, analytic target, squared error -> the point's cotangent (gsc or ub0);
//   phase B  with the ACTUAL cotangent: cotangents of the pre-activations gb_c, the <Z> jet cotangents
//            qbar_c[i] += W3[m][i] gb_c, and the weight gradients in the same lanes: the per-point products
//            sum_c gb_c q_c[i] (W3), gb_0 (b3), gw4 (W4) are summed over the wave's 64 points by DPP reductions and
//            stored straight into the tile's partial row - one row entry has exactly one producing wave.
// The lane = hidden-unit kernel (k_post_wg) recomputed pre-activations, tanh and cotangents per (hidden unit, point)
// from LDS copies of the jets: ~130 wave-instructions per (point, 64 hidden lanes) for what costs 24 multiply-adds and
// a few reductions here.  Residual tiles: k_post_fused6_body below; value tiles: this body.
//
// Value tiles (64 boundary / initial points, value channel only): TPB tiles per block, WPT = 4 / TPB waves per tile.
// Wave k of a tile owns the hidden-unit quarters [k QPW, (k + 1) QPW) of the same quarter split as the four-wave kernels
// (QPW = 4 / WPT quarters per wave), so u is still formed as (q0 + q1) + (q2 + q3) from the same quarter sums.  Per tile
// the LDS holds s_g = [H][64] (the tanh values of phase A, overwritten in place by the pre-activation cotangents of
// phase B) and the waves' u partials [WPT][64].  After phase B wave k forms qbar[i] for i = k, k + WPT, ... as ONE chain
// of multiply-adds over m = 0 .. H - 1 from s_g: the same sums in the same order as a single wave walking every hidden
// unit, so the tile's outputs - u, the loss sums, qbar and every row entry - do not depend on WPT.  A block's tiles past
// the end of the batch skip the work but still meet the barriers.
// Measured at BASELINE config 2 (merged stage isolated): 1 tile x 4 waves (683 blocks after the 1 024
// residual blocks) 24.5 us, 2 tiles x 2 waves 27.4, 4 tiles x 1 wave (round 3) 27.9.
constexpr int QC_POST_VALUE_TPB = 1;   // value tiles per block of the fused post stage

// hidden-unit blocks of the fused post stage (qc_unit_blocks): W3 rows m .. m + K - 1 are one run of K N floats
template <int N>
struct QcPostW {
  template <int K>
  struct Blk { static constexpr int count = K; float w3[K][N], b3[K], w4[K]; };
};
template <int N, int K>
__device__ __forceinline__ void post_blk_load(typename QcPostW<N>::template Blk<K>& w, const float* __restrict__ W3,
                                              const float* __restrict__ b3, const float* __restrict__ W4, const int m) {
  const float* __restrict__ p3 = W3 + m * N;   // one base per run: constant offsets merge into wide loads
  const float* __restrict__ pb = b3 + m;
  const float* __restrict__ p4 = W4 + m;
#pragma unroll
  for (int j = 0; j < K; ++j)
#pragma unroll
    for (int i = 0; i < N; ++i) w.w3[j][i] = p3[j * N + i];
#pragma unroll
  for (int j = 0; j < K; ++j) w.b3[j] = pb[j];
#pragma unroll
  for (int j = 0; j < K; ++j) w.w4[j] = p4[j];
}
// one column of W3 for K consecutive hidden units (the qbar chains of the value tiles)
struct QcColW {
  template <int K>
  struct Blk { static constexpr int count = K; float c[K]; };
};
// phase A.  (n = 3 in blocks of 4 takes the merged kernel from 80 to 102 scalar registers, 7 waves per SIMD instead of
// 8; in blocks of 2 it needs 93 and keeps 8)
constexpr int qc_post_ub_a(int n) { return n == 3 ? 2 : (n <= 4 ? 4 : (n <= 8 ? 2 : 1)); }
constexpr bool qc_post_pf(int n) { return n <= 8; }   // prefetch of the next block
constexpr int qc_post_ub_vb(int n) { return n <= 8 ? 2 : 1; }                 // phase B of a value tile: two reductions side by side

// The weight-gradient sums of one block of K hidden units, reduced by qc_wave_sum_merged: value j (N + 2) + r is unit
// m + j's dW3[r] (r < N), db3 (r = N) or dW4 (r = N + 1), and ends in its home lane of register 16 (k / 16) (k = the
// value's index; the home-lane map of csrc/qc_common.h).  Every home lane stores its own column of the tile row, one store per
// sixteen values; the column is col0 + m cstep, two lane constants formed once per wave.
template <int N, int KMAX>
struct QcPostCols {
  static constexpr int NC = (KMAX * (N + 2) + 15) / 16;
  unsigned col0[NC], cstep[NC];
  bool home;
  __device__ __forceinline__ QcPostCols(const QcLayout& L, const int lane) {
    home = qc_wave_sum_is_home(lane);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int k = 16 * c + qc_wave_sum_home_index(lane), j = k / (N + 2), r = k % (N + 2);
      col0[c] = r < N ? L.oW3 + j * N + r : (r == N ? L.ob3 : L.oW4) + j;
      cstep[c] = r < N ? N : 1;
    }
  }
  template <int K>
  __device__ __forceinline__ void store(float* __restrict__ row, const QcLayout& L, const float (&wg)[K * (N + 2)], const int m,
                                        const int lane) const {
    static_assert(K <= KMAX, "columns formed for KMAX units");
    store_chunk<K, 0>(row, L, wg, m, lane);
  }
  template <int K, int C>
  __device__ __forceinline__ void store_chunk(float* __restrict__ row, const QcLayout& L, const float (&wg)[K * (N + 2)],
                                              const int m, const int lane) const {
    constexpr int NV = K * (N + 2);
    if constexpr (C * 16 < NV) {
      if constexpr (qc_ws_merged(NV, C * 16)) {
        if (home && 16 * C + qc_wave_sum_home_index(lane) < NV) row[col0[C] + __umul24(m, cstep[C])] = wg[qc_wave_sum_home_reg(NV, C * 16)];
      } else if (lane == 63) {   // one or two values left over: unmerged, in lane 63 of their own registers
#pragma unroll
        for (int k = C * 16; k < NV; ++k) {
          const int j = k / (N + 2), r = k % (N + 2);
          row[r < N ? L.oW3 + (m + j) * N + r : (r == N ? L.ob3 : L.oW4) + m + j] = wg[k];
        }
      }
      store_chunk<K, C + 1>(row, L, wg, m, lane);
    }
  }
};

template <int N, int TPB, bool DATA = false, bool LEARN = false, bool BAL = false>
__device__ __forceinline__ void k_post_fused_value_body(const int64_t bid, const float* __restrict__ X,
                                                        const float* __restrict__ prm, QcLayout L, QcPde pde,
                                                        const float* __restrict__ qjets, float* __restrict__ out_u,
                                                        float* __restrict__ qbar, float* __restrict__ part,
                                                        int64_t part_stride, int64_t row0, int64_t B,
                                                        float* __restrict__ s_v, const float* __restrict__ tg = nullptr,
                                                        const QcBal* bl = nullptr) {
  constexpr int WPT = QC_MS / TPB, QPW = QC_MS / WPT;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = wave / WPT, wt = wave % WPT;   // the block's tile, and this wave's place in it
  const int64_t tile = bid * TPB + slot;
  const bool tile_ok = tile * 64 < B;
  const int64_t p = tile * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  float* s_g = s_v + (size_t)slot * (L.H + WPT) * 64;   // [H][64]
  float* s_u = s_g + L.H * 64;                           // [WPT][64]
  float q[N];
#pragma unroll
  for (int i = 0; i < N; ++i) q[i] = qjets[(int64_t)i * B + pc];
  const float* W3 = prm + L.oW3;
  const float* b3 = prm + L.ob3;
  const float* W4 = prm + L.oW4;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  const int m0 = tile_ok ? wt * QPW * hq : 0;
  const int m1 = !tile_ok ? 0 : ((m0 + QPW * hq) < L.H ? (m0 + QPW * hq) : L.H);
  // ---------------- phase A: this wave's quarter sums of u; tanh values parked
  float up[QPW];
#pragma unroll
  for (int k = 0; k < QPW; ++k) {
    up[k] = 0.f;
    const int k0 = m0 + k * hq, k1 = (k0 + hq) < m1 ? (k0 + hq) : m1;
    qc_unit_blocks<QcPostW<N>, qc_post_ub_a(N), qc_post_pf(N)>(
        k0, k1,
        [&](auto& w, const int m) { post_blk_load<N, std::remove_reference_t<decltype(w)>::count>(w, W3, b3, W4, m); },
        [&](const auto& w, const int m) {
          constexpr int K = std::remove_reference_t<decltype(w)>::count;
          float z[K];
#pragma unroll
          for (int j = 0; j < K; ++j) {
            float g = w.b3[j];
#pragma unroll
            for (int i = 0; i < N; ++i) g = fmaf(w.w3[j][i], q[i], g);
            z[j] = qc_tanh(g);
          }
#pragma unroll
          for (int j = 0; j < K; ++j) {
            s_g[(m + j) * 64 + lane] = z[j];
            up[k] = fmaf(w.w4[j], z[j], up[k]);
          }
        });
  }
  float u;
  if constexpr (QPW == 4) u = (up[0] + up[1]) + (up[2] + up[3]);
  else s_u[wt * 64 + lane] = QPW == 2 ? up[0] + up[1] : up[0];
  __syncthreads();
  if constexpr (WPT == 2) u = s_u[lane] + s_u[64 + lane];
  if constexpr (WPT == 4) u = (s_u[lane] + s_u[64 + lane]) + (s_u[128 + lane] + s_u[192 + lane]);
  u += prm[L.ob4];
  // ---------------- error / loss sums / per-point cotangent (every wave of the tile needs ub0; wave 0 stores)
  float* row = part + (row0 + tile) * part_stride;
  const bool seg_a = p < pde.n_seg_a;
  float target;
  if constexpr (DATA) {
    target = tg[pc];
  } else {
    const float t = X[pc * 3 + 0], x = X[pc * 3 + 1], y = X[pc * 3 + 2];
    target = value_target(pde, seg_a, t, x, y);
  }
  if constexpr (BAL) bal_weights<1>(pde, prm, L, bl);
  const float e = live ? u - target : 0.f;
  const float ub0 = (seg_a ? pde.w_val_a : pde.w_val_b) * e;
  if (wt == 0 && tile_ok) {
    const float la = qc_wave_sum_to_lane63(seg_a ? e * e * pde.inv_n_a : 0.f);
    const float lb = qc_wave_sum_to_lane63(seg_a ? 0.f : e * e * pde.inv_n_b);
    // d loss / d b4 = sum of the points' cotangents of u
    const float sb4 = qc_wave_sum_to_lane63(ub0);
    if (lane == 63) {
      row[L.NP + 0] = 0.f;
      row[L.NP + 1] = lb;  // column order: residual, BC, IC; segment a = IC, b = BC
      row[L.NP + 2] = la;
      row[L.ob4] = sb4;
      if constexpr (LEARN) learn_zero_columns(row, L);
      if constexpr (BAL) bal_zero_columns(row, L);
    }
    if (live) out_u[p] = ub0;   // the per-point cotangent (MODE 2 contract of qc_post)
  }
  // ---------------- phase B over the same hidden units: weight gradients; gb parked in place of tanh
  float ub[1];
  expand_ub<1>(ub, ub0, 0.f, pde);
  // W4 only: K values per block; the K units' reductions run as one merged reduction (same tree for every value)
  const QcPostCols<N, qc_post_ub_vb(N)> cols(L, lane);
  qc_unit_blocks<QcColW, qc_post_ub_vb(N), false>(
      m0, m1,
      [&](auto& w, const int m) {
#pragma unroll
        for (int j = 0; j < std::remove_reference_t<decltype(w)>::count; ++j) w.c[j] = W4[m + j];
      },
      [&](const auto& w, const int m) {
        constexpr int K = std::remove_reference_t<decltype(w)>::count;
        float wg[K * (N + 2)];
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const float g[1] = {0.f};   // post_cotangents reads no pre-activation for one channel
          float gb[1], gw4;
          post_cotangents<N, 1>(gb, gw4, g, ub, s_g[(m + j) * 64 + lane], w.c[j]);
          s_g[(m + j) * 64 + lane] = gb[0];
#pragma unroll
          for (int i = 0; i < N; ++i) wg[j * (N + 2) + i] = fmaf(gb[0], q[i], 0.f);
          wg[j * (N + 2) + N] = gb[0];
          wg[j * (N + 2) + N + 1] = gw4;
        }
        qc_wave_sum_merged<K * (N + 2)>(wg);
        cols.template store<K>(row, L, wg, m, lane);
      });
  __syncthreads();
  // ---------------- qbar[i] = sum over m of W3[m][i] gb(m), one chain per i
  if (live) {
    const int mh = tile_ok ? L.H : 0;
    for (int i = wt; i < N; i += WPT) {
      float qb = 0.f;
      // column i of W3, four hidden units per block: their scalar loads and LDS reads are issued together
      qc_unit_blocks<QcColW, 4, true>(
          0, mh,
          [&](auto& w, const int m) {
#pragma unroll
            for (int j = 0; j < std::remove_reference_t<decltype(w)>::count; ++j) w.c[j] = W3[(m + j) * N + i];
          },
          [&](const auto& w, const int m) {
            constexpr int K = std::remove_reference_t<decltype(w)>::count;
            float gbv[K];
#pragma unroll
            for (int j = 0; j < K; ++j) gbv[j] = s_g[(m + j) * 64 + lane];
#pragma unroll
            for (int j = 0; j < K; ++j) qb = fmaf(w.c[j], gbv[j], qb);
          });
      qc_store_wt(&qbar[(int64_t)i * B + p], qb);
    }
  }
}

// Residual tiles (six channels, four waves per tile) of the fused post stage with the three contraction blocks on
// register PAIRS: channels (0,1), (2,3), (4,5) of the <Z> jets ride in the two halves of one 64-bit register, so
//   g_c = sum_i W3[m][i] q_c[i],   qbar_c[i] += W3[m][i] gb_c,   sum_c gb_c q_c[i]
// are v_pk_fma_f32 with a broadcast scalar weight: two multiply-adds per instruction at the issue cost of one and a
// bit (csrc/qc_gates.h, tools/ubench/valu_issue.hip).  Other order of the sums over channel pairs in the weight-gradient
// products than the scalar six-channel form.
// LDS: one dynamic buffer s_dyn of qc_post_fused_lds() floats.  Through phase B it holds the parked tanh values
// s_z = [H][64] and, behind them, the u-jet exchange [4][6][64]; once every wave is past phase B the qbar exchange
// [4][6N][64] reuses it from the start (24 KiB at H = 50, n = 4, against 36.5 KiB unaliased: six blocks per CU, not
// four).

// block sizes and prefetch of the residual tiles' two phases (qc_unit_blocks)
template <int N> constexpr int QC_POST6_UB_A = qc_post_ub_a(N);
template <int N> constexpr bool QC_POST6_PF_A = qc_post_pf(N);
// (phase B in blocks of 2 needs 16 more vector registers at n = 4, 90 against 74, which costs a resident block per CU:
// it keeps one unit per block, whose W3 row, b3 and W4 arrive behind one wait.  A prefetch of the next unit buys nothing
// there: the compiler sinks the request below the row stores of the body's second basic block, next to its wait.)
template <int N> constexpr int QC_POST6_UB_B = 1;
template <int N> constexpr bool QC_POST6_PF_B = false;

// DATA: target from tg[p], residual with the zeroth-order term c_u u; the point then has a cotangent c_u gsc on u
// itself, carried through expand_ub, the b4 column of the tile row and the out_u scratch.
// COEF (with DATA): the point's own operator row coef[k][p] (see k_post_body), loaded ahead of phase A; u is known
// before phase B, so the cubic term only changes the residual and ub0.  out_u receives the six channel cotangents [6][B].
// LEARN (with DATA): the COEF arithmetic on the uniform c_k of `lr` (learn_coefs), and seven more reductions on wave 0 for
// their gradient columns (learn_columns).  OPC below: either of the two.
// BAL (with DATA): see bal_weights; the tile zeroes the three columns of its row.
template <int N, bool DATA = false, bool COEF = false, bool LEARN = false, bool BAL = false>
__device__ __forceinline__ void k_post_fused6_body(const int64_t bid, const float* __restrict__ X, const float* __restrict__ prm,
                                                    QcLayout L, QcPde pde, const float* __restrict__ qjets,
                                                    float* __restrict__ out_u, float* __restrict__ out_res,
                                                    float* __restrict__ qbar, float* __restrict__ part, int64_t part_stride,
                                                    int64_t row0, int64_t B, float* __restrict__ s_dyn,
                                                    const float* __restrict__ tg = nullptr, const float c_u = 0.f,
                                                    const float* __restrict__ coef = nullptr, const QcLearn* lr = nullptr,
                                                    const QcBal* bl = nullptr) {
  static_assert(!COEF || DATA, "per-point operators: tabulated targets only");
  static_assert(!LEARN || (DATA && !COEF), "learned operators: tabulated targets, no table");
  static_assert(!BAL || (DATA && !COEF && !LEARN), "balanced weights: the tabulated kind's operator");
  constexpr bool OPC = COEF || LEARN;
  constexpr int NCH = 6;
  float* s_z = s_dyn;                                                        // [H][64]
  float (*s_u)[NCH][64] = reinterpret_cast<float (*)[NCH][64]>(s_dyn + L.H * 64);   // [QC_MS][NCH][64]
  float (*s_q)[NCH * N][64] = reinterpret_cast<float (*)[NCH * N][64]>(s_dyn);      // [QC_MS][NCH * N][64], after phase B
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = bid;
  const int64_t p = tile * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  mf2 q2[3][N];
#pragma unroll
  for (int cp = 0; cp < 3; ++cp)
#pragma unroll
    for (int i = 0; i < N; ++i)
      q2[cp][i] = (mf2){qjets[((int64_t)(2 * cp) * N + i) * B + pc], qjets[((int64_t)(2 * cp + 1) * N + i) * B + pc]};
  float cf[OPC ? QC_COEF_N : 1];   // seven coalesced loads, first used after phase A
  if constexpr (COEF) {
#pragma unroll
    for (int k = 0; k < QC_COEF_N; ++k) cf[k] = coef[(int64_t)k * B + pc];
  }
  const float* W3 = prm + L.oW3;
  const float* b3 = prm + L.ob3;
  const float* W4 = prm + L.oW4;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  const int m0 = wave * hq, m1 = (m0 + hq) < L.H ? (m0 + hq) : L.H;
  auto preact = [&](const float (&w3)[N], const float b3m, mf2 (&g2)[3]) {
    g2[0] = (mf2){b3m, 0.f};
    g2[1] = g2[2] = (mf2){0.f, 0.f};
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const mf2 w = m_dup(w3[i]);
#pragma unroll
      for (int cp = 0; cp < 3; ++cp) g2[cp] = m_fma(w, q2[cp][i], g2[cp]);
    }
  };
  auto load_blk = [&](auto& w, const int m) {
    post_blk_load<N, std::remove_reference_t<decltype(w)>::count>(w, W3, b3, W4, m);
  };
  // ---------------- phase A
  float u[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) u[c] = 0.f;
  qc_unit_blocks<QcPostW<N>, QC_POST6_UB_A<N>, QC_POST6_PF_A<N>>(m0, m1, load_blk, [&](const auto& w, const int m) {
    constexpr int K = std::remove_reference_t<decltype(w)>::count;
    mf2 g2[K][3];
    float z[K];
#pragma unroll
    for (int j = 0; j < K; ++j) preact(w.w3[j], w.b3[j], g2[j]);
#pragma unroll
    for (int j = 0; j < K; ++j) z[j] = qc_tanh(g2[j][0].x);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      s_z[(m + j) * 64 + lane] = z[j];
      const float w4 = w.w4[j];
      const float d1 = 1.f - z[j] * z[j], d2 = -2.f * z[j] * d1;
      u[0] = fmaf(w4, z[j], u[0]);
      u[1] = fmaf(w4, d1 * g2[j][0].y, u[1]);
      u[2] = fmaf(w4, d1 * g2[j][1].x, u[2]);
      u[3] = fmaf(w4, d1 * g2[j][1].y, u[3]);
      u[4] = fmaf(w4, d2 * g2[j][1].x * g2[j][1].x + d1 * g2[j][2].x, u[4]);
      u[5] = fmaf(w4, d2 * g2[j][1].y * g2[j][1].y + d1 * g2[j][2].y, u[5]);
    }
  });
#pragma unroll
  for (int c = 0; c < NCH; ++c) s_u[wave][c][lane] = u[c];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    u[c] = (s_u[0][c][lane] + s_u[1][c][lane]) + (s_u[2][c][lane] + s_u[3][c][lane]);
  u[0] += prm[L.ob4];
  // ---------------- residual / error / loss sums / per-point cotangent
  float* row = part + (row0 + tile) * part_stride;
  float lscale[LEARN ? QC_COEF_N : 1];
  int lz = 0;
  if constexpr (LEARN) {   // uniform: scalar loads, first needed here
    float lbase[QC_COEF_N];
    lz = learn_late();
    learn_read(lr, lz, lbase, lscale);
    learn_coefs(cf, prm, L, lbase, lscale);
  }
  float res;
  if constexpr (OPC) {
    res = cf[1] * u[1] + cf[2] * u[2] + cf[3] * u[3] - (cf[4] * u[4] + cf[5] * u[5]);
    res = fmaf(fmaf(cf[6] * u[0], u[0], cf[0]), u[0], res);
  } else {
    res = pde.c_t * u[1] + pde.c_x * u[2] + pde.c_y * u[3] - (pde.d_xx * u[4] + pde.d_yy * u[5]);
  }
  float target;
  if constexpr (DATA) {
    if constexpr (!OPC) res = fmaf(c_u, u[0], res);
    target = tg[pc];
  } else {
    const float t = X[pc * 3 + 0], x = X[pc * 3 + 1], y = X[pc * 3 + 2];
    target = residual_target(pde, t, x, y);
  }
  if constexpr (BAL) bal_weights<6>(pde, prm, L, bl);
  const float e = live ? res - target : 0.f;
  const float gsc = pde.w_res * e;
  // analytic problems: the loss sees u only through its derivatives
  float ub0 = DATA ? c_u * gsc : 0.f;
  if constexpr (OPC) ub0 = fmaf(3.f * cf[6] * u[0], u[0], cf[0]) * gsc;
  if (wave == 0) {
    const float ls = qc_wave_sum_to_lane63(e * e * pde.inv_n_res);
    float sb4 = 0.f;      // d loss / d b4 = sum of the points' cotangents of u
    if constexpr (DATA) sb4 = qc_wave_sum_to_lane63(ub0);
    if (lane == 63) {
      row[L.NP + 0] = ls;
      row[L.NP + 1] = 0.f;
      row[L.NP + 2] = 0.f;
      row[L.ob4] = sb4;
      if constexpr (BAL) bal_zero_columns(row, L);
    }
    if constexpr (LEARN) learn_columns(row, L, lr, lz, lscale, cf, gsc, u, lane, tile == 0);
    if constexpr (OPC) {
      if (live) {           // the six channel cotangents (qc_post_coef)
        out_u[p] = ub0;
        out_u[B + p] = gsc * cf[1];
        out_u[2 * B + p] = gsc * cf[2];
        out_u[3 * B + p] = gsc * cf[3];
        out_u[4 * B + p] = -cf[4] * gsc;
        out_u[5 * B + p] = -cf[5] * gsc;
      }
    } else if (live) {    // the per-point cotangents (MODE 2 contract of qc_post)
      out_u[p] = ub0;
      out_res[p] = gsc;
    }
  }
  // ---------------- phase B
  float ub[NCH];
  if constexpr (OPC) {
    ub[0] = ub0; ub[1] = gsc * cf[1]; ub[2] = gsc * cf[2]; ub[3] = gsc * cf[3]; ub[4] = -cf[4] * gsc; ub[5] = -cf[5] * gsc;
  } else {
    expand_ub<NCH>(ub, ub0, gsc, pde);
  }
  mf2 qb2[3][N];
#pragma unroll
  for (int cp = 0; cp < 3; ++cp)
#pragma unroll
    for (int i = 0; i < N; ++i) qb2[cp][i] = (mf2){0.f, 0.f};
  // the K units' weight-gradient reductions run as one merged reduction (same tree for every value)
  const QcPostCols<N, QC_POST6_UB_B<N>> cols(L, lane);
  qc_unit_blocks<QcPostW<N>, QC_POST6_UB_B<N>, QC_POST6_PF_B<N>>(m0, m1, load_blk, [&](const auto& w, const int m) {
    constexpr int K = std::remove_reference_t<decltype(w)>::count;
    float wg[K * (N + 2)];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      mf2 g2[3];
      preact(w.w3[j], w.b3[j], g2);
      const float g[NCH] = {0.f, g2[0].y, g2[1].x, g2[1].y, g2[2].x, g2[2].y};
      const float z = s_z[(m + j) * 64 + lane];
      float gb[NCH], gw4;
      post_cotangents<N, NCH>(gb, gw4, g, ub, z, w.w4[j]);
      const mf2 gb2[3] = {(mf2){gb[0], gb[1]}, (mf2){gb[2], gb[3]}, (mf2){gb[4], gb[5]}};
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const mf2 w3 = m_dup(w.w3[j][i]);
        mf2 acc = gb2[0] * q2[0][i];
#pragma unroll
        for (int cp = 0; cp < 3; ++cp) {
          qb2[cp][i] = m_fma(w3, gb2[cp], qb2[cp][i]);
          if (cp > 0) acc = m_fma(gb2[cp], q2[cp][i], acc);
        }
        wg[j * (N + 2) + i] = acc.x + acc.y;
      }
      wg[j * (N + 2) + N] = gb[0];
      wg[j * (N + 2) + N + 1] = gw4;
    }
    qc_wave_sum_merged<K * (N + 2)>(wg);
    cols.template store<K>(row, L, wg, m, lane);
  });
  __syncthreads();   // every wave is done with s_z and s_u: the qbar partials overwrite them
#pragma unroll
  for (int cp = 0; cp < 3; ++cp)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      s_q[wave][(2 * cp) * N + i][lane] = qb2[cp][i].x;
      s_q[wave][(2 * cp + 1) * N + i][lane] = qb2[cp][i].y;
    }
  __syncthreads();
  if (live) {
    // compile-time trip count (n <= 8): every LDS read of the wave's rows is in flight before the first sum
    constexpr int NF = (NCH * N + QC_MS - 1) / QC_MS;
    if constexpr (NF <= 12) {
      float v[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int f = wave + QC_MS * j, fc = f < NCH * N ? f : 0;
        v[j] = (s_q[0][fc][lane] + s_q[1][fc][lane]) + (s_q[2][fc][lane] + s_q[3][fc][lane]);
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int f = wave + QC_MS * j;
        if (f < NCH * N) qc_store_wt(&qbar[(int64_t)f * B + p], v[j]);
      }
    } else {
      for (int f = wave; f < NCH * N; f += QC_MS)
        qc_store_wt(&qbar[(int64_t)f * B + p], (s_q[0][f][lane] + s_q[1][f][lane]) + (s_q[2][f][lane] + s_q[3][f][lane]));
    }
  }
}

// hidden widths the fused post kernel parks tanh values for (LDS: H x 64 floats per residual tile)
constexpr int QC_POST_FUSED_MAXH = 128;

// dynamic LDS bytes of the fused post kernels: residual tiles (k_post_fused6_body), value tiles (k_post_fused_value_body)
static inline size_t qc_post_fused_lds_res(const QcLayout& L) {
  const int a = L.H * 64 + QC_MS * 6 * 64, b = QC_MS * 6 * L.n * 64;
  return (size_t)(a > b ? a : b) * sizeof(float);
}
static inline size_t qc_post_fused_lds_val(const QcLayout& L) {
  return (size_t)QC_POST_VALUE_TPB * (L.H + QC_MS / QC_POST_VALUE_TPB) * 64 * sizeof(float);
}

template <int N, int NCH, class... TG>
__global__ void __launch_bounds__(256) k_post_fused(const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                                                    QcPde pde, const float* __restrict__ qjets, float* __restrict__ out_u,
                                                    float* __restrict__ out_res, float* __restrict__ qbar,
                                                    float* __restrict__ part, int64_t part_stride, int64_t row0, int64_t B,
                                                    TG... tg) {
  extern __shared__ float s_dyn[];
  using K = QcKind<TG...>;
  if constexpr (NCH == 6)
    k_post_fused6_body<N, K::data, K::coef, K::learn, K::bal>(blockIdx.x, X, prm, L, pde, qjets, out_u, out_res, qbar, part,
                                                              part_stride, row0, B, s_dyn, K::tg_res(tg...), K::c_u(tg...),
                                                              K::table(tg...), K::op(tg...), K::weights(tg...));
  else
    k_post_fused_value_body<N, QC_POST_VALUE_TPB, K::data, K::learn, K::bal>(blockIdx.x, X, prm, L, pde, qjets, out_u, qbar, part,
                                                                             part_stride, row0, B, s_dyn, K::tg_val(tg...),
                                                                             K::weights(tg...));
}

// ================================================================== K outputs behind one shared network (Navier-Stokes)
// A K-output post network Linear(n, H) -> Tanh -> Linear(H, K) (reference nn/pde.py:2-27 differentiates (u, v, p) of ONE
// model) shares pre network, circuit and the hidden layer; only the last layer has a row per output.  The six
// derivative channels of all K outputs come from one pass: f_c(m) (the hidden unit's channel values) is formed once,
// u_k,c = sum_m W4[k][m] f_c(m).  w4k = [K][H + 1] rows (W4[k][0..H-1], b4[k]); the W4 / b4 slots of the flat vector
// are not read.  MODE 4: forward, out = [K][6][B].  MODE 3: reverse, ubar = [K][6][B] -> qbar [6][n][B], the tile's row
// of the shared parameters (W3, b3) in `part` and of the last layer in `partk` ([rows][K * (H + 1)]).  lane = point;
// weight gradients by wave reductions as in k_post_fused6_body.
constexpr int QC_KMAX = 4;

template <int N, int MODE>
__global__ void __launch_bounds__(256) k_post_multi(const float* __restrict__ prm, QcLayout L, int K,
                                                    const float* __restrict__ w4k, const float* __restrict__ qjets,
                                                    float* __restrict__ out_u, const float* __restrict__ ubar,
                                                    float* __restrict__ qbar, float* __restrict__ part, int64_t part_stride,
                                                    float* __restrict__ partk, int64_t partk_stride, int64_t row0, int64_t B) {
  constexpr int NCH = 6;
  __shared__ float s_buf[QC_MS][NCH * (N > QC_KMAX ? N : QC_KMAX)][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = blockIdx.x;
  const int64_t p = tile * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  float q[NCH][N];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) q[c][i] = qjets[((int64_t)c * N + i) * B + pc];
  const float* W3 = prm + L.oW3;
  const float* b3 = prm + L.ob3;
  const int H1 = L.H + 1;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  const int m0 = wave * hq, m1 = (m0 + hq) < L.H ? (m0 + hq) : L.H;
  auto hidden = [&](int m, float (&g)[NCH], float& z, float (&f)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      float sum = (c == 0) ? b3[m] : 0.f;
#pragma unroll
      for (int i = 0; i < N; ++i) sum = fmaf(W3[m * N + i], q[c][i], sum);
      g[c] = sum;
    }
    z = qc_tanh(g[0]);
    const float d1 = 1.f - z * z, d2 = -2.f * z * d1;
    f[0] = z;
    f[1] = d1 * g[1];
    f[2] = d1 * g[2];
    f[3] = d1 * g[3];
    f[4] = d2 * g[2] * g[2] + d1 * g[4];
    f[5] = d2 * g[3] * g[3] + d1 * g[5];
  };
  if constexpr (MODE == 4) {
    float u[QC_KMAX][NCH];
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k)
#pragma unroll
      for (int c = 0; c < NCH; ++c) u[k][c] = 0.f;
    for (int m = m0; m < m1; ++m) {
      float g[NCH], z, f[NCH];
      hidden(m, g, z, f);
#pragma unroll
      for (int k = 0; k < QC_KMAX; ++k)
        if (k < K) {
          const float w4 = w4k[k * H1 + m];
#pragma unroll
          for (int c = 0; c < NCH; ++c) u[k][c] = fmaf(w4, f[c], u[k][c]);
        }
    }
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k)
#pragma unroll
      for (int c = 0; c < NCH; ++c) s_buf[wave][k * NCH + c][lane] = u[k][c];
    __syncthreads();
    if (live) {
      for (int f = wave; f < K * NCH; f += QC_MS) {
        float v = (s_buf[0][f][lane] + s_buf[1][f][lane]) + (s_buf[2][f][lane] + s_buf[3][f][lane]);
        if (f % NCH == 0) v += w4k[(f / NCH) * H1 + L.H];
        out_u[(int64_t)f * B + p] = v;
      }
    }
  } else {
    float ub[QC_KMAX][NCH];
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k)
#pragma unroll
      for (int c = 0; c < NCH; ++c) ub[k][c] = (live && k < K) ? ubar[((int64_t)k * NCH + c) * B + pc] : 0.f;
    float* row = part + (row0 + tile) * part_stride;
    float* rowk = partk + (row0 + tile) * partk_stride;
    if (wave == 0) {   // d / d b4[k] = sum of the points' cotangents of u_k
#pragma unroll
      for (int k = 0; k < QC_KMAX; ++k)
        if (k < K) {
          const float sb = qc_wave_sum_to_lane63(ub[k][0]);
          if (lane == 63) rowk[k * H1 + L.H] = sb;
        }
    }
    float qb[NCH][N];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < N; ++i) qb[c][i] = 0.f;
    for (int m = m0; m < m1; ++m) {
      float g[NCH], z, f[NCH];
      hidden(m, g, z, f);
      float ubw[NCH], gk[QC_KMAX];
#pragma unroll
      for (int c = 0; c < NCH; ++c) ubw[c] = 0.f;
#pragma unroll
      for (int k = 0; k < QC_KMAX; ++k) {
        gk[k] = 0.f;
        if (k < K) {
          const float w4 = w4k[k * H1 + m];
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            ubw[c] = fmaf(w4, ub[k][c], ubw[c]);
            gk[k] = fmaf(ub[k][c], f[c], gk[k]);
          }
        }
      }
      float gb[NCH], gw4;
      post_cotangents<N, NCH>(gb, gw4, g, ubw, z, 1.f);
      float wg[N + 1];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float w3 = W3[m * N + i];
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          qb[c][i] = fmaf(w3, gb[c], qb[c][i]);
          sum = fmaf(gb[c], q[c][i], sum);
        }
        wg[i] = sum;
      }
      wg[N] = gb[0];
      qc_wave_sum_merged<N + 1>(wg);
      post_store_w3b3<N>(row, L, wg, m, lane);
#pragma unroll
      for (int k = 0; k < QC_KMAX; ++k)
        if (k < K) gk[k] = qc_wave_sum_to_lane63(gk[k]);
      if (lane == 63) {
#pragma unroll
        for (int k = 0; k < QC_KMAX; ++k)
          if (k < K) rowk[k * H1 + m] = gk[k];
      }
    }
    if (threadIdx.x == 0) {   // the single-output slots of the flat layout are not parameters here
      for (int m = 0; m < L.H; ++m) row[L.oW4 + m] = 0.f;
      row[L.ob4] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < N; ++i) s_buf[wave][c * N + i][lane] = qb[c][i];
    __syncthreads();
    if (live) {
      for (int f = wave; f < NCH * N; f += QC_MS)
        qbar[(int64_t)f * B + p] = (s_buf[0][f][lane] + s_buf[1][f][lane]) + (s_buf[2][f][lane] + s_buf[3][f][lane]);
    }
  }
}

// ================================================================== residual + value tiles in ONE launch
// The fused step's two pipelines (65 536 residual points with 6 channels, 2 x 21 845 boundary / initial points with
// the value channel) are independent until the row reduction.  Launching each stage once over the blocks of BOTH
// (the lighter value tiles first, so the launch ends on full-occupancy residual tiles; block-uniform branch) removes the side stream, its two
// cross-queue event waits (~7 us of idle queue each) and 6 of the step's 15 launches.
// MAP: output map of the pre network (see angle_map_fwd); RF: boundary points on a random face (qc_philox.h)
template <int N, int MAP, bool RF>
__global__ void __launch_bounds__(256) k_pre_fwd_both(float* __restrict__ Xr, float* __restrict__ Xv,
                                                      const float* __restrict__ prm, QcLayout L, float* __restrict__ ajr,
                                                      float* __restrict__ ajv, int64_t Br, int64_t Bv, int n_val, QcDraw draw) {
  if ((int)blockIdx.x >= n_val) k_pre_fwd_body<N, 6, MAP>(blockIdx.x - n_val, Xr, prm, L, ajr, Br, &draw, Xr);
  else k_pre_fwd_value4<N, MAP, RF>(blockIdx.x, Xv, prm, L, ajv, Bv, &draw, Xv);
}

// ajr / ajv: the angle jets the forward stage wrote (read with MAP = 1 only)
template <int N, int MAP>
__global__ void k_pre_bwd_both(const float* __restrict__ Xr, const float* __restrict__ Xv, const float* __restrict__ prm,
                               QcLayout L, const float* __restrict__ abr, const float* __restrict__ abv,
                               float* __restrict__ part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br,
                               int64_t Bv, int HB, int PS, int n_val, const float* __restrict__ ajr,
                               const float* __restrict__ ajv) {
  if ((int)blockIdx.x >= n_val)
    k_pre_bwd_body<N, 6, MAP>(blockIdx.x - n_val, Xr, prm, L, abr, part, part_stride, row0_r, Br, HB, PS, ajr);
  else k_pre_bwd_body<N, 1, MAP>(blockIdx.x, Xv, prm, L, abv, part, part_stride, row0_v, Bv, HB, PS, ajv);
}

struct QcPostSeg {   // one pipeline's arguments of the fused (mode 2) post kernels
  const float* X;
  const float* qjets;
  float* ub;       // per-point cotangent of u (scratch, B floats)
  float* rb;       // per-point cotangent of the residual (scratch, B floats; residual pipeline only)
  float* qbar;
  int64_t row0, B;
};

// The merged point kernels by target kind (QcKind).  With a coefficient table: residual tiles on the COEF bodies (r.ub =
// the [6][B] cotangent scratch, r.rb unused), value tiles on the DATA code.
template <int N, class... TG>
__global__ void __launch_bounds__(256) k_post_both(const float* __restrict__ prm, QcLayout L, QcPde pde, QcPostSeg r,
                                                   QcPostSeg v, float* __restrict__ part, int64_t part_stride,
                                                   int n_val, TG... tg) {
  using K = QcKind<TG...>;
  if ((int)blockIdx.x >= n_val)
    k_post_body<N, 6, 2, K::data, K::coef, K::learn, K::bal>(blockIdx.x - n_val, r.X, prm, L, pde, r.qjets, r.ub, r.rb, nullptr,
                                                             nullptr, r.qbar, part, part_stride, r.row0, r.B, K::tg_res(tg...),
                                                             K::c_u(tg...), K::table(tg...), K::op(tg...), K::weights(tg...));
  else
    k_post_value4<N, K::data, K::learn, K::bal>(blockIdx.x, v.X, prm, L, pde, v.qjets, v.ub, v.qbar, part, part_stride, v.row0,
                                                v.B, K::tg_val(tg...), K::weights(tg...));
}

// fused post stage: here the residual tiles come first and the (shorter) value blocks fill the slots after them
template <int N, class... TG>
__global__ void __launch_bounds__(256) k_post_fused_both(const float* __restrict__ prm, QcLayout L, QcPde pde, QcPostSeg r,
                                                         QcPostSeg v, float* __restrict__ part, int64_t part_stride,
                                                         int n_res, TG... tg) {
  extern __shared__ float s_dyn[];
  using K = QcKind<TG...>;
  if ((int)blockIdx.x < n_res)
    k_post_fused6_body<N, K::data, K::coef, K::learn, K::bal>(blockIdx.x, r.X, prm, L, pde, r.qjets, r.ub, r.rb, r.qbar, part,
                                                              part_stride, r.row0, r.B, s_dyn, K::tg_res(tg...), K::c_u(tg...),
                                                              K::table(tg...), K::op(tg...), K::weights(tg...));
  else
    k_post_fused_value_body<N, QC_POST_VALUE_TPB, K::data, K::learn, K::bal>(blockIdx.x - n_res, v.X, prm, L, pde, v.qjets, v.ub,
                                                                             v.qbar, part, part_stride, v.row0, v.B, s_dyn,
                                                                             K::tg_val(tg...), K::weights(tg...));
}

// GEN (the coefficient step and the inverse step): the residual tiles read their six channel cotangents from r.ub (gen mode of the body)
template <int N, bool GEN>
__global__ void k_post_wg_both(const float* __restrict__ prm, QcLayout L, QcPde pde, QcPostSeg r, QcPostSeg v,
                               float* __restrict__ part, int64_t part_stride, int HB, int PS, int n_val) {
  if ((int)blockIdx.x >= n_val)
    k_post_wg_body<N, 6>(blockIdx.x - n_val, prm, L, pde, r.qjets, r.ub, GEN ? nullptr : r.rb, part, part_stride, r.row0, r.B,
                         HB, PS, GEN ? 1 : 0);
  else
    k_post_wg_body<N, 1>(blockIdx.x, prm, L, pde, v.qjets, v.ub, nullptr, part, part_stride, v.row0, v.B, HB, PS);
}

}  // namespace

// ------------------------------------------------------------------ launchers
// The wire count as a compile-time value: f(qc_int<N>) for the N in LO .. HI that equals n, QC_ERR_UNSUPPORTED outside.
// The range is the set of instantiations a launcher builds.  It is walked from HI down: the compiler emits the kernels of
// the calls it meets last first, so the code object holds them in ascending N, as it always has (where identical kernels
// lie is worth 0.5 % of the step at config 2: DESIGN.md, "Target kinds").
template <int V> using qc_int = std::integral_constant<int, V>;
template <int LO, class F, int... I>
static inline int qc_dispatch_seq(const int n, F&& f, std::integer_sequence<int, I...>) {
  constexpr int HI = LO + (int)sizeof...(I) - 1;
  const bool hit = ((n == HI - I ? (f(qc_int<HI - I>{}), true) : false) || ...);
  return hit ? QC_OK : QC_ERR_UNSUPPORTED;
}
template <int LO, int HI, class F>
static inline int qc_dispatch_n(const int n, F&& f) {
  return qc_dispatch_seq<LO>(n, f, std::make_integer_sequence<int, HI - LO + 1>{});
}
constexpr int QC_MLP_NMAX = 16;   // every kernel of this file exists for n = 1 .. 16

// lane = hidden unit kernels: HB lanes per group (one per hidden unit), PS groups share the tile's 64
// points.  Narrow hidden layers pack groups back to back (HB = H: 5 groups of 50 fill 250 of 256 lanes
// instead of 4 x 64 with 14 idle lanes each); the block is rounded up to whole waves.  Target block size 256
// (QC_MLP_THREADS): the 1 708 tiles of BASELINE config 2 are then resident in one round of 8 blocks per CU (512: 1.7
// rounds of 4; measured 15.3 against 16.4 us for the stage; 128 / 192 / 320 / 384 / 768 / 1024: 17.3 .. 24.4).
static inline void hidden_geometry(int H, int* HB, int* PS, int* threads) {
  static const int target = [] { const char* e = getenv("QC_MLP_THREADS"); const int v = e ? atoi(e) : 0; return v >= 64 && v <= 1024 ? v : 256; }();
  if (H <= target) {
    *HB = H;
    int ps = target / H;
    *PS = ps > 64 ? 64 : ps;
  } else {
    *HB = 64 * qc_ceil_div(H, 64);
    int ps = 1024 / *HB;
    *PS = ps >= 4 ? 4 : (ps >= 2 ? 2 : 1);
  }
  *threads = 64 * qc_ceil_div(*HB * *PS, 64);
}

static inline bool post_fused_ok(const QcLayout& L) {
  static const bool split = [] { const char* e = getenv("QC_POST_SPLIT"); return e && e[0] == '1'; }();
  return !split && L.H <= QC_POST_FUSED_MAXH;
}

int qc_mlp_pre_fwd(const float* X, const float* prm, QcLayout L, float* ajets, int64_t B, int nch,
                   hipStream_t st, int map) {
  const int grid = qc_ceil_div(B, 64);
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto c, auto m) {
      hipLaunchKernelGGL((k_pre_fwd<n(), c(), m()>), dim3(grid), dim3(256), 0, st, X, prm, L, ajets, B);
    };
    if (map) { if (nch == 6) launch(qc_int<6>{}, qc_int<1>{}); else launch(qc_int<1>{}, qc_int<1>{}); }
    else if (nch == 6) launch(qc_int<6>{}, qc_int<0>{});
    else launch(qc_int<1>{}, qc_int<0>{});
  });
}

int qc_mlp_pre_bwd(const float* X, const float* prm, QcLayout L, const float* abar, float* part,
                   int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t st, int map, const float* aj) {
  const int grid = qc_ceil_div(B, 64);
  if (L.H > 1024 || L.n > 64) return QC_ERR_UNSUPPORTED;
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (4 + L.n) * HB * sizeof(float);
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto c, auto m) {
      hipLaunchKernelGGL((k_pre_bwd<n(), c(), m()>), dim3(grid), dim3(threads), sh, st, X, prm, L, abar, part, part_stride,
                         row0, B, HB, PS, aj);
    };
    if (map) { if (nch == 6) launch(qc_int<6>{}, qc_int<1>{}); else launch(qc_int<1>{}, qc_int<1>{}); }
    else if (nch == 6) launch(qc_int<6>{}, qc_int<0>{});
    else launch(qc_int<1>{}, qc_int<0>{});
  });
}

// The mode as a compile-time value, for the instantiations that exist: modes 3 and 4 with six channels only, and with a
// target argument mode 2 only.
template <int NCH, bool DATA, class F>
static inline void qc_post_mode(const int mode, F&& f) {
  if constexpr (!DATA) {
    if (mode == 0) return f(qc_int<0>{});
    if (mode == 1) return f(qc_int<1>{});
    if constexpr (NCH == 6) {
      if (mode == 3) return f(qc_int<3>{});
      if (mode == 4) return f(qc_int<4>{});
    }
  }
  f(qc_int<2>{});
}

// the learned-operator kind of both post launchers: defined at the end of this file, so that its instantiations lie behind
// every other kernel of the code object (see qc_dispatch_seq)
static int post_learn(const float* prm, QcLayout L, QcPde pde, const float* qjets, float* out_u, float* qbar, float* part,
                      int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t st, const QcTarget& tg);
static int post_both_learn(const float* prm, QcLayout L, QcPde pde, const QcPostSeg& r, const QcPostSeg& v, float* part,
                           int64_t part_stride, hipStream_t st, const QcTarget& tg);
// the balanced kind of both, behind those
static int post_bal(const float* prm, QcLayout L, QcPde pde, const float* qjets, float* out_u, float* out_res, float* qbar,
                    float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t st, const QcTarget& tg);
static int post_both_bal(const float* prm, QcLayout L, QcPde pde, const QcPostSeg& r, const QcPostSeg& v, float* part,
                         int64_t part_stride, hipStream_t st, const QcTarget& tg);

int qc_mlp_post(int mode, const float* X, const float* prm, QcLayout L, QcPde pde, const float* qjets,
                float* out_u, float* out_res, const float* in_ubar, const float* in_rbar, float* qbar,
                float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t st, const QcTarget& tg) {
  if (L.H > 1024) return QC_ERR_UNSUPPORTED;
  if (!tg.ok(mode, nch, pde.problem)) return QC_ERR_ARG;
  if (tg.kind == QC_TARGET_LEARN) return post_learn(prm, L, pde, qjets, out_u, qbar, part, part_stride, row0, B, nch, st, tg);
  if (tg.kind == QC_TARGET_BAL) return post_bal(prm, L, pde, qjets, out_u, out_res, qbar, part, part_stride, row0, B, nch, st, tg);
  const int tiles = qc_ceil_div(B, 64);
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (L.n + 2) * HB * sizeof(float);
  // cotangent sources of the weight-gradient kernel: given (modes 1, 3) or produced by the point kernel (mode 2); one
  // per derivative channel (its gen mode) in mode 3 and behind the point kernel of a coefficient table
  const float* ub_src = (mode == 1 || mode == 3) ? in_ubar : out_u;
  const float* rb_src = mode == 1 ? in_rbar : (tg.kind == QC_TARGET_COEF ? nullptr : out_res);
  const int gen = (mode == 3 || tg.kind == QC_TARGET_COEF) ? 1 : 0;
  // the step's form (mode 2): one kernel, lane = point in both phases; QC_POST_SPLIT=1 and wide hidden layers keep the pair
  const bool fused = mode == 2 && post_fused_ok(L);
  const size_t shr = qc_post_fused_lds_res(L), shv = qc_post_fused_lds_val(L);
  // the one launch sequence, for n wires, nch channels and the target arguments t (none: analytic)
  auto launch = [&](auto n, auto c, const auto&... t) {
    constexpr int N = n(), NCH = c();
    if (fused) {
      hipLaunchKernelGGL((k_post_fused<N, NCH, std::decay_t<decltype(t)>...>),
                         dim3(NCH == 6 ? tiles : qc_ceil_div(tiles, QC_POST_VALUE_TPB)), dim3(256), NCH == 6 ? shr : shv, st, X,
                         prm, L, pde, qjets, out_u, out_res, qbar, part, part_stride, row0, B, t...);
      return;
    }
    qc_post_mode<NCH, (sizeof...(t) > 0)>(mode, [&](auto m) {
      hipLaunchKernelGGL((k_post<N, NCH, m(), std::decay_t<decltype(t)>...>), dim3(tiles), dim3(256), 0, st, X, prm, L, pde,
                         qjets, out_u, out_res, in_ubar, in_rbar, qbar, part, part_stride, row0, B, t...);
    });
    if (mode >= 1 && mode <= 3)
      hipLaunchKernelGGL((k_post_wg<N, NCH>), dim3(tiles), dim3(threads), sh, st, prm, L, pde, qjets, ub_src,
                         (NCH == 6 ? rb_src : nullptr), part, part_stride, row0, B, HB, PS, gen);
  };
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto by_nch = [&](const auto&... t) {
      if (nch == 6) launch(n, qc_int<6>{}, t...);
      else launch(n, qc_int<1>{}, t...);
    };
    if (tg.kind == QC_TARGET_COEF) launch(n, qc_int<6>{}, tg.tab, tg.coef);   // residual points only (QcTarget::ok)
    else if (tg.kind == QC_TARGET_TAB) by_nch(tg.tab);
    else by_nch();
  });
}

// ------------------------------------------------------------------ merged residual + value launches (fused step)
// draw_*: when `draw` != 0 the launch first draws its own points (qc_sample_collocation_faces semantics) into Xr / Xv
int qc_mlp_pre_fwd_both(const QcBatches& b, int draw, int64_t face_pts, const float* prm, QcLayout L, float* ajr, float* ajv,
                        hipStream_t st, int map) {
  float *Xr = b.X_res, *Xv = b.X_val;
  const int64_t Br = b.n_res, Bv = b.n_ic + b.n_bc;
  const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(qc_ceil_div(Bv, 64), 4);   // value tiles: 4 per block, one per wave
  const QcDraw dr = {draw, b.n_ic, b.off_res, b.off_ic, b.off_bc, face_pts, b.seed, b.step};
  const bool rf = draw && face_pts < 0;
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto m, auto r) {
      hipLaunchKernelGGL((k_pre_fwd_both<n(), m(), r()>), dim3(nr + nv), dim3(256), 0, st, Xr, Xv, prm, L, ajr, ajv, Br, Bv, nv,
                         dr);
    };
    if (map) { if (rf) launch(qc_int<1>{}, std::true_type{}); else launch(qc_int<1>{}, std::false_type{}); }
    else if (rf) launch(qc_int<0>{}, std::true_type{});
    else launch(qc_int<0>{}, std::false_type{});
  });
}

int qc_mlp_pre_bwd_both(const float* Xr, const float* Xv, const float* prm, QcLayout L, const float* abr, const float* abv,
                        float* part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br, int64_t Bv,
                        hipStream_t st, int map, const float* ajr, const float* ajv) {
  if (L.H > 1024 || L.n > 64) return QC_ERR_UNSUPPORTED;
  const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 64);
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (4 + L.n) * HB * sizeof(float);
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto m) {
      hipLaunchKernelGGL((k_pre_bwd_both<n(), m()>), dim3(nr + nv), dim3(threads), sh, st, Xr, Xv, prm, L, abr, abv, part,
                         part_stride, row0_r, row0_v, Br, Bv, HB, PS, nv, ajr, ajv);
    };
    if (map) launch(qc_int<1>{}); else launch(qc_int<0>{});
  });
}

// mode-2 post stage of both pipelines: the fused kernel, or point kernel and weight-gradient kernel
int qc_mlp_post_both(const float* prm, QcLayout L, QcPde pde, const float* Xr, const float* qjr, float* ubr, float* rbr,
                     float* qbr, int64_t row0_r, int64_t Br, const float* Xv, const float* qjv, float* ubv, float* qbv,
                     int64_t row0_v, int64_t Bv, float* part, int64_t part_stride, hipStream_t st, const QcTarget& tg) {
  if (L.H > 1024) return QC_ERR_UNSUPPORTED;
  if (!tg.ok(2, 6, pde.problem)) return QC_ERR_ARG;
  if (tg.kind == QC_TARGET_LEARN)
    return post_both_learn(prm, L, pde, QcPostSeg{Xr, qjr, ubr, rbr, qbr, row0_r, Br}, QcPostSeg{Xv, qjv, ubv, nullptr, qbv, row0_v, Bv},
                           part, part_stride, st, tg);
  if (tg.kind == QC_TARGET_BAL)
    return post_both_bal(prm, L, pde, QcPostSeg{Xr, qjr, ubr, rbr, qbr, row0_r, Br}, QcPostSeg{Xv, qjv, ubv, nullptr, qbv, row0_v, Bv},
                         part, part_stride, st, tg);
  const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 64);
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (L.n + 2) * HB * sizeof(float);
  const int nv4 = qc_ceil_div(nv, 4);   // point kernel: 4 value tiles per block, one per wave
  // (with a coefficient table ubr is the [6][Br] cotangent scratch of the residual tiles)
  const QcPostSeg r = {Xr, qjr, ubr, rbr, qbr, row0_r, Br}, v = {Xv, qjv, ubv, nullptr, qbv, row0_v, Bv};
  const bool fused = post_fused_ok(L);
  // fused: residual blocks, then value blocks of QC_POST_VALUE_TPB tiles; one dynamic LDS size serves both bodies
  const int nvf = qc_ceil_div(nv, QC_POST_VALUE_TPB);
  const size_t shr = qc_post_fused_lds_res(L), shv = qc_post_fused_lds_val(L), shf = shr > shv ? shr : shv;
  // the one launch sequence, for n wires and the target arguments t (none: analytic)
  auto launch = [&](auto n, const auto&... t) {
    constexpr int N = n();
    if (fused) {
      hipLaunchKernelGGL((k_post_fused_both<N, std::decay_t<decltype(t)>...>), dim3(nr + nvf), dim3(256), shf, st, prm, L, pde,
                         r, v, part, part_stride, nr, t...);
    } else {
      hipLaunchKernelGGL((k_post_both<N, std::decay_t<decltype(t)>...>), dim3(nr + nv4), dim3(256), 0, st, prm, L, pde, r, v,
                         part, part_stride, nv4, t...);
      hipLaunchKernelGGL((k_post_wg_both<N, QcKind<std::decay_t<decltype(t)>...>::coef>), dim3(nr + nv), dim3(threads), sh, st,
                         prm, L, pde, r, v, part, part_stride, HB, PS, nv);
    }
  };
  // the merged form exists for the register family only (n = 2 .. 5), so the kernels of the youngest kind are built for
  // those widths alone (the weight-gradient kernel would need scratch memory from n = 13)
  if (tg.kind == QC_TARGET_COEF) return qc_dispatch_n<2, 5>(L.n, [&](auto n) { launch(n, tg.tab, tg.coef); });
  if (tg.kind == QC_TARGET_TAB) return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) { launch(n, tg.tab); });
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) { launch(n); });
}

// K-output post stage (k_post_multi): mode 4 forward / mode 3 reverse, six channels
int qc_mlp_post_multi(int mode, const float* prm, QcLayout L, int K, const float* w4k, const float* qjets, float* out_u,
                      const float* ubar, float* qbar, float* part, int64_t part_stride, float* partk, int64_t partk_stride,
                      int64_t row0, int64_t B, hipStream_t st) {
  if (K < 1 || K > QC_KMAX || L.H > 1024) return QC_ERR_UNSUPPORTED;
  const int tiles = qc_ceil_div(B, 64);
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto m) {
      hipLaunchKernelGGL((k_post_multi<n(), m()>), dim3(tiles), dim3(256), 0, st, prm, L, K, w4k, qjets, out_u, ubar, qbar, part,
                         part_stride, partk, partk_stride, row0, B);
    };
    if (mode == 4) launch(qc_int<4>{}); else launch(qc_int<3>{});
  });
}

// ================================================================== system post stage: K outputs, the operator as a term list
// The post stage of qc_fused_pinn_system_step (Navier-Stokes behind one shared network, nn/pde.py:2-27, and every system
// of that shape): ONE kernel per 64-point tile for the hidden layer, the K x NCH channels u[k][c], the residuals of the
// n_eq equations from the term list, the loss columns, the cotangents ub[k][c] (product rule over up to three factors)
// and the reverse pass of k_post_multi's mode 3, with the last layer's gradients in the flat row at oW4 + k H + m and
// ob4 + k of the K-row layout.  lane = point, the four waves split the hidden units.
// The term fields are wave-uniform run-time values: indexing the per-lane arrays u[k][c] / ub[k][c] by them would send
// the arrays to scratch memory.  After the cross-wave sum the channels lie in LDS in lane-private columns, so wave 0
// runs the term loop on LDS rows (s_buf[0]: u, s_buf[1]: ub) and every wave then loads ub with compile-time indices.
// NCH = 1 (value points): u_k = W4[k] z + b4[k] against tg[k][p], weighted by segment (IC below pde.n_seg_a) and w_out[k];
// no term list is read.  tg: [n_eq][B] (NCH = 6; null: zero) or [K][B] (NCH = 1).
template <int N, int NCH>
__global__ void __launch_bounds__(256) k_post_system(const float* __restrict__ prm, QcLayout L, QcSys sys, QcPde pde,
                                                     const float* __restrict__ qjets, const float* __restrict__ tg,
                                                     float* __restrict__ qbar, float* __restrict__ part, int64_t part_stride,
                                                     int64_t row0, int64_t B) {
  constexpr int ROWS = NCH * (N > QC_KMAX ? N : QC_KMAX);
  __shared__ float s_buf[QC_MS][ROWS][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = blockIdx.x;
  const int64_t p = tile * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  const int K = sys.K;
  float q[NCH][N];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) q[c][i] = qjets[((int64_t)c * N + i) * B + pc];
  const float* W3 = prm + L.oW3;
  const float* b3 = prm + L.ob3;
  const float* W4 = prm + L.oW4;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  const int m0 = wave * hq, m1 = (m0 + hq) < L.H ? (m0 + hq) : L.H;
  auto hidden = [&](int m, float (&g)[NCH], float& z, float (&f)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      float sum = (c == 0) ? b3[m] : 0.f;
#pragma unroll
      for (int i = 0; i < N; ++i) sum = fmaf(W3[m * N + i], q[c][i], sum);
      g[c] = sum;
    }
    z = qc_tanh(g[0]);
    f[0] = z;
    if constexpr (NCH == 6) {
      const float d1 = 1.f - z * z, d2 = -2.f * z * d1;
      f[1] = d1 * g[1];
      f[2] = d1 * g[2];
      f[3] = d1 * g[3];
      f[4] = d2 * g[2] * g[2] + d1 * g[4];
      f[5] = d2 * g[3] * g[3] + d1 * g[5];
    }
  };
  // ---- forward: this wave's share of u[k][c], then the sum over the waves
  {
    float u[QC_KMAX][NCH];
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k)
#pragma unroll
      for (int c = 0; c < NCH; ++c) u[k][c] = 0.f;
    for (int m = m0; m < m1; ++m) {
      float g[NCH], z, f[NCH];
      hidden(m, g, z, f);
#pragma unroll
      for (int k = 0; k < QC_KMAX; ++k)
        if (k < K) {
          const float w4 = W4[k * L.H + m];
#pragma unroll
          for (int c = 0; c < NCH; ++c) u[k][c] = fmaf(w4, f[c], u[k][c]);
        }
    }
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k)
#pragma unroll
      for (int c = 0; c < NCH; ++c) s_buf[wave][k * NCH + c][lane] = u[k][c];
  }
  __syncthreads();
  float* row = part + (row0 + tile) * part_stride;
  float ub[QC_KMAX][NCH];
  if constexpr (NCH == 1) {
    // every wave forms the K values and their cotangents itself (compile-time indices); wave 0 writes the columns
    const bool seg_a = p < pde.n_seg_a;
    const float wv = seg_a ? pde.w_val_a : pde.w_val_b;
    float la = 0.f, lb = 0.f;
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k) {
      ub[k][0] = 0.f;
      if (k < K) {
        const float uk = ((s_buf[0][k][lane] + s_buf[1][k][lane]) + (s_buf[2][k][lane] + s_buf[3][k][lane])) + prm[L.ob4 + k];
        const float e = live ? uk - tg[(int64_t)k * B + pc] : 0.f;
        const float we = sys.w_out[k] * e;
        ub[k][0] = wv * we;
        la += seg_a ? we * e * pde.inv_n_a : 0.f;
        lb += seg_a ? 0.f : we * e * pde.inv_n_b;
      }
    }
    if (wave == 0) {
      la = qc_wave_sum_to_lane63(la);
      lb = qc_wave_sum_to_lane63(lb);
      if (lane == 63) {
        row[L.NP + 0] = 0.f;
        row[L.NP + 1] = lb;  // column order: residual, BC, IC; segment a = IC, b = BC
        row[L.NP + 2] = la;
      }
    }
  } else {
    if (wave == 0) {
      // u[k][c] -> s_buf[0][k * 6 + c]; zeroed cotangents -> s_buf[1] (the other waves' partial sums are consumed here)
      for (int f = 0; f < K * NCH; ++f) {
        float v = (s_buf[0][f][lane] + s_buf[1][f][lane]) + (s_buf[2][f][lane] + s_buf[3][f][lane]);
        if (f % NCH == 0) v += prm[L.ob4 + f / NCH];
        s_buf[0][f][lane] = v;
      }
      for (int f = 0; f < QC_KMAX * NCH; ++f) s_buf[1][f][lane] = 0.f;
      float res[QC_SYS_EQ] = {0.f, 0.f, 0.f, 0.f};
      for (int t = 0; t < sys.n_terms; ++t) {
        const QcSysTerm tm = sys.terms[t];
        float v = tm.coef * s_buf[0][tm.out * NCH + tm.chan][lane];
        if (tm.mul0 >= 0) v *= s_buf[0][tm.mul0 * NCH][lane];
        if (tm.mul1 >= 0) v *= s_buf[0][tm.mul1 * NCH][lane];
#pragma unroll
        for (int e = 0; e < QC_SYS_EQ; ++e) res[e] += (tm.eq == e) ? v : 0.f;
      }
      float gsc[QC_SYS_EQ], ls = 0.f;
#pragma unroll
      for (int e = 0; e < QC_SYS_EQ; ++e) {
        gsc[e] = 0.f;
        if (e < sys.n_eq) {
          const float err = live ? res[e] - (tg ? tg[(int64_t)e * B + pc] : 0.f) : 0.f;
          const float we = sys.w_eq[e] * err;
          gsc[e] = pde.w_res * we;
          ls += we * err * pde.inv_n_res;
        }
      }
      ls = qc_wave_sum_to_lane63(ls);
      if (lane == 63) {
        row[L.NP + 0] = ls;
        row[L.NP + 1] = 0.f;
        row[L.NP + 2] = 0.f;
      }
      for (int t = 0; t < sys.n_terms; ++t) {
        const QcSysTerm tm = sys.terms[t];
        float gv = 0.f;
#pragma unroll
        for (int e = 0; e < QC_SYS_EQ; ++e) gv = (tm.eq == e) ? gsc[e] : gv;
        gv *= tm.coef;
        const float a = s_buf[0][tm.out * NCH + tm.chan][lane];
        const float x0 = tm.mul0 >= 0 ? s_buf[0][tm.mul0 * NCH][lane] : 1.f;
        const float x1 = tm.mul1 >= 0 ? s_buf[0][tm.mul1 * NCH][lane] : 1.f;
        s_buf[1][tm.out * NCH + tm.chan][lane] += gv * x0 * x1;
        if (tm.mul0 >= 0) s_buf[1][tm.mul0 * NCH][lane] += gv * a * x1;
        if (tm.mul1 >= 0) s_buf[1][tm.mul1 * NCH][lane] += gv * a * x0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k)
#pragma unroll
      for (int c = 0; c < NCH; ++c) ub[k][c] = k < K ? s_buf[1][k * NCH + c][lane] : 0.f;
    __syncthreads();   // s_buf[1] is read by every wave before any wave refills its slice below
  }
  // ---- reverse (k_post_multi mode 3): d / d b4[k] = sum of the points' cotangents of u_k
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k)
      if (k < K) {
        const float sb = qc_wave_sum_to_lane63(ub[k][0]);
        if (lane == 63) row[L.ob4 + k] = sb;
      }
  }
  float qb[NCH][N];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) qb[c][i] = 0.f;
  for (int m = m0; m < m1; ++m) {
    float g[NCH], z, f[NCH];
    hidden(m, g, z, f);
    float ubw[NCH], gk[QC_KMAX];
#pragma unroll
    for (int c = 0; c < NCH; ++c) ubw[c] = 0.f;
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k) {
      gk[k] = 0.f;
      if (k < K) {
        const float w4 = W4[k * L.H + m];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          ubw[c] = fmaf(w4, ub[k][c], ubw[c]);
          gk[k] = fmaf(ub[k][c], f[c], gk[k]);
        }
      }
    }
    float gb[NCH], gw4;
    post_cotangents<N, NCH>(gb, gw4, g, ubw, z, 1.f);
    float wg[N + 1];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float w3 = W3[m * N + i];
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        qb[c][i] = fmaf(w3, gb[c], qb[c][i]);
        sum = fmaf(gb[c], q[c][i], sum);
      }
      wg[i] = sum;
    }
    wg[N] = gb[0];
    qc_wave_sum_merged<N + 1>(wg);
    post_store_w3b3<N>(row, L, wg, m, lane);
#pragma unroll
    for (int k = 0; k < QC_KMAX; ++k)
      if (k < K) gk[k] = qc_wave_sum_to_lane63(gk[k]);
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < QC_KMAX; ++k)
        if (k < K) row[L.oW4 + k * L.H + m] = gk[k];
    }
  }
  if constexpr (NCH == 1) __syncthreads();   // the partial sums of u are read by every wave before any slice is refilled
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) s_buf[wave][c * N + i][lane] = qb[c][i];
  __syncthreads();
  if (live) {
    for (int f = wave; f < NCH * N; f += QC_MS)
      qbar[(int64_t)f * B + p] = (s_buf[0][f][lane] + s_buf[1][f][lane]) + (s_buf[2][f][lane] + s_buf[3][f][lane]);
  }
}

int qc_mlp_post_system(const float* prm, QcLayout L, const QcSys& sys, QcPde pde, const float* qjets, const float* tg,
                       float* qbar, float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t st) {
  static_assert(QC_SYS_K == QC_KMAX, "outputs of a system");
  if (sys.K < 1 || sys.K > QC_KMAX || L.H > 1024) return QC_ERR_UNSUPPORTED;
  const int tiles = qc_ceil_div(B, 64);
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto c) {
      hipLaunchKernelGGL((k_post_system<n(), c()>), dim3(tiles), dim3(256), 0, st, prm, L, sys, pde, qjets, tg, qbar, part,
                         part_stride, row0, B);
    };
    if (nch == 6) launch(qc_int<6>{}); else launch(qc_int<1>{});
  });
}

// ------------------------------------------------------------------ the learned-operator kind (the inverse step)
// qc_mlp_post (mode 2) with the trailing arguments (QcTab, QcLearn): the fused kernel, or point kernel and weight-gradient
// kernel; the residual tiles leave their six channel cotangents in out_u, which the weight-gradient kernel reads in its
// gen mode
static int post_learn(const float* prm, QcLayout L, QcPde pde, const float* qjets, float* out_u, float* qbar, float* part,
                      int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t st, const QcTarget& tg) {
  const int tiles = qc_ceil_div(B, 64);
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (L.n + 2) * HB * sizeof(float);
  const bool fused = post_fused_ok(L);
  const size_t shr = qc_post_fused_lds_res(L), shv = qc_post_fused_lds_val(L);
  const float* X = nullptr;      // tabulated targets: not read
  float* out_res = nullptr;      // six cotangents in out_u: not written
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto c) {
      constexpr int N = n(), NCH = c();
      if (fused) {
        hipLaunchKernelGGL((k_post_fused<N, NCH, QcTab, QcLearn>), dim3(NCH == 6 ? tiles : qc_ceil_div(tiles, QC_POST_VALUE_TPB)),
                           dim3(256), NCH == 6 ? shr : shv, st, X, prm, L, pde, qjets, out_u, out_res, qbar, part, part_stride, row0,
                           B, tg.tab, tg.learn);
        return;
      }
      hipLaunchKernelGGL((k_post<N, NCH, 2, QcTab, QcLearn>), dim3(tiles), dim3(256), 0, st, X, prm, L, pde, qjets, out_u, out_res,
                         (const float*)nullptr, (const float*)nullptr, qbar, part, part_stride, row0, B, tg.tab, tg.learn);
      hipLaunchKernelGGL((k_post_wg<N, NCH>), dim3(tiles), dim3(threads), sh, st, prm, L, pde, qjets, (const float*)out_u,
                         (const float*)nullptr, part, part_stride, row0, B, HB, PS, NCH == 6 ? 1 : 0);
    };
    if (nch == 6) launch(qc_int<6>{}); else launch(qc_int<1>{});
  });
}

// qc_mlp_post_both with the same arguments: the merged form exists for the register family only (n = 2 .. 5)
static int post_both_learn(const float* prm, QcLayout L, QcPde pde, const QcPostSeg& r, const QcPostSeg& v, float* part,
                           int64_t part_stride, hipStream_t st, const QcTarget& tg) {
  const int nr = qc_ceil_div(r.B, 64), nv = qc_ceil_div(v.B, 64);
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (L.n + 2) * HB * sizeof(float);
  const int nv4 = qc_ceil_div(nv, 4), nvf = qc_ceil_div(nv, QC_POST_VALUE_TPB);
  const bool fused = post_fused_ok(L);
  const size_t shr = qc_post_fused_lds_res(L), shv = qc_post_fused_lds_val(L), shf = shr > shv ? shr : shv;
  return qc_dispatch_n<2, 5>(L.n, [&](auto n) {
    constexpr int N = n();
    if (fused) {
      hipLaunchKernelGGL((k_post_fused_both<N, QcTab, QcLearn>), dim3(nr + nvf), dim3(256), shf, st, prm, L, pde, r, v, part,
                         part_stride, nr, tg.tab, tg.learn);
    } else {
      hipLaunchKernelGGL((k_post_both<N, QcTab, QcLearn>), dim3(nr + nv4), dim3(256), 0, st, prm, L, pde, r, v, part, part_stride,
                         nv4, tg.tab, tg.learn);
      hipLaunchKernelGGL((k_post_wg_both<N, true>), dim3(nr + nv), dim3(threads), sh, st, prm, L, pde, r, v, part, part_stride,
                         HB, PS, nv);
    }
  });
}

// ------------------------------------------------------------------ the balanced kind (the balanced step)
// qc_mlp_post (mode 2) with the trailing arguments (QcTab, QcBal): the tabulated kind's launches (per-point cotangents in
// out_u / out_res, the weight-gradient kernel in its plain mode)
static int post_bal(const float* prm, QcLayout L, QcPde pde, const float* qjets, float* out_u, float* out_res, float* qbar,
                    float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t st, const QcTarget& tg) {
  const int tiles = qc_ceil_div(B, 64);
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (L.n + 2) * HB * sizeof(float);
  const bool fused = post_fused_ok(L);
  const size_t shr = qc_post_fused_lds_res(L), shv = qc_post_fused_lds_val(L);
  const float* X = nullptr;      // tabulated targets: not read
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto c) {
      constexpr int N = n(), NCH = c();
      if (fused) {
        hipLaunchKernelGGL((k_post_fused<N, NCH, QcTab, QcBal>), dim3(NCH == 6 ? tiles : qc_ceil_div(tiles, QC_POST_VALUE_TPB)),
                           dim3(256), NCH == 6 ? shr : shv, st, X, prm, L, pde, qjets, out_u, out_res, qbar, part, part_stride, row0,
                           B, tg.tab, tg.bal);
        return;
      }
      hipLaunchKernelGGL((k_post<N, NCH, 2, QcTab, QcBal>), dim3(tiles), dim3(256), 0, st, X, prm, L, pde, qjets, out_u, out_res,
                         (const float*)nullptr, (const float*)nullptr, qbar, part, part_stride, row0, B, tg.tab, tg.bal);
      hipLaunchKernelGGL((k_post_wg<N, NCH>), dim3(tiles), dim3(threads), sh, st, prm, L, pde, qjets, (const float*)out_u,
                         (NCH == 6 ? (const float*)out_res : nullptr), part, part_stride, row0, B, HB, PS, 0);
    };
    if (nch == 6) launch(qc_int<6>{}); else launch(qc_int<1>{});
  });
}

// qc_mlp_post_both with the same arguments: the merged form exists for the register family only (n = 2 .. 5)
static int post_both_bal(const float* prm, QcLayout L, QcPde pde, const QcPostSeg& r, const QcPostSeg& v, float* part,
                         int64_t part_stride, hipStream_t st, const QcTarget& tg) {
  const int nr = qc_ceil_div(r.B, 64), nv = qc_ceil_div(v.B, 64);
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (L.n + 2) * HB * sizeof(float);
  const int nv4 = qc_ceil_div(nv, 4), nvf = qc_ceil_div(nv, QC_POST_VALUE_TPB);
  const bool fused = post_fused_ok(L);
  const size_t shr = qc_post_fused_lds_res(L), shv = qc_post_fused_lds_val(L), shf = shr > shv ? shr : shv;
  return qc_dispatch_n<2, 5>(L.n, [&](auto n) {
    constexpr int N = n();
    if (fused) {
      hipLaunchKernelGGL((k_post_fused_both<N, QcTab, QcBal>), dim3(nr + nvf), dim3(256), shf, st, prm, L, pde, r, v, part,
                         part_stride, nr, tg.tab, tg.bal);
    } else {
      hipLaunchKernelGGL((k_post_both<N, QcTab, QcBal>), dim3(nr + nv4), dim3(256), 0, st, prm, L, pde, r, v, part, part_stride,
                         nv4, tg.tab, tg.bal);
      hipLaunchKernelGGL((k_post_wg_both<N, false>), dim3(nr + nv), dim3(threads), sh, st, prm, L, pde, r, v, part, part_stride,
                         HB, PS, nv);
    }
  });
}

// ================================================================== Fourier-feature input encoding of the pre network
// gamma(X) = [sin(2 pi X B), cos(2 pi X B)] in front of Linear(2m, H) (Tancik et al. 2020; the reference's
// hybrid_testing/modified_qpinn_cg.py:75-95).  B is [3][m] fp32, not trained; W1 is [H][2m] row-major in the order of
// torch.cat([sin, cos]).  Per point r_j = B_tj t + B_xj x + B_yj y (turns), s_j = sin 2 pi r_j, c_j = cos 2 pi r_j,
// w_jk = 2 pi B_kj; hidden unit u with P_j = W1[u][j], Q_j = W1[u][m + j], A_j = P_j s_j + Q_j c_j, D_j = P_j c_j - Q_j s_j:
//   h = b1[u] + sum_j A_j,   h_k = sum_j w_jk D_j (k = t, x, y),   h_kk = -sum_j w_jk^2 A_j (kk = xx, yy)
// and from the six channels of h on the stage is the plain one (tanh jets, W2, angle map).  These kernels stand behind
// every other kernel of the code object; the plain stages keep their code.  m is a run-time value (1 .. QC_FF_MAX).
namespace {

constexpr int QC_FF_FB = 8;    // frequencies per block of the forward pass (a block's P, Q: two runs of eight scalar loads)
constexpr int QC_FF_BB = 16;   // frequencies per block of the reverse pass (2 x 16 accumulators)
constexpr float QC_2PI_F = 6.28318530717958647692f;

struct QcFF {
  const float* freq;   // [3][m], device
  int m;
};

// sine and cosine of frequency j at a point.  r minus its nearest integer is exact in fp32, so the argument is at most half
// a turn whatever the scale of B; sinpif / cospif reduce exactly as well and take no private array (the large-argument
// path of sinf does), so these kernels stay without scratch.
__device__ __forceinline__ void ff_trig(const float* __restrict__ fq, const int m, const int j, const float t, const float x,
                                        const float y, float& s, float& c) {
  float r = fmaf(fq[j], t, fmaf(fq[m + j], x, fq[2 * m + j] * y));
  r -= rintf(r);
  s = sinpif(2.f * r);
  c = cospif(2.f * r);
}

// the table of the five factors a channel takes per frequency: w_t, w_x, w_y, w_x^2, w_y^2 as [5][mp], zero from m to mp
__device__ __forceinline__ void ff_stage_omega(float* __restrict__ s_om, const QcFF& ff, const int mp) {
  for (int i = threadIdx.x; i < 5 * mp; i += blockDim.x) {
    const int k = i / mp, j = i - k * mp;
    float w = 0.f;
    if (j < ff.m) {
      w = QC_2PI_F * ff.freq[(k < 3 ? k : k - 2) * ff.m + j];
      if (k >= 3) w = w * w;
    }
    s_om[i] = w;
  }
}

// Forward.  Block = 4 waves on one 64-point tile, lane = point, as k_pre_fwd_body (the same draw, the same Xout).  Wave w
// forms s_j, c_j for j = w, w + 4, ... once per tile and parks them in LDS as [2][mp][64] (lane-contiguous rows); then each
// wave walks its quarter of the hidden units over frequency blocks of QC_FF_FB.  The row of W1 is wave-uniform and
// contiguous: P and Q of a block arrive as scalar loads.  The tail block reads on past m (still inside the flat vector:
// at least seven entries follow W1 in every layout) and takes zero weights; the LDS rows from m to mp (m rounded up to a
// block) hold zeros, so a block's rows sit at constant offsets from one base.
// s_dyn: [2][mp][64] trig rows (sines, cosines), then the [5][mp] factor table; s_part: [QC_MS][NCH * N][64].
template <int N, int NCH, int MAP, bool RF>
__device__ __forceinline__ void k_pre_ff_fwd_body(const int64_t bid, const float* __restrict__ X, const float* __restrict__ prm,
                                                  QcLayout L, float* __restrict__ ajets, int64_t B, const QcFF ff,
                                                  float* __restrict__ s_dyn, float* __restrict__ s_part,
                                                  const QcDraw* __restrict__ draw, float* __restrict__ Xout) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = ff.m, mp = (m + QC_FF_FB - 1) & ~(QC_FF_FB - 1);
  float* __restrict__ s_trig = s_dyn;
  float* __restrict__ s_om = s_dyn + (size_t)2 * mp * 64;
  const int64_t p = (int64_t)bid * 64 + lane;
  const int64_t pc = p < B ? p : B - 1;
  float t, x, y;
  if (draw != nullptr && draw->enabled) {
    if (NCH == 6) qc_draw_point(0, draw->off_res + pc, 0, draw->seed, draw->step, t, x, y);
    else if (pc < draw->n_ic) qc_draw_point(1, draw->off_ic + pc, 0, draw->seed, draw->step, t, x, y);
    else qc_draw_point<RF>(2, draw->off_bc + (pc - draw->n_ic), draw->face_pts, draw->seed, draw->step, t, x, y);
    if (wave == 0 && p < B) {
      Xout[p * 3 + 0] = t;
      Xout[p * 3 + 1] = x;
      Xout[p * 3 + 2] = y;
    }
  } else {
    t = X[pc * 3 + 0];
    x = X[pc * 3 + 1];
    y = X[pc * 3 + 2];
  }
  ff_stage_omega(s_om, ff, mp);
  for (int j = wave; j < mp; j += QC_MS) {
    float s = 0.f, c = 0.f;
    if (j < m) ff_trig(ff.freq, m, j, t, x, y, s, c);
    s_trig[j * 64 + lane] = s;
    s_trig[(mp + j) * 64 + lane] = c;
  }
  __syncthreads();
  constexpr int NP2 = NCH == 6 ? 3 : 1;
  mf2 acc2[NP2][N];
#pragma unroll
  for (int cp = 0; cp < NP2; ++cp)
#pragma unroll
    for (int i = 0; i < N; ++i) acc2[cp][i] = (mf2){0.f, 0.f};
  const float* __restrict__ W1 = prm + L.oW1;
  const float* __restrict__ b1 = prm + L.ob1;
  const float* __restrict__ W2 = prm + L.oW2;
  const int hq = (L.H + QC_MS - 1) / QC_MS;
  const int u0 = wave * hq, u1 = (u0 + hq) < L.H ? (u0 + hq) : L.H;
  for (int u = u0; u < u1; ++u) {
    const float* __restrict__ Pr = W1 + (size_t)u * 2 * m;
    const float b1u = b1[u];
    float w2u[N];
#pragma unroll
    for (int i = 0; i < N; ++i) w2u[i] = W2[i * L.H + u];
    float h[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) h[c] = 0.f;
    for (int jb = 0; jb < m; jb += QC_FF_FB) {
      float P[QC_FF_FB], Q[QC_FF_FB];
      const float* __restrict__ pp = Pr + jb;
      const float* __restrict__ pq = Pr + m + jb;
#pragma unroll
      for (int i = 0; i < QC_FF_FB; ++i) P[i] = pp[i];
#pragma unroll
      for (int i = 0; i < QC_FF_FB; ++i) Q[i] = pq[i];
      const float* __restrict__ ts = s_trig + jb * 64 + lane;
      const float* __restrict__ tc = ts + mp * 64;
      const float* __restrict__ om = s_om + jb;
#pragma unroll
      for (int i = 0; i < QC_FF_FB; ++i) {
        const bool ok = jb + i < m;
        const float pj = ok ? P[i] : 0.f, qj = ok ? Q[i] : 0.f;
        const float s = ts[i * 64], c = tc[i * 64];
        if constexpr (NCH == 6) {
          const float A = fmaf(pj, s, qj * c), D = fmaf(pj, c, -(qj * s));
          h[0] += A;
          h[1] = fmaf(om[i], D, h[1]);
          h[2] = fmaf(om[mp + i], D, h[2]);
          h[3] = fmaf(om[2 * mp + i], D, h[3]);
          h[4] = fmaf(-om[3 * mp + i], A, h[4]);
          h[5] = fmaf(-om[4 * mp + i], A, h[5]);
        } else {
          h[0] = fmaf(pj, s, fmaf(qj, c, h[0]));
        }
      }
    }
    const float z = qc_tanh(h[0] + b1u);
    if constexpr (NCH == 6) {
      const float d1 = 1.f - z * z, d2 = -2.f * z * d1;
      const mf2 zc2[3] = {(mf2){z, d1 * h[1]}, (mf2){d1 * h[2], d1 * h[3]},
                          (mf2){fmaf(d2 * h[2], h[2], d1 * h[4]), fmaf(d2 * h[3], h[3], d1 * h[5])}};
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const mf2 wi = m_dup(w2u[i]);
#pragma unroll
        for (int cp = 0; cp < 3; ++cp) acc2[cp][i] = m_fma(wi, zc2[cp], acc2[cp][i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) acc2[0][i].x = fmaf(w2u[i], z, acc2[0][i].x);
    }
  }
  // from here the plain stage's epilogue: the four partial jets meet in LDS, b2, the optional angle map
  constexpr int NF = NCH * N;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i)
      s_part[(wave * NF + c * N + i) * 64 + lane] = (c & 1) ? acc2[c >> 1][i].y : acc2[c >> 1][i].x;
  __syncthreads();
  if (p < B) {
    auto total = [&](const int f) {
      return (s_part[f * 64 + lane] + s_part[(NF + f) * 64 + lane]) + (s_part[(2 * NF + f) * 64 + lane] + s_part[(3 * NF + f) * 64 + lane]);
    };
    if constexpr (MAP == 0) {
      for (int f = wave; f < NF; f += QC_MS) {
        float v = total(f);
        if (f < N) v += prm[L.ob2 + f];
        qc_store_wt(&ajets[(int64_t)f * B + p], v);
      }
    } else {
      for (int i = wave; i < N; i += QC_MS) {
        float v[NCH], a[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = total(c * N + i);
        v[0] += prm[L.ob2 + i];
        angle_map_fwd<NCH>(v, a);
#pragma unroll
        for (int c = 0; c < NCH; ++c) qc_store_wt(&ajets[(int64_t)(c * N + i) * B + p], a[c]);
      }
    }
  }
}

template <int N, int NCH, int MAP>
__global__ void __launch_bounds__(256) k_pre_ff_fwd(const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                                                    float* __restrict__ ajets, int64_t B, QcFF ff) {
  extern __shared__ float s_dyn[];
  __shared__ float s_part[QC_MS * NCH * N * 64];
  k_pre_ff_fwd_body<N, NCH, MAP, false>(blockIdx.x, X, prm, L, ajets, B, ff, s_dyn, s_part, nullptr, nullptr);
}

// merged launch: the value tiles first (one tile per block here as well: a tile's trig rows are shared by its four waves)
template <int N, int MAP, bool RF>
__global__ void __launch_bounds__(256) k_pre_ff_fwd_both(float* __restrict__ Xr, float* __restrict__ Xv,
                                                         const float* __restrict__ prm, QcLayout L, float* __restrict__ ajr,
                                                         float* __restrict__ ajv, int64_t Br, int64_t Bv, int n_val, QcDraw draw,
                                                         QcFF ff) {
  extern __shared__ float s_dyn[];
  __shared__ float s_part[QC_MS * 6 * N * 64];
  if ((int)blockIdx.x >= n_val) k_pre_ff_fwd_body<N, 6, MAP, RF>(blockIdx.x - n_val, Xr, prm, L, ajr, Br, ff, s_dyn, s_part, &draw, Xr);
  else k_pre_ff_fwd_body<N, 1, MAP, RF>(blockIdx.x, Xv, prm, L, ajv, Bv, ff, s_dyn, s_part, &draw, Xv);
}

// Reverse.  Lane = hidden unit, PS groups of HB threads share the tile's 64 points (ff_geometry).  The tile's s, c rows are
// formed once into LDS and read as broadcasts; pre-activations and tanh are recomputed.  dP, dQ are accumulated per block
// of QC_FF_BB frequencies with the point loop inside the block, so m = 64 needs 32 live accumulators, not 128; every block
// after the first recomputes the unit's six channels at each point (m <= 16: one block, nothing recomputed twice).
// Group sums: qc_group_sums, ascending in the group; PS = 1 stores from registers.  Fixed order, no atomics.
// s_dyn: [2][mp][64] trig rows (mp: m rounded up to QC_FF_BB; zeros from m on), [5][mp] factor table, s_acc [PS][2 QC_FF_BB][HB]
// (PS > 1).
template <int N, int NCH, int MAP>
__device__ __forceinline__ void k_pre_ff_bwd_body(const int64_t bid, const float* __restrict__ X, const float* __restrict__ prm,
                                                  QcLayout L, const float* __restrict__ abar, float* __restrict__ part,
                                                  int64_t part_stride, int64_t row0, int64_t B, int HB, int PS,
                                                  const float* __restrict__ aj, const QcFF ff, float* __restrict__ s_dyn,
                                                  float* __restrict__ sX, mf2* __restrict__ sA2) {
  constexpr int KA = 2 * QC_FF_BB;
  static_assert(KA >= 1 + N, "the b1 / W2 sums pass through the same buffer");
  const int m = ff.m, mp = (m + QC_FF_BB - 1) & ~(QC_FF_BB - 1);
  float* __restrict__ s_trig = s_dyn;
  float* __restrict__ s_om = s_dyn + (size_t)2 * mp * 64;
  float* __restrict__ s_acc = s_om + 5 * mp;
  const int64_t base = (int64_t)bid * 64;
  const int cnt = (int)((B - base) < 64 ? (B - base) : 64);
  for (int i = threadIdx.x; i < 64 * 3; i += blockDim.x) {
    const int pp = i / 3, k = i % 3;
    sX[k * 64 + pp] = pp < cnt ? X[(base + pp) * 3 + k] : 0.f;
  }
  if constexpr (MAP == 0) {
    for (int i = threadIdx.x; i < NCH * N * 64; i += blockDim.x) {
      const int f = i >> 6, pp = i & 63;      // f = c * N + wire
      const int c = f / N, w = f % N;
      const float v = pp < cnt ? abar[(int64_t)f * B + base + pp] : 0.f;
      if (c & 1) sA2[((c >> 1) * N + w) * 64 + pp].y = v;
      else sA2[((c >> 1) * N + w) * 64 + pp].x = v;
    }
  } else {
    for (int i = threadIdx.x; i < N * 64; i += blockDim.x) {
      const int w = i >> 6, pp = i & 63;
      float ab[NCH], a[NCH], vb[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int64_t o = (int64_t)(c * N + w) * B + base + pp;
        ab[c] = pp < cnt ? abar[o] : 0.f;
        a[c] = pp < cnt ? aj[o] : 0.f;
      }
      angle_map_bwd<NCH>(ab, a, vb);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (c & 1) sA2[((c >> 1) * N + w) * 64 + pp].y = vb[c];
        else sA2[((c >> 1) * N + w) * 64 + pp].x = vb[c];
      }
    }
  }
  ff_stage_omega(s_om, ff, mp);
  __syncthreads();
  for (int i = threadIdx.x; i < mp * 64; i += blockDim.x) {
    const int j = i >> 6, pp = i & 63;
    float s = 0.f, c = 0.f;
    if (j < m) ff_trig(ff.freq, m, j, sX[pp], sX[64 + pp], sX[128 + pp], s, c);
    s_trig[j * 64 + pp] = s;
    s_trig[(mp + j) * 64 + pp] = c;
  }
  __syncthreads();

  const int grp = threadIdx.x / HB, u = threadIdx.x % HB;
  const bool active = grp < PS && u < L.H;
  // a group walks `per` points from p0 on: a wave-uniform trip count (a wave may hold lanes of two groups).  Points from
  // cnt to 63 were staged as zero cotangents and add exact zeros; a point index past 63 (PS does not divide 64) is skipped
  const int per = (64 + PS - 1) / PS;
  const int p0 = grp * per;
  const int uc = u < L.H ? u : L.H - 1;       // (a thread without a hidden unit reads the last one's and stores nothing)
  const float* __restrict__ Pr = prm + L.oW1 + (size_t)uc * 2 * m;
  const float b1u = prm[L.ob1 + uc];
  float w2c[N];
#pragma unroll
  for (int i = 0; i < N; ++i) w2c[i] = prm[L.oW2 + i * L.H + uc];
  float gb1 = 0.f, gW2[N];   // (one register per wire, not a pair: the frequency block needs the rest)
#pragma unroll
  for (int i = 0; i < N; ++i) gW2[i] = 0.f;
  float* row = part + (row0 + bid) * part_stride;

  for (int f0 = 0; f0 < m; f0 += QC_FF_BB) {
    float gP[QC_FF_BB], gQ[QC_FF_BB];
#pragma unroll
    for (int i = 0; i < QC_FF_BB; ++i) gP[i] = gQ[i] = 0.f;
    {
      for (int k = 0; k < per; ++k) {
        const int pp = p0 + k;
        if (pp >= 64) continue;
        float h[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) h[c] = 0.f;
#pragma unroll 1
        for (int j = 0; j < m; ++j) {
          const float pj = Pr[j], qj = Pr[m + j];
          const float s = s_trig[j * 64 + pp], c = s_trig[(mp + j) * 64 + pp];
          if constexpr (NCH == 6) {
            const float A = fmaf(pj, s, qj * c), D = fmaf(pj, c, -(qj * s));
            h[0] += A;
            h[1] = fmaf(s_om[j], D, h[1]);
            h[2] = fmaf(s_om[mp + j], D, h[2]);
            h[3] = fmaf(s_om[2 * mp + j], D, h[3]);
            h[4] = fmaf(-s_om[3 * mp + j], A, h[4]);
            h[5] = fmaf(-s_om[4 * mp + j], A, h[5]);
          } else {
            h[0] = fmaf(pj, s, fmaf(qj, c, h[0]));
          }
        }
        const float z = qc_tanh(h[0] + b1u);
        const float d1 = 1.f - z * z;
        float hb[NCH];
        if constexpr (NCH == 6) {
          const float d2 = -2.f * z * d1;
          const float d3 = -2.f * (d1 * d1 + z * d2);
          const mf2 zc2[3] = {(mf2){z, d1 * h[1]}, (mf2){d1 * h[2], d1 * h[3]},
                              (mf2){fmaf(d2 * h[2], h[2], d1 * h[4]), fmaf(d2 * h[3], h[3], d1 * h[5])}};
          mf2 zb2[3] = {(mf2){0.f, 0.f}, (mf2){0.f, 0.f}, (mf2){0.f, 0.f}};
          // a cotangent pair is read once and used twice (never kept: 6 N registers the frequency block needs)
#pragma unroll
          for (int i = 0; i < N; ++i)
#pragma unroll
            for (int cp = 0; cp < 3; ++cp) {
              const mf2 a2 = sA2[(cp * N + i) * 64 + pp];
              zb2[cp] = m_fma(m_dup(w2c[i]), a2, zb2[cp]);
              if (f0 == 0) gW2[i] = fmaf(a2.x, zc2[cp].x, fmaf(a2.y, zc2[cp].y, gW2[i]));
            }
          const float zb[6] = {zb2[0].x, zb2[0].y, zb2[1].x, zb2[1].y, zb2[2].x, zb2[2].y};
          hb[0] = zb[0] * d1 + (zb[1] * h[1] + zb[2] * h[2] + zb[3] * h[3]) * d2 +
                  zb[4] * (d3 * h[2] * h[2] + d2 * h[4]) + zb[5] * (d3 * h[3] * h[3] + d2 * h[5]);
          hb[1] = zb[1] * d1;
          hb[2] = zb[2] * d1 + 2.f * zb[4] * d2 * h[2];
          hb[3] = zb[3] * d1 + 2.f * zb[5] * d2 * h[3];
          hb[4] = zb[4] * d1;
          hb[5] = zb[5] * d1;
        } else {
          float zb0 = 0.f;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const float a = sA2[i * 64 + pp].x;
            zb0 = fmaf(w2c[i], a, zb0);
            if (f0 == 0) gW2[i] = fmaf(a, z, gW2[i]);
          }
          hb[0] = zb0 * d1;
        }
        if (f0 == 0) gb1 += hb[0];
        const float* __restrict__ ts = s_trig + f0 * 64 + pp;
        const float* __restrict__ tc = ts + mp * 64;
        // the block's eighty factors do not depend on the point: read here they stay LDS broadcasts; hoisted out of the point
        // loop they would be eighty registers, so the address passes through an empty asm at every point
#if defined(__HIP_DEVICE_COMPILE__)
        const __attribute__((address_space(3))) float* om = (const __attribute__((address_space(3))) float*)(s_om + f0);
        asm volatile("" : "+v"(om));
#else
        const float* om = s_om + f0;
#endif
#pragma unroll
        for (int i = 0; i < QC_FF_BB; ++i) {
          const float s = ts[i * 64], c = tc[i * 64];
          if constexpr (NCH == 6) {
            const float al = fmaf(-om[4 * mp + i], hb[5], fmaf(-om[3 * mp + i], hb[4], hb[0]));
            const float be = fmaf(om[2 * mp + i], hb[3], fmaf(om[mp + i], hb[2], om[i] * hb[1]));
            gP[i] += fmaf(s, al, c * be);
            gQ[i] += fmaf(c, al, -(s * be));
          } else {
            gP[i] = fmaf(s, hb[0], gP[i]);
            gQ[i] = fmaf(c, hb[0], gQ[i]);
          }
        }
      }
    }
    if (PS == 1) {
      if (active) {
#pragma unroll
        for (int i = 0; i < QC_FF_BB; ++i)
          if (f0 + i < m) {
            row[L.oW1 + (size_t)u * 2 * m + f0 + i] = gP[i];
            row[L.oW1 + (size_t)u * 2 * m + m + f0 + i] = gQ[i];
          }
      }
    } else {
      __syncthreads();   // the previous block's sums have been read
      if (grp < PS) {
        float* mine = s_acc + (size_t)grp * KA * HB;
#pragma unroll
        for (int i = 0; i < QC_FF_BB; ++i) {
          mine[i * HB + u] = gP[i];
          mine[(QC_FF_BB + i) * HB + u] = gQ[i];
        }
      }
      __syncthreads();
      if (grp == 0 && u < L.H) {
        float tot[KA];
        qc_group_sums<KA>(s_acc, PS, HB, u, tot);
#pragma unroll
        for (int i = 0; i < QC_FF_BB; ++i)
          if (f0 + i < m) {
            row[L.oW1 + (size_t)u * 2 * m + f0 + i] = tot[i];
            row[L.oW1 + (size_t)u * 2 * m + m + f0 + i] = tot[QC_FF_BB + i];
          }
      }
    }
  }
  // b1 and W2: one more pass through the buffer (its first 1 + N rows of each group, stride KA as before)
  if (PS == 1) {
    if (active) {
      row[L.ob1 + u] = gb1;
#pragma unroll
      for (int i = 0; i < N; ++i) row[L.oW2 + i * L.H + u] = gW2[i];
    }
  } else {
    __syncthreads();
    if (grp < PS) {
      float* mine = s_acc + (size_t)grp * KA * HB;
      mine[u] = gb1;
#pragma unroll
      for (int i = 0; i < N; ++i) mine[(1 + i) * HB + u] = gW2[i];
    }
    __syncthreads();
    if (grp == 0 && u < L.H) {
      float tb = 0.f, tw[N];
#pragma unroll
      for (int i = 0; i < N; ++i) tw[i] = 0.f;
      for (int g = 0; g < PS; ++g) {
        const float* his = s_acc + (size_t)g * KA * HB;
        tb += his[u];
#pragma unroll
        for (int i = 0; i < N; ++i) tw[i] += his[(1 + i) * HB + u];
      }
      row[L.ob1 + u] = tb;
#pragma unroll
      for (int i = 0; i < N; ++i) row[L.oW2 + i * L.H + u] = tw[i];
    }
  }
  if (threadIdx.x < N) {  // b2 only feeds the value channel
    float sum = 0.f;
    for (int pp = 0; pp < cnt; ++pp) sum += sA2[threadIdx.x * 64 + pp].x;
    row[L.ob2 + threadIdx.x] = sum;
  }
}

template <int N, int NCH, int MAP>
__global__ void k_pre_ff_bwd(const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                             const float* __restrict__ abar, float* __restrict__ part, int64_t part_stride, int64_t row0,
                             int64_t B, int HB, int PS, const float* __restrict__ aj, QcFF ff) {
  extern __shared__ float s_dyn[];
  __shared__ float sX[3 * 64];
  __shared__ mf2 sA2[(NCH == 6 ? 3 : 1) * N * 64];
  k_pre_ff_bwd_body<N, NCH, MAP>(blockIdx.x, X, prm, L, abar, part, part_stride, row0, B, HB, PS, aj, ff, s_dyn, sX, sA2);
}

template <int N, int MAP>
__global__ void k_pre_ff_bwd_both(const float* __restrict__ Xr, const float* __restrict__ Xv, const float* __restrict__ prm,
                                  QcLayout L, const float* __restrict__ abr, const float* __restrict__ abv,
                                  float* __restrict__ part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br,
                                  int64_t Bv, int HB, int PS, int n_val, const float* __restrict__ ajr,
                                  const float* __restrict__ ajv, QcFF ff) {
  extern __shared__ float s_dyn[];
  __shared__ float sX[3 * 64];
  __shared__ mf2 sA2[3 * N * 64];
  if ((int)blockIdx.x >= n_val)
    k_pre_ff_bwd_body<N, 6, MAP>(blockIdx.x - n_val, Xr, prm, L, abr, part, part_stride, row0_r, Br, HB, PS, ajr, ff, s_dyn, sX, sA2);
  else
    k_pre_ff_bwd_body<N, 1, MAP>(blockIdx.x, Xv, prm, L, abv, part, part_stride, row0_v, Bv, HB, PS, ajv, ff, s_dyn, sX, sA2);
}

}  // namespace

// ------------------------------------------------------------------ launchers of the Fourier-feature stages
static inline size_t ff_fwd_lds(const int m) {
  return (size_t)(2 * 64 + 5) * ((m + QC_FF_FB - 1) & ~(QC_FF_FB - 1)) * sizeof(float);
}
// the plain stage's geometry, with as many groups as keep the [PS][2 QC_FF_BB][HB] sums within 64 KB (PS HB <= 512); one
// group stores from registers and keeps no sums
static inline void ff_geometry(int H, int* HB, int* PS, int* threads) {
  hidden_geometry(H, HB, PS, threads);
  while (*PS > 1 && *HB * *PS > 512) *PS /= 2;
  *threads = 64 * qc_ceil_div(*HB * *PS, 64);
}
static inline size_t ff_bwd_lds(const int m, const int HB, const int PS) {
  const size_t acc = PS > 1 ? (size_t)PS * 2 * QC_FF_BB * HB : 0;
  return ((size_t)(2 * 64 + 5) * ((m + QC_FF_BB - 1) & ~(QC_FF_BB - 1)) + acc) * sizeof(float);
}

int qc_mlp_pre_ff_fwd(const float* X, const float* prm, QcLayout L, float* ajets, int64_t B, int nch, hipStream_t st, int map,
                      const float* freq, int m) {
  const int grid = qc_ceil_div(B, 64);
  const QcFF ff = {freq, m};
  const size_t sh = ff_fwd_lds(m);
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto c, auto mp) {
      hipLaunchKernelGGL((k_pre_ff_fwd<n(), c(), mp()>), dim3(grid), dim3(256), sh, st, X, prm, L, ajets, B, ff);
    };
    if (map) { if (nch == 6) launch(qc_int<6>{}, qc_int<1>{}); else launch(qc_int<1>{}, qc_int<1>{}); }
    else if (nch == 6) launch(qc_int<6>{}, qc_int<0>{});
    else launch(qc_int<1>{}, qc_int<0>{});
  });
}

int qc_mlp_pre_ff_bwd(const float* X, const float* prm, QcLayout L, const float* abar, float* part, int64_t part_stride,
                      int64_t row0, int64_t B, int nch, hipStream_t st, int map, const float* aj, const float* freq, int m) {
  const int grid = qc_ceil_div(B, 64);
  if (L.H > 1024 || L.n > 64) return QC_ERR_UNSUPPORTED;
  int HB, PS, threads;
  ff_geometry(L.H, &HB, &PS, &threads);
  const QcFF ff = {freq, m};
  const size_t sh = ff_bwd_lds(m, HB, PS);
  return qc_dispatch_n<1, QC_MLP_NMAX>(L.n, [&](auto n) {
    auto launch = [&](auto c, auto mp) {
      hipLaunchKernelGGL((k_pre_ff_bwd<n(), c(), mp()>), dim3(grid), dim3(threads), sh, st, X, prm, L, abar, part, part_stride,
                         row0, B, HB, PS, aj, ff);
    };
    if (map) { if (nch == 6) launch(qc_int<6>{}, qc_int<1>{}); else launch(qc_int<1>{}, qc_int<1>{}); }
    else if (nch == 6) launch(qc_int<6>{}, qc_int<0>{});
    else launch(qc_int<1>{}, qc_int<0>{});
  });
}

int qc_mlp_pre_ff_fwd_both(const QcBatches& b, int draw, int64_t face_pts, const float* prm, QcLayout L, float* ajr, float* ajv,
                           hipStream_t st, int map, const float* freq, int m) {
  float *Xr = b.X_res, *Xv = b.X_val;
  const int64_t Br = b.n_res, Bv = b.n_ic + b.n_bc;
  const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 64);
  const QcDraw dr = {draw, b.n_ic, b.off_res, b.off_ic, b.off_bc, face_pts, b.seed, b.step};
  const bool rf = draw && face_pts < 0;
  const QcFF ff = {freq, m};
  const size_t sh = ff_fwd_lds(m);
  // the merged form exists for the register family only (n = 2 .. 5)
  return qc_dispatch_n<2, 5>(L.n, [&](auto n) {
    auto launch = [&](auto mp, auto r) {
      hipLaunchKernelGGL((k_pre_ff_fwd_both<n(), mp(), r()>), dim3(nr + nv), dim3(256), sh, st, Xr, Xv, prm, L, ajr, ajv, Br, Bv,
                         nv, dr, ff);
    };
    if (map) { if (rf) launch(qc_int<1>{}, std::true_type{}); else launch(qc_int<1>{}, std::false_type{}); }
    else if (rf) launch(qc_int<0>{}, std::true_type{});
    else launch(qc_int<0>{}, std::false_type{});
  });
}

int qc_mlp_pre_ff_bwd_both(const float* Xr, const float* Xv, const float* prm, QcLayout L, const float* abr, const float* abv,
                           float* part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br, int64_t Bv,
                           hipStream_t st, int map, const float* ajr, const float* ajv, const float* freq, int m) {
  if (L.H > 1024 || L.n > 64) return QC_ERR_UNSUPPORTED;
  const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 64);
  int HB, PS, threads;
  ff_geometry(L.H, &HB, &PS, &threads);
  const QcFF ff = {freq, m};
  const size_t sh = ff_bwd_lds(m, HB, PS);
  return qc_dispatch_n<2, 5>(L.n, [&](auto n) {
    auto launch = [&](auto mp) {
      hipLaunchKernelGGL((k_pre_ff_bwd_both<n(), mp()>), dim3(nr + nv), dim3(threads), sh, st, Xr, Xv, prm, L, abr, abv, part,
                         part_stride, row0_r, row0_v, Br, Bv, HB, PS, nv, ajr, ajv, ff);
    };
    if (map) launch(qc_int<1>{}); else launch(qc_int<0>{});
  });
}

// ================================================================== ensembles: M members per launch
// One wrapper per merged stage of the fused step, grid (blocks of one member, M): member blockIdx.y's slices lie
// blockIdx.y strides behind member 0's (scalar arithmetic on kernel arguments), its sampler key is seed + blockIdx.y, its
// operator record comes from the table when there is one (scalar loads), and the tile runs the body of the single-model
// kernel: k_pre_fwd_both, k_post_fused_both (analytic targets) and k_pre_bwd_both.  Register family only (n = 2 .. 5).
namespace {

template <int N, int MAP, bool RF>
__global__ void __launch_bounds__(256) k_pre_fwd_ens(float* __restrict__ Xr, float* __restrict__ Xv,
                                                     const float* __restrict__ prm, QcLayout L, float* __restrict__ ajr,
                                                     float* __restrict__ ajv, int64_t Br, int64_t Bv, int n_val, QcDraw draw,
                                                     QcEns e) {
  // (the points and the angle jets are addressed per lane: their bases ride in vector registers, which this kernel has
  // to spare, where scalar registers are short)
  auto lanes = [](float* p) {
    asm volatile("" : "+v"(p));
    return p;
  };
  const int64_t m = blockIdx.y;
  draw.seed += (uint64_t)m;
  prm += m * e.prm;
  if ((int)blockIdx.x >= n_val) {
    float* X = lanes(Xr + m * e.X_res);
    k_pre_fwd_body<N, 6, MAP>(blockIdx.x - n_val, X, prm, L, lanes(ajr + m * e.jets_res), Br, &draw, X);
  } else {
    float* X = lanes(Xv + m * e.X_val);
    k_pre_fwd_value4<N, MAP, RF>(blockIdx.x, X, prm, L, lanes(ajv + m * e.jets_val), Bv, &draw, X);
  }
}

template <int N>
__global__ void __launch_bounds__(256) k_post_fused_ens(const float* __restrict__ prm, QcLayout L, QcPde pde, QcPostSeg r,
                                                        QcPostSeg v, float* __restrict__ part, int64_t part_stride, int n_res,
                                                        QcEns e) {
  extern __shared__ float s_dyn[];
  const int64_t m = blockIdx.y;
  if (e.pde != nullptr) pde = qc_ens_record(e.pde, (int)blockIdx.y);
  prm += m * e.prm;
  part += m * e.part;
  if ((int)blockIdx.x < n_res)
    k_post_fused6_body<N>(blockIdx.x, r.X + m * e.X_res, prm, L, pde, r.qjets + m * e.jets_res, r.ub + m * e.jets_res,
                          r.rb + m * e.jets_res, r.qbar + m * e.jets_res, part, part_stride, r.row0, r.B, s_dyn);
  else
    k_post_fused_value_body<N, QC_POST_VALUE_TPB>(blockIdx.x - n_res, v.X + m * e.X_val, prm, L, pde, v.qjets + m * e.jets_val,
                                                  v.ub + m * e.jets_val, v.qbar + m * e.jets_val, part, part_stride, v.row0, v.B,
                                                  s_dyn);
}

template <int N, int MAP>
__global__ void k_pre_bwd_ens(const float* __restrict__ Xr, const float* __restrict__ Xv, const float* __restrict__ prm,
                              QcLayout L, const float* __restrict__ abr, const float* __restrict__ abv,
                              float* __restrict__ part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br,
                              int64_t Bv, int HB, int PS, int n_val, const float* __restrict__ ajr,
                              const float* __restrict__ ajv, QcEns e) {
  const int64_t m = blockIdx.y;
  prm += m * e.prm;
  part += m * e.part;
  if ((int)blockIdx.x >= n_val)
    k_pre_bwd_body<N, 6, MAP>(blockIdx.x - n_val, Xr + m * e.X_res, prm, L, abr + m * e.jets_res, part, part_stride, row0_r, Br,
                              HB, PS, ajr + m * e.jets_res);
  else
    k_pre_bwd_body<N, 1, MAP>(blockIdx.x, Xv + m * e.X_val, prm, L, abv + m * e.jets_val, part, part_stride, row0_v, Bv, HB, PS,
                              ajv + m * e.jets_val);
}

}  // namespace

bool qc_mlp_ens_ok(const QcLayout& L) { return L.H <= QC_POST_FUSED_MAXH; }

int qc_mlp_pre_fwd_ens(const QcBatches& b, int draw, int64_t face_pts, const float* prm, QcLayout L, float* ajr, float* ajv,
                       hipStream_t st, int map, const QcEns& e) {
  float *Xr = b.X_res, *Xv = b.X_val;
  const int64_t Br = b.n_res, Bv = b.n_ic + b.n_bc;
  const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(qc_ceil_div(Bv, 64), 4);
  const QcDraw dr = {draw, b.n_ic, b.off_res, b.off_ic, b.off_bc, face_pts, b.seed, b.step};
  const bool rf = draw && face_pts < 0;
  return qc_dispatch_n<2, 5>(L.n, [&](auto n) {
    auto launch = [&](auto m, auto r) {
      hipLaunchKernelGGL((k_pre_fwd_ens<n(), m(), r()>), dim3(nr + nv, e.M), dim3(256), 0, st, Xr, Xv, prm, L, ajr, ajv, Br, Bv,
                         nv, dr, e);
    };
    if (map) { if (rf) launch(qc_int<1>{}, std::true_type{}); else launch(qc_int<1>{}, std::false_type{}); }
    else if (rf) launch(qc_int<0>{}, std::true_type{});
    else launch(qc_int<0>{}, std::false_type{});
  });
}

int qc_mlp_post_ens(const float* prm, QcLayout L, QcPde pde, const float* Xr, const float* qjr, float* ubr, float* rbr, float* qbr,
                    int64_t row0_r, int64_t Br, const float* Xv, const float* qjv, float* ubv, float* qbv, int64_t row0_v,
                    int64_t Bv, float* part, int64_t part_stride, hipStream_t st, const QcEns& e) {
  if (!qc_mlp_ens_ok(L)) return QC_ERR_UNSUPPORTED;
  const int nr = qc_ceil_div(Br, 64), nvf = qc_ceil_div(qc_ceil_div(Bv, 64), QC_POST_VALUE_TPB);
  const QcPostSeg r = {Xr, qjr, ubr, rbr, qbr, row0_r, Br}, v = {Xv, qjv, ubv, nullptr, qbv, row0_v, Bv};
  const size_t shr = qc_post_fused_lds_res(L), shv = qc_post_fused_lds_val(L), shf = shr > shv ? shr : shv;
  return qc_dispatch_n<2, 5>(L.n, [&](auto n) {
    hipLaunchKernelGGL((k_post_fused_ens<n()>), dim3(nr + nvf, e.M), dim3(256), shf, st, prm, L, pde, r, v, part, part_stride, nr,
                       e);
  });
}

int qc_mlp_pre_bwd_ens(const float* Xr, const float* Xv, const float* prm, QcLayout L, const float* abr, const float* abv,
                       float* part, int64_t part_stride, int64_t row0_r, int64_t row0_v, int64_t Br, int64_t Bv, hipStream_t st,
                       int map, const float* ajr, const float* ajv, const QcEns& e) {
  const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 64);
  int HB, PS, threads;
  hidden_geometry(L.H, &HB, &PS, &threads);
  const size_t sh = (size_t)PS * (4 + L.n) * HB * sizeof(float);
  return qc_dispatch_n<2, 5>(L.n, [&](auto n) {
    auto launch = [&](auto m) {
      hipLaunchKernelGGL((k_pre_bwd_ens<n(), m()>), dim3(nr + nv, e.M), dim3(threads), sh, st, Xr, Xv, prm, L, abr, abv, part,
                         part_stride, row0_r, row0_v, Br, Bv, HB, PS, nv, ajr, ajv, e);
    };
    if (map) launch(qc_int<1>{}); else launch(qc_int<0>{});
  });
}
