// Variational-circuit kernels, "reg" family (2 <= n <= 5), SEVEN derivative channels: the six of
// qc_circuit_reg_kernels.h and channel 6 = d2/dt2, for equations that are second order in time over two space
// dimensions (u_tt = c^2 (u_xx + u_yy); reference nn/pde.py:28-52 differentiates twice in time through the simulator).
//
//   jets_tt_fwd : angle jets[7][n][B]          -> <Z_w> jets[7][n][B]
//   jets_tt_bwd : angle jets, cot jets[7][n][B] -> d(angle jets)[7][n][B], d_theta partial rows
//
// A block is 7 waves x 64 points, wave c = channel c.  The direction of a channel and the second-order channel of a
// direction (t = 1, x = 2, y = 3):
//   dir(ch) = ch <= 3 ? ch : (ch == 6 ? 1 : ch - 2),      sec(d) = d == 1 ? 6 : d + 2.
// Forward: chi_ss is built from (a_s, a_ss) with the order-2 embedding series, and
//   q_ss[w] = 2 Re<chi_0|Z_w|chi_ss> + 2 <chi_s|Z_w|chi_s>,
// so the three first-order waves publish their 2 <chi|Z|chi> sums.  Adjoint: lam_0 = sum_c D_c chi_c over seven
// channels, lam_s = D_s chi_0 + 2 D_sec(s) chi_s, lam_ss = D_ss chi_0; the tail gives abar[s] = ip0(mu_s) + 2 ip1(mu_sec(s)),
// abar[ss] = ip0(mu_ss), abar[0] = the seven waves' own terms.  The final states are recomputed (nothing is kept
// between the two kernels), the gate program is run-time data (DynProg), angle encoding only.
#pragma once
#include "qc_circuit_reg_kernels.h"

#define QC_NCH_TT 7

namespace {

__device__ __forceinline__ int qc_tt_dir(int ch) { return ch <= 3 ? ch : (ch == 6 ? 1 : ch - 2); }
__device__ __forceinline__ int qc_tt_sec(int d) { return d == 1 ? 6 : d + 2; }

// first / second derivative of the embedding angles along channel `ch`'s direction for this lane's point
template <int N>
__device__ __forceinline__ void qc_tt_angle_jets(float (&da)[N], float (&dda)[N], int ch, const float* __restrict__ ajets,
                                                 int64_t B, int64_t pc) {
  const int dirch = qc_tt_dir(ch);
#pragma unroll
  for (int w = 0; w < N; ++w) {
    da[w] = ch >= 1 ? ajets[((int64_t)dirch * N + w) * B + pc] : 0.f;
    dda[w] = ch >= 4 ? ajets[((int64_t)ch * N + w) * B + pc] : 0.f;
  }
}

// Initial vector of channel `ch` (angle encoding; `cs`: the block's [cos | sin][N][64] table in LDS)
template <int N>
__device__ __forceinline__ void qc_tt_build_channel(SV<N>& v, int ch, const float* __restrict__ ajets, int64_t B, int64_t pc,
                                                    const float* cs) {
  float ca[N], sa[N], da[N], dda[N];
  load_sincos_lds<N>(ca, sa, cs);
  qc_tt_angle_jets<N>(da, dda, ch, ajets, B, pc);
  QcPk<(1 << N)> P0, P1, P2;
  if (ch == 0) {
    qc_embed_series<N, 0>(P0, P1, P2, ca, sa, da, dda);
    qc_phase_load<N>(v, P0);
  } else if (ch <= 3) {
    qc_embed_series<N, 1>(P0, P1, P2, ca, sa, da, dda);
    qc_phase_load<N>(v, P1);
  } else {
    qc_embed_series<N, 2>(P0, P1, P2, ca, sa, da, dda);
    qc_phase_load<N>(v, P2);
  }
}

template <class PG>
__global__ void __launch_bounds__(448) k_jets_tt_fwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                     const float* __restrict__ umat, int n_gates,
                                                     const float* __restrict__ ajets, float* __restrict__ qjets, int64_t B,
                                                     int absorb) {
  constexpr int N = PG::N;
  constexpr int A2 = 2 << N;                 // floats per statevector
  __shared__ float s_chi0[A2 * 64];          // [amplitude][lane] (re, im)
  __shared__ float s_sq[3 * N * 64];         // 2<chi_s|Z_w|chi_s> for s = t, x, y
  __shared__ float s_cs[2 * N * 64];         // half-angle cos | sin of the block's 64 points, one wire per wave
  const int lane = threadIdx.x & 63;
  const int ch = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave index = channel (scalar)
  const int64_t p = (int64_t)blockIdx.x * 64 + lane;
  const int64_t pc = p < B ? p : B - 1;

  if (ch < N) qc_wire_sincos(s_cs[ch * 64 + lane], s_cs[(N + ch) * 64 + lane], ajets, B, pc, ch, trig, absorb);
  __syncthreads();
  SV<N> v[1];
  qc_tt_build_channel<N>(v[0], ch, ajets, B, pc, s_cs);
  PG::fwd(v, prog, trig, umat, n_gates, absorb);

  QcPk<(1 << N)> t;
  float q[N];
  qf2* s_x0 = reinterpret_cast<qf2*>(s_chi0);   // [amplitude][lane]
  if (ch <= 3) {
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) {
      if (ch == 0) s_x0[k * 64 + lane] = v[0].a[k];
      const qf2 m = v[0].a[k] * v[0].a[k];
      t[k] = m.x + m.y;
    }
    qc_signed_sums<N>(q, t);
    if (ch != 0) {
#pragma unroll
      for (int w = 0; w < N; ++w) s_sq[((ch - 1) * N + w) * 64 + lane] = 2.f * q[w];
    }
  }
  __syncthreads();
  if (ch != 0) {
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) {
      const qf2 m = s_x0[k * 64 + lane] * v[0].a[k];   // Re(conj(chi_0) chi_c)
      t[k] = m.x + m.y;
    }
    qc_signed_sums<N>(q, t);
#pragma unroll
    for (int w = 0; w < N; ++w) q[w] *= 2.f;
    if (ch >= 4) {
      const int d = qc_tt_dir(ch);
#pragma unroll
      for (int w = 0; w < N; ++w) q[w] += s_sq[((d - 1) * N + w) * 64 + lane];
    }
  }
  if (p < B) {
#pragma unroll
    for (int w = 0; w < N; ++w) qjets[((int64_t)ch * N + w) * B + p] = q[w];
  }
}

// dynamic LDS: [7][A2][64] exchange of the recomputed final states (reused as [7 waves][3][N][64] by the tail),
// [7 waves][n_params] gradient accumulators, [cos | sin][N][64]
template <class PG>
__global__ void __launch_bounds__(448) k_jets_tt_bwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                     const float* __restrict__ umat, int n_gates, int n_params,
                                                     const float* __restrict__ ajets, const float* __restrict__ qbar,
                                                     float* __restrict__ abar, float* __restrict__ part, int64_t part_stride,
                                                     int64_t row0, int64_t B, int absorb) {
  constexpr int N = PG::N;
  constexpr int A2 = 2 << N;
  constexpr int NW = QC_NCH_TT;
  static_assert(3 * N <= A2, "the tail's [3][N] rows of a wave fit its slice of the exchange region");
  extern __shared__ float smem[];
  float* s_chi = smem;                       // [7][A2][64]
  float* s_acc = smem + NW * A2 * 64;        // [7 waves][n_params]
  float* s_cs = s_acc + NW * n_params;       // [cos | sin][N][64]
  const int lane = threadIdx.x & 63;
  const int ch = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < NW * n_params; i += 64 * NW) s_acc[i] = 0.f;
  const int64_t bid = blockIdx.x;
  const int64_t p = bid * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  if (ch < N) qc_wire_sincos(s_cs[ch * 64 + lane], s_cs[(N + ch) * 64 + lane], ajets, B, pc, ch, trig, absorb);
  __syncthreads();

  SV<N> cl[2];   // [0] = chi, [1] = lambda
  {
    SV<N> v[1];
    qc_tt_build_channel<N>(v[0], ch, ajets, B, pc, s_cs);
    PG::template fwd<-1, true>(v, prog, trig, umat, n_gates, absorb);
    cl[0] = v[0];
  }
  {
    qf2* mine = reinterpret_cast<qf2*>(s_chi) + ch * (A2 / 2) * 64;
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) mine[k * 64 + lane] = cl[0].a[k];
  }
  __syncthreads();
  auto other = [&](int c, int k) -> qf2 { return reinterpret_cast<const qf2*>(s_chi)[(c * (A2 / 2) + k) * 64 + lane]; };
  auto dvec = [&](int c, QcPk<(1 << N)>& d) {
    float qb[N];
#pragma unroll
    for (int w = 0; w < N; ++w) qb[w] = live ? qbar[((int64_t)c * N + w) * B + pc] : 0.f;
    qc_sign_sums<N>(d, qb);
  };
  QcPk<(1 << N)> d;
  if (ch == 0) {
    dvec(0, d);
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_dup(d[k]) * cl[0].a[k];
#pragma unroll 1
    for (int c = 1; c < NW; ++c) {   // one channel at a time: keeps the live set at one vector
      dvec(c, d);
#pragma unroll
      for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_pk_fma(qc_dup(d[k]), other(c, k), cl[1].a[k]);
    }
  } else {
    dvec(ch, d);
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_dup(d[k]) * other(0, k);
    if (ch <= 3) {
      dvec(qc_tt_sec(ch), d);
#pragma unroll
      for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_pk_fma(qc_dup(2.f * d[k]), cl[0].a[k], cl[1].a[k]);
    }
  }
  __syncthreads();  // everyone is done reading s_chi

  PG::bwd(cl, prog, trig, umat, n_gates, s_acc + ch * n_params, lane, absorb);

  // cotangents of the angle jets in the frame pulled back through the embedding (qc_gates.h)
  const float* aj = qc_launder(ajets);
  float ca[N], sa[N], da[N], dda[N];
  load_sincos_lds<N>(ca, sa, s_cs);
  qc_unembed<N>(cl[1], ca, sa);
  qc_tt_angle_jets<N>(da, dda, ch, aj, B, pc);
  float* buf = s_chi + ch * 3 * N * 64;  // [3][N][64] per wave
  float T[N];
  if (ch == 0) {
    qc_pull_ip0<N>(T, cl[1]);
#pragma unroll
    for (int w = 0; w < N; ++w) buf[(0 * N + w) * 64 + lane] = T[w];
  } else if (ch <= 3) {
    qc_pull_ip1<N>(T, cl[1], da);
#pragma unroll
    for (int w = 0; w < N; ++w) buf[(0 * N + w) * 64 + lane] = T[w];
    qc_pull_ip0<N>(T, cl[1]);
#pragma unroll
    for (int w = 0; w < N; ++w) buf[(1 * N + w) * 64 + lane] = T[w];
  } else {
    qc_pull_ip2<N>(T, cl[1], da, dda);
#pragma unroll
    for (int w = 0; w < N; ++w) buf[(0 * N + w) * 64 + lane] = T[w];
    qc_pull_ip1<N>(T, cl[1], da);
#pragma unroll
    for (int w = 0; w < N; ++w) buf[(1 * N + w) * 64 + lane] = 2.f * T[w];
    qc_pull_ip0<N>(T, cl[1]);
#pragma unroll
    for (int w = 0; w < N; ++w) buf[(2 * N + w) * 64 + lane] = T[w];
  }
  __syncthreads();
  auto at = [&](int wv, int slot, int w) { return s_chi[((wv * 3 + slot) * N + w) * 64 + lane]; };
#pragma unroll
  for (int w = 0; w < N; ++w) {
    float r;
    if (ch == 0)
      r = (((at(0, 0, w) + at(1, 0, w)) + (at(2, 0, w) + at(3, 0, w))) + (at(4, 0, w) + at(5, 0, w))) + at(6, 0, w);
    else if (ch <= 3)
      r = at(ch, 1, w) + at(qc_tt_sec(ch), 1, w);
    else
      r = at(ch, 2, w);
    if (live) abar[((int64_t)ch * N + w) * B + p] = r;
    if (absorb && ch == 0) {   // folded RX layer: d L / d theta_w = sum over points of d L / d angle_w
      const float tot = qc_wave_sum6_to_lane63(live ? r : 0.f);
      if (lane == 63) s_acc[prog[w].slot] += tot;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_params; i += 64 * NW) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < NW; ++wv) s += s_acc[wv * n_params + i];
    part[(row0 + bid) * part_stride + i] = s;
  }
}

}  // namespace
