// Variational-circuit kernels, "reup" family: 2 <= n <= 5 qubits, gate programs that hold EMBED gates (data
// re-uploading, Perez-Salinas et al. 2020): RX(a_w(X)) on wire w in the middle of the program, with the same per-point
// angle a_w (and angle jet) as the implicit embedding in front of the program.
//
// The kernels are run-time-program interpreters with the block shapes of the register family (qc_circuit_reg_kernels.h):
// one lane = one statevector in VGPRs; value kernels one vector per lane, jet kernels six waves = six channels.  Between
// EMBED gates a segment runs through DynProg<N>; a run of consecutive EMBED gates on distinct wires (a layer, or any part
// of one: wire mask m) is one exchange through LDS.  With G_v = -i X_v / 2, A_k = sum_{v in m} da_{v,k} G_v,
// AA_kk = sum_{v in m} dda_{v,kk} G_v and U = prod_{v in m} RX(a_v) (all commute):
//   chi_0'  = U chi_0
//   chi_k'  = U (chi_k  + A_k chi_0)                                   k  = t, x, y
//   chi_kk' = U (chi_kk + 2 A_k chi_k + (A_k^2 + AA_kk) chi_0)          kk = xx, yy
// and backwards from (chi_c', lam_c'), T(L, f) = Im <L| X_w |f>:
//   abar_w      += sum_c T(lam_c', chi_c')
//   abar_{w,k}  += T(lam_k', chi_0') + 2 T(lam_kk', chi_k')
//   abar_{w,kk} += T(lam_kk', chi_0')
//   chi_k  = U^+ (chi_k' - A_k chi_0'),  chi_kk = U^+ (chi_kk' - 2 A_k chi_k' + (A_k^2 - AA_kk) chi_0')
//   lam_kk = U^+ lam_kk',  lam_k = U^+ (lam_k' - 2 A_k lam_kk'),
//   lam_0  = U^+ (lam_0' - sum_k A_k lam_k' + sum_kk (A_k^2 - AA_kk) lam_kk')
// The adjoint kernels recompute the forward sweep (no kept states).  Gate gradients reach the tile's partial row in gate
// order through one LDS row per wave; no float atomics.
//
// SCALED (a program with at least one EMBED_S gate, RX(s_v a_v) with s_v = theta[slot] = trig[g].th; a plain EMBED gate
// in such a program has s_v = 1 and no gradient): all of the above with the effective angle b_v = s_v a_v per gate of the
// run.  The half-angle cos / sin of a run are those of b_v (not the block's one s_cs table: the jet kernels compute them
// once per run, wire and point and share them through LDS, the value kernels per lane), da_{v,k} and dda_{v,kk} become
// db_{v,k} = s_v da_{v,k} and ddb_{v,kk} = s_v dda_{v,kk}, and the run's T terms are the cotangents bbar of b.  At the end
// of each run
//   abar_{v,c} += s_v bbar_{v,c},   dL/ds_v = sum_points sum_c bbar_{v,c} a_{v,c}
// where each wave forms its share t0 a_{v,0} + t1 a_{v,dir} + t2 a_{v,ch} per lane, sums it over the wave and adds it to
// its own LDS row at the gate's slot, like a gate gradient.  The SCALED = false instantiations are the kernels of a
// program without EMBED_S gates, instruction for instruction what they were before the parameter existed.
#pragma once
#include "qc_circuit_reg_kernels.h"

namespace {

// an embedding gate of the program: EMBED, and in a SCALED program EMBED_S as well
template <bool SCALED>
__device__ __forceinline__ bool reup_is_embed(int op) {
  if constexpr (SCALED) return op == QC_EMBED || op == QC_EMBED_S;
  else return op == QC_EMBED;
}
// first embedding gate at or after g (n_gates if none) / last embedding gate before g (-1 if none)
template <bool SCALED = false>
__device__ __forceinline__ int reup_next(const QcGate* __restrict__ prog, int g, int n_gates) {
  while (g < n_gates && !reup_is_embed<SCALED>(prog[g].op)) ++g;
  return g;
}
template <bool SCALED = false>
__device__ __forceinline__ int reup_prev(const QcGate* __restrict__ prog, int g) {
  --g;
  while (g >= 0 && !reup_is_embed<SCALED>(prog[g].op)) --g;
  return g;
}
// the run of embedding gates on distinct wires that starts at e (forwards) / ends at e (backwards): wire mask, next index
template <int N, bool SCALED = false>
__device__ __forceinline__ int reup_run_fwd(const QcGate* __restrict__ prog, int e, int n_gates, int& mask) {
  mask = 0;
  while (e < n_gates) {
    const QcGate g = prog[e];
    const int bit = 1 << (N - 1 - g.ba);
    if (!reup_is_embed<SCALED>(g.op) || (mask & bit)) break;
    mask |= bit;
    ++e;
  }
  return e;
}
template <int N, bool SCALED = false>
__device__ __forceinline__ int reup_run_bwd(const QcGate* __restrict__ prog, int e, int& mask) {
  mask = 0;
  while (e >= 0) {
    const QcGate g = prog[e];
    const int bit = 1 << (N - 1 - g.ba);
    if (!reup_is_embed<SCALED>(g.op) || (mask & bit)) break;
    mask |= bit;
    --e;
  }
  return e;
}

// RX(a_w) (ADJ: its adjoint) on the wires of `mask`, the lane's own half-angle cos / sin
template <int N, int K, bool ADJ, int W = 0>
__device__ __forceinline__ void reup_rx(SV<N> (&v)[K], int mask, const float (&ca)[N], const float (&sa)[N]) {
  if constexpr (W < N) {
    if ((mask >> W) & 1) {
#pragma unroll
      for (int q = 0; q < K; ++q) g_rx<N, N - 1 - W>(v[q], ca[W], ADJ ? -sa[W] : sa[W]);
    }
    reup_rx<N, K, ADJ, W + 1>(v, mask, ca, sa);
  }
}
// T[w] += Im <lam| X_w |chi> on the wires of `mask`, both vectors in registers
template <int N, int W = 0>
__device__ __forceinline__ void reup_ip(float (&T)[N], int mask, const SV<N>& lam, const SV<N>& chi) {
  if constexpr (W < N) {
    if ((mask >> W) & 1) T[W] += ip_x<N, N - 1 - W>(lam, chi);
    reup_ip<N, W + 1>(T, mask, lam, chi);
  }
}
// T[w] += sc * Im <lam| X_w |src> on the wires of `mask`, src a published vector: [amplitude][lane] in LDS
template <int N>
__device__ __forceinline__ void reup_ip_lds(float (&T)[N], int mask, const SV<N>& lam, const qf2* src, int lane, float sc) {
#pragma unroll
  for (int w = 0; w < N; ++w) {
    if (!((mask >> w) & 1)) continue;
    qf2 acc = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) acc = qc_pk_fma(lam.a[k], qc_swp(src[(k ^ (1 << (N - 1 - w))) * 64 + lane]), acc);
    T[w] = fmaf(sc, acc.x - acc.y, T[w]);
  }
}
// v += sc * (sum_w coef_w G_w) src,  G_w = -i X_w / 2: an index permutation of the published vector times -i/2
// (a wire outside the run's mask comes with a zero coefficient and is NOT skipped: a branch per wire was built and keeps the
// compiler from pairing the LDS reads of neighbouring passes - at N = 5 the forward kernel's scratch went from 204 to 460
// bytes per lane, the adjoint's from 432 to 556 - and whole layers, all that build_program emits, have no such wire)
template <int N>
__device__ __forceinline__ void reup_gen1(SV<N>& v, const qf2* src, int lane, const float (&coef)[N], float sc) {
#pragma unroll
  for (int w = 0; w < N; ++w) {
    const qf2 cw = qc_pm(0.5f * sc * coef[w]);   // (-i/2)(x + i y) = (y - i x) / 2
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) v.a[k] = qc_pk_fma(cw, qc_swp(src[(k ^ (1 << (N - 1 - w))) * 64 + lane]), v.a[k]);
  }
}
// v += sc * (sum_w coef_w G_w)^2 src = -sc/4 [ (sum_w coef_w^2) src + 2 sum_{u<w} coef_u coef_w X_u X_w src ]
template <int N>
__device__ __forceinline__ void reup_gen2(SV<N>& v, const qf2* src, int lane, const float (&coef)[N], float sc) {
  float S = 0.f;
#pragma unroll
  for (int w = 0; w < N; ++w) S = fmaf(coef[w], coef[w], S);
  const qf2 c0 = qc_dup(-0.25f * sc * S);
#pragma unroll
  for (int k = 0; k < (1 << N); ++k) v.a[k] = qc_pk_fma(c0, src[k * 64 + lane], v.a[k]);
#pragma unroll
  for (int u = 0; u < N; ++u) {
#pragma unroll
    for (int w = u + 1; w < N; ++w) {
      const qf2 cuw = qc_dup(-0.5f * sc * coef[u] * coef[w]);
#pragma unroll
      for (int k = 0; k < (1 << N); ++k)
        v.a[k] = qc_pk_fma(cuw, src[(k ^ (1 << (N - 1 - u)) ^ (1 << (N - 1 - w))) * 64 + lane], v.a[k]);
    }
  }
}
// channel `c`'s row of the angle jets on the wires of `mask` (0 elsewhere)
template <int N>
__device__ __forceinline__ void reup_coef(float (&co)[N], int mask, int c, const float* __restrict__ ajets, int64_t B, int64_t pc) {
#pragma unroll
  for (int w = 0; w < N; ++w) co[w] = ((mask >> w) & 1) ? ajets[((int64_t)c * N + w) * B + pc] : 0.f;
}

// ---- SCALED programs
// the input scaling of embedding gate gi: theta[slot] of an EMBED_S gate (the trig table's `th`), 1 for a plain EMBED gate
__device__ __forceinline__ float reup_scale(const QcGate& g, const QcTrig* __restrict__ trig, int gi) {
  return g.op == QC_EMBED_S ? trig[gi].th : 1.f;
}
// wave w < N: half-angle cos / sin of wire w's scaled angle sc_w a_w for the block's 64 points, into the run's table.
// (a branch per wire on the wave-uniform index: a select chain over the register array `sc` is turned into a private
// array with a run-time index by the compiler)
template <int N>
__device__ __forceinline__ void reup_run_sincos(float* s_rcs, int ch, const float (&sc)[N], const float* __restrict__ ajets,
                                                int64_t B, int64_t pc, int lane) {
#pragma unroll
  for (int w = 0; w < N; ++w) {
    if (ch == w) {
      float c1, s1;
      sincosf(0.5f * sc[w] * ajets[(int64_t)w * B + pc], &s1, &c1);
      s_rcs[w * 64 + lane] = c1;
      s_rcs[(N + w) * 64 + lane] = s1;
    }
  }
}
// per-wire scalings of the run of gates [g0, g1) (0 on a wire outside the run)
template <int N>
__device__ __forceinline__ void reup_run_scales(float (&sc)[N], const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                int g0, int g1) {
#pragma unroll
  for (int w = 0; w < N; ++w) sc[w] = 0.f;
  for (int gi = g0; gi < g1; ++gi) {
    const QcGate g = prog[gi];
    const float s = reup_scale(g, trig, gi);
#pragma unroll
    for (int w = 0; w < N; ++w) sc[w] = (N - 1 - g.ba == w) ? s : sc[w];
  }
}
// channel `c`'s row of the jets of the effective angles b_w = sc_w a_w
template <int N>
__device__ __forceinline__ void reup_coef_s(float (&co)[N], int mask, int c, const float (&sc)[N], const float* __restrict__ ajets,
                                            int64_t B, int64_t pc) {
  reup_coef<N>(co, mask, c, ajets, B, pc);
#pragma unroll
  for (int w = 0; w < N; ++w) co[w] *= sc[w];
}
// RX(sc a_w) (ADJ: its adjoint) of one embedding gate, the half-angle cos / sin formed by the lane
template <int N, int K, bool ADJ>
__device__ __forceinline__ void reup_rx_lane(SV<N> (&v)[K], int w, float sc, const float* __restrict__ angles, int64_t B, int64_t pc) {
  float c1, s1;
  sincosf(0.5f * sc * angles[(int64_t)w * B + pc], &s1, &c1);
  float cb[N], sb[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    cb[k] = c1;
    sb[k] = s1;
  }
  reup_rx<N, K, ADJ>(v, 1 << w, cb, sb);
}

// ================================================================== value channel only
template <int N>
__device__ __forceinline__ void reup_value_sweep(SV<N> (&v)[1], const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                 const float* __restrict__ umat, int n_gates, const float (&ca)[N],
                                                 const float (&sa)[N]) {
  int g = 0;
  while (true) {
    const int e = reup_next(prog, g, n_gates);
    DynProg<N>::template fwd<0, true>(v, prog + g, trig + g, umat, e - g, 0);
    if (e >= n_gates) break;
    reup_rx<N, 1, false>(v, 1 << (N - 1 - prog[e].ba), ca, sa);
    g = e + 1;
  }
}

// SCALED: every embedding gate with its own scaling
template <int N>
__device__ __forceinline__ void reup_value_sweep_s(SV<N> (&v)[1], const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                   const float* __restrict__ umat, int n_gates, const float* __restrict__ angles,
                                                   int64_t B, int64_t pc) {
  int g = 0;
  while (true) {
    const int e = reup_next<true>(prog, g, n_gates);
    DynProg<N>::template fwd<0, true>(v, prog + g, trig + g, umat, e - g, 0);
    if (e >= n_gates) break;
    const QcGate ge = prog[e];
    reup_rx_lane<N, 1, false>(v, N - 1 - ge.ba, reup_scale(ge, trig, e), angles, B, pc);
    g = e + 1;
  }
}

template <int N, bool SCALED>
__global__ void __launch_bounds__(256) k_reup_value_fwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                        const float* __restrict__ umat, int n_gates,
                                                        const float* __restrict__ angles, float* __restrict__ expval, int64_t B) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t pc = p < B ? p : B - 1;
  float ca[N], sa[N];
  load_sincos<N, 0>(ca, sa, angles, B, pc, trig, 0);
  SV<N> v[1];
  build_channel<N, 0>(v[0], 0, angles, B, pc, 0, trig, 0);
  if constexpr (SCALED) reup_value_sweep_s<N>(v, prog, trig, umat, n_gates, angles, B, pc);
  else reup_value_sweep<N>(v, prog, trig, umat, n_gates, ca, sa);
  QcPk<(1 << N)> t;
  float q[N];
#pragma unroll
  for (int k = 0; k < (1 << N); ++k) {
    const qf2 m = v[0].a[k] * v[0].a[k];
    t[k] = m.x + m.y;
  }
  qc_signed_sums<N>(q, t);
  if (p < B) {
#pragma unroll
    for (int w = 0; w < N; ++w) expval[(int64_t)w * B + p] = q[w];
  }
}

template <int N, bool SCALED>
__global__ void __launch_bounds__(256) k_reup_value_bwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                        const float* __restrict__ umat, int n_gates, int n_params,
                                                        const float* __restrict__ angles, const float* __restrict__ cot,
                                                        float* __restrict__ d_angles, float* __restrict__ part,
                                                        int64_t part_stride, int64_t row0, int64_t B) {
  extern __shared__ float smem[];  // [4 waves][n_params]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < 4 * n_params; i += 256) smem[i] = 0.f;
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  float ca[N], sa[N];
  load_sincos<N, 0>(ca, sa, angles, B, pc, trig, 0);
  SV<N> cl[2];  // [0] = chi, [1] = lambda
  {
    SV<N> v[1];
    build_channel<N, 0>(v[0], 0, angles, B, pc, 0, trig, 0);
    if constexpr (SCALED) reup_value_sweep_s<N>(v, prog, trig, umat, n_gates, angles, B, pc);
    else reup_value_sweep<N>(v, prog, trig, umat, n_gates, ca, sa);
    cl[0] = v[0];
  }
  {
    float qb[N];
#pragma unroll
    for (int w = 0; w < N; ++w) qb[w] = live ? cot[(int64_t)w * B + pc] : 0.f;
    QcPk<(1 << N)> d;
    qc_sign_sums<N>(d, qb);
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_dup(d[k]) * cl[0].a[k];
  }
  float T[N];   // cotangents of the angles: the EMBED gates' terms, then the first embedding's
#pragma unroll
  for (int w = 0; w < N; ++w) T[w] = 0.f;
  int g1 = n_gates;
  while (true) {
    const int e = reup_prev<SCALED>(prog, g1);
    DynProg<N>::template bwd<0>(cl, prog + e + 1, trig + e + 1, umat, g1 - e - 1, smem + wave * n_params, lane, 0);
    if (e < 0) break;
    if constexpr (SCALED) {
      const QcGate ge = prog[e];
      const int w = N - 1 - ge.ba;
      const float sc = reup_scale(ge, trig, e);
      float Tb[N];   // cotangent of b_w = sc a_w (0 on the other wires)
#pragma unroll
      for (int k = 0; k < N; ++k) Tb[k] = 0.f;
      reup_ip<N>(Tb, 1 << w, cl[1], cl[0]);
#pragma unroll
      for (int k = 0; k < N; ++k) T[k] = fmaf(sc, Tb[k], T[k]);
      if (ge.op == QC_EMBED_S) {
        float tb = Tb[0];   // (0 on every wire but w)
#pragma unroll
        for (int k = 1; k < N; ++k) tb += Tb[k];
        const float gr = qc_wave_sum6_to_lane63(live ? tb * angles[(int64_t)w * B + pc] : 0.f);
        if (lane == 63) smem[wave * n_params + ge.slot] += gr;
      }
      reup_rx_lane<N, 2, true>(cl, w, sc, angles, B, pc);
    } else {
      const int m = 1 << (N - 1 - prog[e].ba);
      reup_ip<N>(T, m, cl[1], cl[0]);
      reup_rx<N, 2, true>(cl, m, ca, sa);
    }
    g1 = e;
  }
  {
    float T0[N];
    QcPk<(1 << N)> Q0, Q1, Q2;
    channel_series<N, 0>(Q0, Q1, Q2, 0, qc_launder(angles), B, pc, trig, 0);
    qc_embed_ip<N>(T0, cl[1], Q0);
#pragma unroll
    for (int w = 0; w < N; ++w) T[w] += T0[w];
  }
  if (live) {
#pragma unroll
    for (int w = 0; w < N; ++w) d_angles[(int64_t)w * B + p] = T[w];
  }
  __syncthreads();
  const int64_t tile = (int64_t)blockIdx.x * 4 + wave;   // one partial row per 64-point tile
  if (tile * 64 < B)
    for (int i = lane; i < n_params; i += 64) part[(row0 + tile) * part_stride + i] = smem[wave * n_params + i];
}

// ================================================================== six derivative channels
// The <Z> jets at the end of k_reup_jets_fwd, and in k_reup_jets_bwd the cotangents of the final states and the pulled-back
// tail of the first embedding, RESTATE the corresponding parts of k_jets_fwd_body / k_jets_bwd_body<PG, false>
// (qc_circuit_reg_kernels.h) instead of sharing a helper with them, so that the register family's kernels keep their
// instruction streams: a fix to one copy belongs in the other as well.
// One run of EMBED gates, forwards.  s_pub: [3][2^N][64] amplitudes (chi_0, chi_x, chi_y before the run).
template <int N>
__device__ __forceinline__ void reup_layer_fwd(SV<N> (&v)[1], int ch, int mask, float* s_pub, const float* s_cs,
                                               const float* __restrict__ ajets, int64_t B, int64_t pc, int lane) {
  constexpr int NA = 1 << N;
  qf2* pub = reinterpret_cast<qf2*>(s_pub);
  __syncthreads();   // the last run's readers are done
  if (ch == 0 || ch == 2 || ch == 3) {
    qf2* mine = pub + (ch == 0 ? 0 : ch - 1) * NA * 64;
#pragma unroll
    for (int k = 0; k < NA; ++k) mine[k * 64 + lane] = v[0].a[k];
  }
  __syncthreads();
  if (ch >= 1) {
    float da[N];
    reup_coef<N>(da, mask, ch <= 3 ? ch : ch - 2, ajets, B, pc);
    if (ch <= 3) {
      reup_gen1<N>(v[0], pub, lane, da, 1.f);
    } else {
      float dda[N];
      reup_coef<N>(dda, mask, ch, ajets, B, pc);
      reup_gen1<N>(v[0], pub + (ch - 3) * NA * 64, lane, da, 2.f);
      reup_gen1<N>(v[0], pub, lane, dda, 1.f);
      reup_gen2<N>(v[0], pub, lane, da, 1.f);
    }
  }
  float ca[N], sa[N];
  load_sincos_lds<N>(ca, sa, s_cs);
  reup_rx<N, 1, false>(v, mask, ca, sa);
}

// SCALED: the run with per-wire scalings sc.  s_rcs: [cos | sin][N][64], the run's half-angle cos / sin of b_w = sc_w a_w,
// wave w computes wire w (sc_w = 0 outside the run: the identity, and never applied)
template <int N>
__device__ __forceinline__ void reup_layer_fwd_s(SV<N> (&v)[1], int ch, int mask, const float (&sc)[N], float* s_pub, float* s_rcs,
                                                 const float* __restrict__ ajets, int64_t B, int64_t pc, int lane) {
  constexpr int NA = 1 << N;
  qf2* pub = reinterpret_cast<qf2*>(s_pub);
  __syncthreads();   // the last run's readers are done, with s_rcs too
  if (ch == 0 || ch == 2 || ch == 3) {
    qf2* mine = pub + (ch == 0 ? 0 : ch - 1) * NA * 64;
#pragma unroll
    for (int k = 0; k < NA; ++k) mine[k * 64 + lane] = v[0].a[k];
  }
  reup_run_sincos<N>(s_rcs, ch, sc, ajets, B, pc, lane);
  __syncthreads();
  if (ch >= 1) {
    float da[N];
    reup_coef_s<N>(da, mask, ch <= 3 ? ch : ch - 2, sc, ajets, B, pc);
    if (ch <= 3) {
      reup_gen1<N>(v[0], pub, lane, da, 1.f);
    } else {
      float dda[N];
      reup_coef_s<N>(dda, mask, ch, sc, ajets, B, pc);
      reup_gen1<N>(v[0], pub + (ch - 3) * NA * 64, lane, da, 2.f);
      reup_gen1<N>(v[0], pub, lane, dda, 1.f);
      reup_gen2<N>(v[0], pub, lane, da, 1.f);
    }
  }
  float ca[N], sa[N];
  load_sincos_lds<N>(ca, sa, s_rcs);
  reup_rx<N, 1, false>(v, mask, ca, sa);
}

// s_rcs: the SCALED runs' cos / sin table (unused otherwise)
template <int N, bool SCALED>
__device__ __forceinline__ void reup_jets_sweep(SV<N> (&v)[1], int ch, const QcGate* __restrict__ prog,
                                                const QcTrig* __restrict__ trig, const float* __restrict__ umat, int n_gates,
                                                float* s_pub, const float* s_cs, float* s_rcs, const float* __restrict__ ajets,
                                                int64_t B, int64_t pc, int lane) {
  int g = 0;
  while (true) {
    const int e = reup_next<SCALED>(prog, g, n_gates);
    DynProg<N>::template fwd<0, true>(v, prog + g, trig + g, umat, e - g, 0);
    if (e >= n_gates) break;
    int mask;
    g = reup_run_fwd<N, SCALED>(prog, e, n_gates, mask);
    if constexpr (SCALED) {
      float sc[N];
      reup_run_scales<N>(sc, prog, trig, e, g);
      reup_layer_fwd_s<N>(v, ch, mask, sc, s_pub, s_rcs, ajets, B, pc, lane);
    } else {
      reup_layer_fwd<N>(v, ch, mask, s_pub, s_cs, ajets, B, pc, lane);
    }
  }
}

template <int N, bool SCALED>
__global__ void __launch_bounds__(384) k_reup_jets_fwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                       const float* __restrict__ umat, int n_gates,
                                                       const float* __restrict__ ajets, float* __restrict__ qjets, int64_t B) {
  constexpr int A2 = 2 << N;
  __shared__ float s_pub[3 * A2 * 64];       // [3][amp*2+{re,im}][lane]; slot 0 again for the final chi_0
  __shared__ float s_sq[2 * N * 64];         // 2<chi_k|Z_w|chi_k> for k = x, y
  __shared__ float s_cs[2 * N * 64];         // half-angle cos | sin of the block's 64 points, one wire per wave
  float* s_rcs = nullptr;
  if constexpr (SCALED) {
    __shared__ float s_run_cs[2 * N * 64];   // the same of the scaled angles of one run
    s_rcs = s_run_cs;
  }
  const int lane = threadIdx.x & 63;
  const int ch = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave index = channel (scalar)
  const int64_t p = (int64_t)blockIdx.x * 64 + lane;
  const int64_t pc = p < B ? p : B - 1;
  if (ch < N) qc_wire_sincos<0>(s_cs[ch * 64 + lane], s_cs[(N + ch) * 64 + lane], ajets, B, pc, ch, trig, 0);
  __syncthreads();
  SV<N> v[1];
  build_channel<N, 0>(v[0], ch, ajets, B, pc, 0, trig, 0, s_cs);
  reup_jets_sweep<N, SCALED>(v, ch, prog, trig, umat, n_gates, s_pub, s_cs, s_rcs, ajets, B, pc, lane);
  __syncthreads();   // the last run's readers are done with slot 0

  QcPk<(1 << N)> t;
  float q[N];
  qf2* s_x0 = reinterpret_cast<qf2*>(s_pub);   // [amplitude][lane]
  if (ch == 0) {
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) {
      s_x0[k * 64 + lane] = v[0].a[k];
      const qf2 m = v[0].a[k] * v[0].a[k];
      t[k] = m.x + m.y;
    }
    qc_signed_sums<N>(q, t);
  } else if (ch == 2 || ch == 3) {
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) {
      const qf2 m = v[0].a[k] * v[0].a[k];
      t[k] = m.x + m.y;
    }
    qc_signed_sums<N>(q, t);
#pragma unroll
    for (int w = 0; w < N; ++w) s_sq[((ch - 2) * N + w) * 64 + lane] = 2.f * q[w];
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
#pragma unroll
      for (int w = 0; w < N; ++w) q[w] += s_sq[((ch - 4) * N + w) * 64 + lane];
    }
  }
  if (p < B) {
#pragma unroll
    for (int w = 0; w < N; ++w) qjets[((int64_t)ch * N + w) * B + p] = q[w];
  }
}

// One run of EMBED gates, backwards from (chi_c', lam_c') = cl of wave c.  s_x: [6][2^N][64] amplitudes, the six chi'
// in the first phase, the six lam' in the second.  T0 / T1 / T2: this wave's terms of abar_w, of abar_{w,k} (its
// direction) and of abar_{w,kk} (its channel), as the tail of the kernel sums them.
template <int N>
__device__ __forceinline__ void reup_layer_bwd(SV<N> (&cl)[2], int ch, int mask, float* s_x, const float* s_cs,
                                               const float* __restrict__ ajets, int64_t B, int64_t pc, int lane,
                                               float (&T0)[N], float (&T1)[N], float (&T2)[N]) {
  constexpr int NA = 1 << N;
  qf2* x = reinterpret_cast<qf2*>(s_x);
  qf2* mine = x + ch * NA * 64;
  __syncthreads();   // whoever read s_x before is done
#pragma unroll
  for (int k = 0; k < NA; ++k) mine[k * 64 + lane] = cl[0].a[k];
  __syncthreads();
  reup_ip<N>(T0, mask, cl[1], cl[0]);
  if (ch >= 1 && ch <= 3) {
    float da[N];
    reup_coef<N>(da, mask, ch, ajets, B, pc);
    reup_ip_lds<N>(T1, mask, cl[1], x, lane, 1.f);
    reup_gen1<N>(cl[0], x, lane, da, -1.f);
  } else if (ch >= 4) {
    float da[N], dda[N];
    reup_coef<N>(da, mask, ch - 2, ajets, B, pc);
    reup_coef<N>(dda, mask, ch, ajets, B, pc);
    const qf2* xk = x + (ch - 2) * NA * 64;
    reup_ip_lds<N>(T1, mask, cl[1], xk, lane, 2.f);
    reup_ip_lds<N>(T2, mask, cl[1], x, lane, 1.f);
    reup_gen1<N>(cl[0], xk, lane, da, -2.f);
    reup_gen1<N>(cl[0], x, lane, dda, -1.f);
    reup_gen2<N>(cl[0], x, lane, da, 1.f);
  }
  __syncthreads();   // chi' read by everyone
#pragma unroll
  for (int k = 0; k < NA; ++k) mine[k * 64 + lane] = cl[1].a[k];
  __syncthreads();
  if (ch == 2 || ch == 3) {
    float da[N];
    reup_coef<N>(da, mask, ch, ajets, B, pc);
    reup_gen1<N>(cl[1], x + (ch + 2) * NA * 64, lane, da, -2.f);
  } else if (ch == 0) {
#pragma unroll 1
    for (int k = 1; k <= 3; ++k) {   // one direction at a time: keeps the live set small
      float da[N];
      reup_coef<N>(da, mask, k, ajets, B, pc);
      reup_gen1<N>(cl[1], x + k * NA * 64, lane, da, -1.f);
      if (k >= 2) {
        float dda[N];
        reup_coef<N>(dda, mask, k + 2, ajets, B, pc);
        reup_gen2<N>(cl[1], x + (k + 2) * NA * 64, lane, da, 1.f);
        reup_gen1<N>(cl[1], x + (k + 2) * NA * 64, lane, dda, -1.f);
      }
    }
  }
  float ca[N], sa[N];
  load_sincos_lds<N>(ca, sa, s_cs);
  reup_rx<N, 2, true>(cl, mask, ca, sa);
}

// SCALED: the run of gates [g0, g1) backwards.  t0 / t1 / t2 are the run's terms for the effective angles b; they are folded
// into T0 / T1 / T2 with the wires' scalings, and into the scalings' gradients (acc_wave, this wave's LDS row), as soon as
// they are complete.
template <int N>
__device__ __forceinline__ void reup_layer_bwd_s(SV<N> (&cl)[2], int ch, int mask, const QcGate* __restrict__ prog,
                                                 const QcTrig* __restrict__ trig, int g0, int g1, float* s_x, float* s_rcs,
                                                 const float* __restrict__ ajets, int64_t B, int64_t pc, int lane, bool live,
                                                 float* acc_wave, float (&T0)[N], float (&T1)[N], float (&T2)[N]) {
  constexpr int NA = 1 << N;
  qf2* x = reinterpret_cast<qf2*>(s_x);
  qf2* mine = x + ch * NA * 64;
  float sc[N];
  reup_run_scales<N>(sc, prog, trig, g0, g1);
  __syncthreads();   // whoever read s_x or s_rcs before is done
#pragma unroll
  for (int k = 0; k < NA; ++k) mine[k * 64 + lane] = cl[0].a[k];
  reup_run_sincos<N>(s_rcs, ch, sc, ajets, B, pc, lane);
  __syncthreads();
  {
    float t0[N], gv[N];   // gv: this lane's share of dL/ds per wire
#pragma unroll
    for (int w = 0; w < N; ++w) t0[w] = 0.f;
    reup_ip<N>(t0, mask, cl[1], cl[0]);
    reup_coef<N>(gv, mask, 0, ajets, B, pc);
#pragma unroll
    for (int w = 0; w < N; ++w) {
      gv[w] *= t0[w];
      T0[w] = fmaf(sc[w], t0[w], T0[w]);
    }
    if (ch >= 1 && ch <= 3) {
      float da[N], t1[N];
#pragma unroll
      for (int w = 0; w < N; ++w) t1[w] = 0.f;
      reup_coef<N>(da, mask, ch, ajets, B, pc);
      reup_ip_lds<N>(t1, mask, cl[1], x, lane, 1.f);
#pragma unroll
      for (int w = 0; w < N; ++w) {
        gv[w] = fmaf(t1[w], da[w], gv[w]);
        T1[w] = fmaf(sc[w], t1[w], T1[w]);
        da[w] *= sc[w];
      }
      reup_gen1<N>(cl[0], x, lane, da, -1.f);
    } else if (ch >= 4) {
      float da[N], dda[N], t1[N], t2[N];
#pragma unroll
      for (int w = 0; w < N; ++w) t1[w] = t2[w] = 0.f;
      reup_coef<N>(da, mask, ch - 2, ajets, B, pc);
      reup_coef<N>(dda, mask, ch, ajets, B, pc);
      const qf2* xk = x + (ch - 2) * NA * 64;
      reup_ip_lds<N>(t1, mask, cl[1], xk, lane, 2.f);
      reup_ip_lds<N>(t2, mask, cl[1], x, lane, 1.f);
#pragma unroll
      for (int w = 0; w < N; ++w) {
        gv[w] = fmaf(t1[w], da[w], fmaf(t2[w], dda[w], gv[w]));
        T1[w] = fmaf(sc[w], t1[w], T1[w]);
        T2[w] = fmaf(sc[w], t2[w], T2[w]);
        da[w] *= sc[w];
        dda[w] *= sc[w];
      }
      reup_gen1<N>(cl[0], xk, lane, da, -2.f);
      reup_gen1<N>(cl[0], x, lane, dda, -1.f);
      reup_gen2<N>(cl[0], x, lane, da, 1.f);
    }
    for (int gi = g1 - 1; gi >= g0; --gi) {   // the scalings' gradients, in the reverse sweep's gate order
      const QcGate g = prog[gi];
      if (g.op != QC_EMBED_S) continue;
#pragma unroll
      for (int w = 0; w < N; ++w) {
        if (N - 1 - g.ba == w) {
          const float gr = qc_wave_sum6_to_lane63(live ? gv[w] : 0.f);
          if (lane == 63) acc_wave[g.slot] += gr;
        }
      }
    }
  }
  __syncthreads();   // chi' read by everyone
#pragma unroll
  for (int k = 0; k < NA; ++k) mine[k * 64 + lane] = cl[1].a[k];
  __syncthreads();
  if (ch == 2 || ch == 3) {
    float da[N];
    reup_coef_s<N>(da, mask, ch, sc, ajets, B, pc);
    reup_gen1<N>(cl[1], x + (ch + 2) * NA * 64, lane, da, -2.f);
  } else if (ch == 0) {
#pragma unroll 1
    for (int k = 1; k <= 3; ++k) {   // one direction at a time: keeps the live set small
      float da[N];
      reup_coef_s<N>(da, mask, k, sc, ajets, B, pc);
      reup_gen1<N>(cl[1], x + k * NA * 64, lane, da, -1.f);
      if (k >= 2) {
        float dda[N];
        reup_coef_s<N>(dda, mask, k + 2, sc, ajets, B, pc);
        reup_gen2<N>(cl[1], x + (k + 2) * NA * 64, lane, da, 1.f);
        reup_gen1<N>(cl[1], x + (k + 2) * NA * 64, lane, dda, -1.f);
      }
    }
  }
  float ca[N], sa[N];
  load_sincos_lds<N>(ca, sa, s_rcs);
  reup_rx<N, 2, true>(cl, mask, ca, sa);
}

template <int N, bool SCALED>
__global__ void __launch_bounds__(384) k_reup_jets_bwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                       const float* __restrict__ umat, int n_gates, int n_params,
                                                       const float* __restrict__ ajets, const float* __restrict__ qbar,
                                                       float* __restrict__ abar, float* __restrict__ part,
                                                       int64_t part_stride, int64_t row0, int64_t B) {
  constexpr int A2 = 2 << N;
  constexpr int NA = 1 << N;
  extern __shared__ float smem[];
  float* s_x = smem;                         // [6][A2][64]; reused as [6 waves][3][N][64] at the end
  float* s_acc = smem + 6 * A2 * 64;         // [6 waves][n_params]
  float* s_cs = s_acc + 6 * n_params;        // [cos | sin][N][64] of the embedding half-angles
  float* s_rcs = SCALED ? s_cs + 2 * N * 64 : nullptr;   // SCALED: the same of one run's scaled angles
  const int lane = threadIdx.x & 63;
  const int ch = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < 6 * n_params; i += 384) s_acc[i] = 0.f;
  const int64_t p = (int64_t)blockIdx.x * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  if (ch < N) qc_wire_sincos<0>(s_cs[ch * 64 + lane], s_cs[(N + ch) * 64 + lane], ajets, B, pc, ch, trig, 0);
  __syncthreads();

  SV<N> cl[2];
  {
    SV<N> v[1];
    build_channel<N, 0>(v[0], ch, ajets, B, pc, 0, trig, 0, s_cs);
    reup_jets_sweep<N, SCALED>(v, ch, prog, trig, umat, n_gates, s_x, s_cs, s_rcs, ajets, B, pc, lane);
    cl[0] = v[0];
  }
  __syncthreads();   // the last run's readers are done
  {
    qf2* mine = reinterpret_cast<qf2*>(s_x) + ch * NA * 64;
#pragma unroll
    for (int k = 0; k < NA; ++k) mine[k * 64 + lane] = cl[0].a[k];
  }
  __syncthreads();
  auto other = [&](int c, int k) -> qf2 { return reinterpret_cast<const qf2*>(s_x)[(c * NA + k) * 64 + lane]; };
  // ---- cotangent of this channel's final state (the bilinear <Z> forms of the register family)
  auto dvec = [&](int c, QcPk<NA>& d) {
    float qb[N];
#pragma unroll
    for (int w = 0; w < N; ++w) qb[w] = live ? qbar[((int64_t)c * N + w) * B + pc] : 0.f;
    qc_sign_sums<N>(d, qb);
  };
  {
    QcPk<NA> d;
    if (ch == 0) {
      dvec(0, d);
#pragma unroll
      for (int k = 0; k < NA; ++k) cl[1].a[k] = qc_dup(d[k]) * cl[0].a[k];
#pragma unroll 1
      for (int c = 1; c < QC_NCH; ++c) {
        dvec(c, d);
#pragma unroll
        for (int k = 0; k < NA; ++k) cl[1].a[k] = qc_pk_fma(qc_dup(d[k]), other(c, k), cl[1].a[k]);
      }
    } else {
      dvec(ch, d);
#pragma unroll
      for (int k = 0; k < NA; ++k) cl[1].a[k] = qc_dup(d[k]) * other(0, k);
      if (ch == 2 || ch == 3) {
        dvec(ch + 2, d);
#pragma unroll
        for (int k = 0; k < NA; ++k) cl[1].a[k] = qc_pk_fma(qc_dup(2.f * d[k]), cl[0].a[k], cl[1].a[k]);
      }
    }
  }

  float T0[N], T1[N], T2[N];
#pragma unroll
  for (int w = 0; w < N; ++w) T0[w] = T1[w] = T2[w] = 0.f;
  int g1 = n_gates;
  while (true) {
    const int e = reup_prev<SCALED>(prog, g1);
    DynProg<N>::template bwd<0>(cl, prog + e + 1, trig + e + 1, umat, g1 - e - 1, s_acc + ch * n_params, lane, 0);
    if (e < 0) break;
    int mask;
    g1 = reup_run_bwd<N, SCALED>(prog, e, mask) + 1;
    if constexpr (SCALED)
      reup_layer_bwd_s<N>(cl, ch, mask, prog, trig, g1, e + 1, s_x, s_rcs, ajets, B, pc, lane, live, s_acc + ch * n_params, T0, T1,
                          T2);
    else
      reup_layer_bwd<N>(cl, ch, mask, s_x, s_cs, ajets, B, pc, lane, T0, T1, T2);
  }
  __syncthreads();   // s_x is free for the tail

  // ---- the first embedding: Im<Lambda| X_w |phi_c> in the frame pulled back through it (qc_gates.h)
  {
    const float* aj = qc_launder(ajets);
    float ca[N], sa[N], da[N], dda[N];
    load_sincos_lds<N>(ca, sa, s_cs);
    qc_unembed<N>(cl[1], ca, sa);
    const int dirch = ch == 0 ? 0 : (ch <= 3 ? ch : ch - 2);
#pragma unroll
    for (int w = 0; w < N; ++w) {
      da[w] = ch >= 1 ? aj[((int64_t)dirch * N + w) * B + pc] : 0.f;
      dda[w] = ch >= 4 ? aj[((int64_t)ch * N + w) * B + pc] : 0.f;
    }
    float* buf = s_x + ch * 3 * N * 64;  // [3][N][64] per wave
    float T[N];
    if (ch == 0) {
      qc_pull_ip0<N>(T, cl[1]);
#pragma unroll
      for (int w = 0; w < N; ++w) buf[(0 * N + w) * 64 + lane] = T[w] + T0[w];
    } else if (ch <= 3) {
      qc_pull_ip1<N>(T, cl[1], da);
#pragma unroll
      for (int w = 0; w < N; ++w) buf[(0 * N + w) * 64 + lane] = T[w] + T0[w];
      qc_pull_ip0<N>(T, cl[1]);
#pragma unroll
      for (int w = 0; w < N; ++w) buf[(1 * N + w) * 64 + lane] = T[w] + T1[w];
    } else {
      qc_pull_ip2<N>(T, cl[1], da, dda);
#pragma unroll
      for (int w = 0; w < N; ++w) buf[(0 * N + w) * 64 + lane] = T[w] + T0[w];
      qc_pull_ip1<N>(T, cl[1], da);
#pragma unroll
      for (int w = 0; w < N; ++w) buf[(1 * N + w) * 64 + lane] = 2.f * T[w] + T1[w];
      qc_pull_ip0<N>(T, cl[1]);
#pragma unroll
      for (int w = 0; w < N; ++w) buf[(2 * N + w) * 64 + lane] = T[w] + T2[w];
    }
    __syncthreads();
    auto at = [&](int wv, int slot, int w) { return s_x[((wv * 3 + slot) * N + w) * 64 + lane]; };
#pragma unroll
    for (int w = 0; w < N; ++w) {
      float r;
      if (ch == 0)
        r = ((at(0, 0, w) + at(1, 0, w)) + (at(2, 0, w) + at(3, 0, w))) + (at(4, 0, w) + at(5, 0, w));
      else if (ch == 1)
        r = at(1, 1, w);
      else if (ch <= 3)
        r = at(ch, 1, w) + at(ch + 2, 1, w);
      else
        r = at(ch, 2, w);
      if (live) abar[((int64_t)ch * N + w) * B + p] = r;
    }
  }
  // (s_acc: every wave's last write is before the barrier above)
  for (int i = threadIdx.x; i < n_params; i += 384) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < 6; ++wv) s += s_acc[wv * n_params + i];
    part[(row0 + blockIdx.x) * part_stride + i] = s;
  }
}

}  // namespace
