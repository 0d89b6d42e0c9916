// Classical pre / post networks of DVPDESolver with SEVEN derivative channels: the six of qc_mlp.hip and channel
// 6 = d2/dt2, for residuals that are second order in time over two space dimensions,
//   res_p = c_u u + c_3 u^3 + c_t u_t + c_x u_x + c_y u_y - (d_xx u_xx + d_yy u_yy + d_tt u_tt)
// (wave: d_tt = -1, d_xx = d_yy = c^2; the 2-D forms of wave_operator / klein_gordon_operator, reference nn/pde.py:28-52).
//
// The kernels of qc_mlp.hip are not touched: these are separate bodies, one 64-point tile per block of four waves, a
// lane per point and wave w on the hidden units w, w + 4, ..  Plain inputs (no Fourier map), no angle map, 2 <= n <= 5
// (the qubit counts of the seven-channel circuit stages).  Flat parameter vector, partial rows and loss columns are
// those of qc_mlp.hip; weight gradients are wave sums written by one lane: fixed order, no atomics.
//
// Channel algebra.  Pre: s_j = W1[j] . X + b1[j], z = tanh s, d1 = 1 - z^2, d2 = -2 z d1, d3 = -2 (d1^2 + z d2),
// w_k = W1[j][k] (k = t, x, y):
//   a[i] = sum_j W2[i][j] z + b2[i],  a_k[i] = sum_j W2[i][j] d1 w_k,  a_kk[i] = sum_j W2[i][j] d2 w_k^2   (kk = xx, yy, tt).
// Post: g_c = W3[m] . q_c, h = tanh(g_0 + b3[m]):  u = sum_m W4[m] h + b4,  u_k = sum_m W4[m] d1 g_k,
//   u_kk = sum_m W4[m] (d1 g_kk + d2 g_k^2).
#include "qc_internal.h"

#include <type_traits>

#define QC_TT_NCH 7
#define QC_TT_COEF 8   // == QC_COEF_TT_COLS of the public header

namespace {

constexpr int TT_MS = 4;   // waves per block

__device__ __forceinline__ float tt_tanh(float x) {   // qc_tanh of qc_mlp.hip
  const float e = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}
// the channel that holds the second derivative along direction k = 1, 2, 3 (t, x, y)
__device__ __forceinline__ constexpr int tt_sec(int k) { return k == 1 ? 6 : k + 2; }

template <int N>
__global__ void __launch_bounds__(256) k_tt_pre_fwd(const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                                                    float* __restrict__ ajets, int64_t B) {
  __shared__ float s_part[TT_MS][QC_TT_NCH * N][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p = (int64_t)blockIdx.x * 64 + lane;
  const int64_t pc = p < B ? p : B - 1;
  const float t = X[pc * 3 + 0], x = X[pc * 3 + 1], y = X[pc * 3 + 2];
  const float *W1 = prm + L.oW1, *b1 = prm + L.ob1, *W2 = prm + L.oW2, *b2 = prm + L.ob2;
  float acc[QC_TT_NCH][N];
#pragma unroll
  for (int c = 0; c < QC_TT_NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) acc[c][i] = 0.f;
  for (int j = wave; j < L.H; j += TT_MS) {
    const float w0 = W1[j * 3 + 0], w1 = W1[j * 3 + 1], w2 = W1[j * 3 + 2];
    const float z = tt_tanh(fmaf(w0, t, fmaf(w1, x, fmaf(w2, y, b1[j]))));
    const float d1 = 1.f - z * z, d2 = -2.f * z * d1;
    const float f[QC_TT_NCH] = {z, d1 * w0, d1 * w1, d1 * w2, d2 * w1 * w1, d2 * w2 * w2, d2 * w0 * w0};
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float w = W2[i * L.H + j];
#pragma unroll
      for (int c = 0; c < QC_TT_NCH; ++c) acc[c][i] = fmaf(w, f[c], acc[c][i]);
    }
  }
#pragma unroll
  for (int c = 0; c < QC_TT_NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) s_part[wave][c * N + i][lane] = acc[c][i];
  __syncthreads();
  if (p < B) {
    for (int f = wave; f < QC_TT_NCH * N; f += TT_MS) {
      float v = (s_part[0][f][lane] + s_part[1][f][lane]) + (s_part[2][f][lane] + s_part[3][f][lane]);
      if (f < N) v += b2[f];
      ajets[(int64_t)f * B + p] = v;
    }
  }
}

// the tile's row: W1[H][3], b1[H], W2[n][H], b2[n] columns, every one written
template <int N>
__global__ void __launch_bounds__(256) k_tt_pre_bwd(const float* __restrict__ X, const float* __restrict__ prm, QcLayout L,
                                                    const float* __restrict__ abar, float* __restrict__ part,
                                                    int64_t part_stride, int64_t row0, int64_t B) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p = (int64_t)blockIdx.x * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  const float t = X[pc * 3 + 0], x = X[pc * 3 + 1], y = X[pc * 3 + 2];
  const float *W1 = prm + L.oW1, *b1 = prm + L.ob1, *W2 = prm + L.oW2;
  float* __restrict__ row = part + (row0 + blockIdx.x) * part_stride;
  float ab[QC_TT_NCH][N];
#pragma unroll
  for (int c = 0; c < QC_TT_NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) ab[c][i] = live ? abar[(int64_t)(c * N + i) * B + pc] : 0.f;
  for (int j = wave; j < L.H; j += TT_MS) {
    const float w0 = W1[j * 3 + 0], w1 = W1[j * 3 + 1], w2 = W1[j * 3 + 2];
    const float z = tt_tanh(fmaf(w0, t, fmaf(w1, x, fmaf(w2, y, b1[j]))));
    const float d1 = 1.f - z * z, d2 = -2.f * z * d1, d3 = -2.f * (d1 * d1 + z * d2);
    const float f[QC_TT_NCH] = {z, d1 * w0, d1 * w1, d1 * w2, d2 * w1 * w1, d2 * w2 * w2, d2 * w0 * w0};
    float A[QC_TT_NCH];   // cotangents of the seven hidden-unit jets
#pragma unroll
    for (int c = 0; c < QC_TT_NCH; ++c) A[c] = 0.f;
    float g[4 + N];       // dW1[j][0..2], db1[j], dW2[0..N)[j]
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float w = W2[i * L.H + j];
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < QC_TT_NCH; ++c) {
        A[c] = fmaf(w, ab[c][i], A[c]);
        s = fmaf(ab[c][i], f[c], s);
      }
      g[4 + i] = s;
    }
    const float ds = A[0] * d1 + (A[1] * w0 + A[2] * w1 + A[3] * w2) * d2 + (A[4] * w1 * w1 + A[5] * w2 * w2 + A[6] * w0 * w0) * d3;
    g[0] = fmaf(ds, t, A[1] * d1 + 2.f * A[6] * d2 * w0);
    g[1] = fmaf(ds, x, A[2] * d1 + 2.f * A[4] * d2 * w1);
    g[2] = fmaf(ds, y, A[3] * d1 + 2.f * A[5] * d2 * w2);
    g[3] = ds;
#pragma unroll
    for (int k = 0; k < 4 + N; ++k) g[k] = qc_wave_sum_to_lane63(g[k]);
    if (lane == 63) {
      row[L.oW1 + j * 3 + 0] = g[0];
      row[L.oW1 + j * 3 + 1] = g[1];
      row[L.oW1 + j * 3 + 2] = g[2];
      row[L.ob1 + j] = g[3];
#pragma unroll
      for (int i = 0; i < N; ++i) row[L.oW2 + i * L.H + j] = g[4 + i];
    }
  }
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float s = qc_wave_sum_to_lane63(ab[0][i]);
      if (lane == 63) row[L.ob2 + i] = s;
    }
  }
}

// hidden unit m of the post network at this lane's point: g_c = W3[m] . q_c, z = tanh(g_0 + b3[m])
template <int N>
__device__ __forceinline__ float tt_hidden(float (&g)[QC_TT_NCH], const float (&q)[QC_TT_NCH][N], const float* __restrict__ W3,
                                           const float b3m, const int m) {
#pragma unroll
  for (int c = 0; c < QC_TT_NCH; ++c) g[c] = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float w = W3[m * N + i];
#pragma unroll
    for (int c = 0; c < QC_TT_NCH; ++c) g[c] = fmaf(w, q[c][i], g[c]);
  }
  return tt_tanh(g[0] + b3m);
}

// MODE 2: forward, residual against target with the [8][B] operator rows, loss column, the seven channel cotangents
//         (-> cot[7][B]) and the reverse pass (qbar, W3 / b3 / W4 / b4 columns and the three loss columns of the tile's row);
// MODE 3: the reverse pass alone from given cotangents ubar[7][B] (io) of the seven channels (no loss columns);
// MODE 4: forward only, the seven channels of u -> io[7][B].
template <int N, int MODE>
__global__ void __launch_bounds__(256) k_tt_post(const float* __restrict__ prm, QcLayout L, QcPde pde,
                                                 const float* __restrict__ qjets, const float* __restrict__ target,
                                                 const float* __restrict__ coef, float* __restrict__ io,
                                                 float* __restrict__ qbar, float* __restrict__ part, int64_t part_stride,
                                                 int64_t row0, int64_t B) {
  __shared__ float s_buf[TT_MS][QC_TT_NCH * N][64];   // partial u jets first (7 rows), partial qbar later
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p = (int64_t)blockIdx.x * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  const float *W3 = prm + L.oW3, *b3 = prm + L.ob3, *W4 = prm + L.oW4;
  float q[QC_TT_NCH][N];
#pragma unroll
  for (int c = 0; c < QC_TT_NCH; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) q[c][i] = qjets[(int64_t)(c * N + i) * B + pc];

  float ub[QC_TT_NCH];
  if constexpr (MODE != 3) {
    float u[QC_TT_NCH];
#pragma unroll
    for (int c = 0; c < QC_TT_NCH; ++c) u[c] = 0.f;
    for (int m = wave; m < L.H; m += TT_MS) {
      float g[QC_TT_NCH];
      const float z = tt_hidden<N>(g, q, W3, b3[m], m);
      const float d1 = 1.f - z * z, d2 = -2.f * z * d1, w4 = W4[m];
      u[0] = fmaf(w4, z, u[0]);
#pragma unroll
      for (int k = 1; k <= 3; ++k) {
        u[k] = fmaf(w4, d1 * g[k], u[k]);
        u[tt_sec(k)] = fmaf(w4, fmaf(d2 * g[k], g[k], d1 * g[tt_sec(k)]), u[tt_sec(k)]);
      }
    }
#pragma unroll
    for (int c = 0; c < QC_TT_NCH; ++c) s_buf[wave][c][lane] = u[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < QC_TT_NCH; ++c) u[c] = (s_buf[0][c][lane] + s_buf[1][c][lane]) + (s_buf[2][c][lane] + s_buf[3][c][lane]);
    __syncthreads();   // s_buf is reused for the qbar partials below
    u[0] += prm[L.ob4];
    if constexpr (MODE == 4) {
      if (live && wave == 0) {
#pragma unroll
        for (int c = 0; c < QC_TT_NCH; ++c) io[(int64_t)c * B + p] = u[c];
      }
      return;
    } else {
      float cf[QC_TT_COEF];
#pragma unroll
      for (int k = 0; k < QC_TT_COEF; ++k) cf[k] = coef[(int64_t)k * B + pc];
      float res = cf[1] * u[1] + cf[2] * u[2] + cf[3] * u[3] - (cf[4] * u[4] + cf[5] * u[5] + cf[7] * u[6]);
      res = fmaf(fmaf(cf[6] * u[0], u[0], cf[0]), u[0], res);
      const float e = live ? res - target[pc] : 0.f;
      const float gsc = pde.w_res * e;
      ub[0] = (cf[0] + 3.f * cf[6] * u[0] * u[0]) * gsc;
      ub[1] = gsc * cf[1];
      ub[2] = gsc * cf[2];
      ub[3] = gsc * cf[3];
      ub[4] = -cf[4] * gsc;
      ub[5] = -cf[5] * gsc;
      ub[6] = -cf[7] * gsc;
      if (wave == 0) {
        float* __restrict__ row = part + (row0 + blockIdx.x) * part_stride;
        const float ls = qc_wave_sum_to_lane63(e * e * pde.inv_n_res);
        const float sb4 = qc_wave_sum_to_lane63(ub[0]);
        if (lane == 63) {
          row[L.NP + 0] = ls;
          row[L.NP + 1] = 0.f;
          row[L.NP + 2] = 0.f;
          row[L.ob4] = sb4;
        }
        if (live) {
#pragma unroll
          for (int c = 0; c < QC_TT_NCH; ++c) io[(int64_t)c * B + p] = ub[c];
        }
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < QC_TT_NCH; ++c) ub[c] = live ? io[(int64_t)c * B + pc] : 0.f;
    if (wave == 0) {
      const float sb4 = qc_wave_sum_to_lane63(ub[0]);
      if (lane == 63) part[(row0 + blockIdx.x) * part_stride + L.ob4] = sb4;
    }
  }

  if constexpr (MODE != 4) {
    float* __restrict__ row = part + (row0 + blockIdx.x) * part_stride;
    float qb[QC_TT_NCH][N];
#pragma unroll
    for (int c = 0; c < QC_TT_NCH; ++c)
#pragma unroll
      for (int i = 0; i < N; ++i) qb[c][i] = 0.f;
    for (int m = wave; m < L.H; m += TT_MS) {
      float g[QC_TT_NCH];
      const float z = tt_hidden<N>(g, q, W3, b3[m], m);
      const float d1 = 1.f - z * z, d2 = -2.f * z * d1, d3 = -2.f * (d1 * d1 + z * d2), w4 = W4[m];
      // the t analogue of the gx2 / g[4] terms of post_cotangents (qc_mlp.hip), and those terms themselves
      float gw4 = ub[0] * z, gb[QC_TT_NCH];
      gb[0] = ub[0] * d1;
#pragma unroll
      for (int k = 1; k <= 3; ++k) {
        const int kk = tt_sec(k);
        const float g2 = g[k] * g[k];
        gw4 += d1 * ub[k] * g[k] + ub[kk] * (d2 * g2 + d1 * g[kk]);
        gb[0] += d2 * ub[k] * g[k] + ub[kk] * (d3 * g2 + d2 * g[kk]);
        gb[k] = ub[k] * d1 + 2.f * ub[kk] * d2 * g[k];
        gb[kk] = ub[kk] * d1;
      }
#pragma unroll
      for (int c = 0; c < QC_TT_NCH; ++c) gb[c] *= w4;
      float wg[N + 2];   // dW3[m][0..N), db3[m], dW4[m]
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float w3 = W3[m * N + i];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < QC_TT_NCH; ++c) {
          s = fmaf(gb[c], q[c][i], s);
          qb[c][i] = fmaf(w3, gb[c], qb[c][i]);
        }
        wg[i] = s;
      }
      wg[N] = gb[0];
      wg[N + 1] = gw4;
#pragma unroll
      for (int k = 0; k < N + 2; ++k) wg[k] = qc_wave_sum_to_lane63(wg[k]);
      if (lane == 63) {
#pragma unroll
        for (int i = 0; i < N; ++i) row[L.oW3 + m * N + i] = wg[i];
        row[L.ob3 + m] = wg[N];
        row[L.oW4 + m] = wg[N + 1];
      }
    }
#pragma unroll
    for (int c = 0; c < QC_TT_NCH; ++c)
#pragma unroll
      for (int i = 0; i < N; ++i) s_buf[wave][c * N + i][lane] = qb[c][i];
    __syncthreads();
    if (live) {
      for (int f = wave; f < QC_TT_NCH * N; f += TT_MS)
        qbar[(int64_t)f * B + p] = (s_buf[0][f][lane] + s_buf[1][f][lane]) + (s_buf[2][f][lane] + s_buf[3][f][lane]);
    }
  }
}

template <class F>
inline int tt_dispatch_n(const int n, F&& f) {
  switch (n) {
    case 2: f(std::integral_constant<int, 2>{}); return QC_OK;
    case 3: f(std::integral_constant<int, 3>{}); return QC_OK;
    case 4: f(std::integral_constant<int, 4>{}); return QC_OK;
    case 5: f(std::integral_constant<int, 5>{}); return QC_OK;
    default: return QC_ERR_UNSUPPORTED;
  }
}

}  // namespace

int qc_tt_pre_fwd(const float* X, const float* prm, QcLayout L, float* ajets, int64_t B, hipStream_t st) {
  return tt_dispatch_n(L.n, [&](auto n) {
    constexpr int N = n();
    hipLaunchKernelGGL((k_tt_pre_fwd<N>), dim3(qc_ceil_div(B, 64)), dim3(256), 0, st, X, prm, L, ajets, B);
  });
}

int qc_tt_pre_bwd(const float* X, const float* prm, QcLayout L, const float* abar, float* part, int64_t part_stride,
                  int64_t row0, int64_t B, hipStream_t st) {
  return tt_dispatch_n(L.n, [&](auto n) {
    constexpr int N = n();
    hipLaunchKernelGGL((k_tt_pre_bwd<N>), dim3(qc_ceil_div(B, 64)), dim3(256), 0, st, X, prm, L, abar, part, part_stride, row0, B);
  });
}

int qc_tt_post(int mode, const float* prm, QcLayout L, QcPde pde, const float* qjets, const float* target, const float* coef,
               float* io, float* qbar, float* part, int64_t part_stride, int64_t row0, int64_t B, hipStream_t st) {
  return tt_dispatch_n(L.n, [&](auto n) {
    constexpr int N = n();
    const dim3 grid(qc_ceil_div(B, 64)), block(256);
    if (mode == 2)
      hipLaunchKernelGGL((k_tt_post<N, 2>), grid, block, 0, st, prm, L, pde, qjets, target, coef, io, qbar, part, part_stride, row0, B);
    else if (mode == 3)
      hipLaunchKernelGGL((k_tt_post<N, 3>), grid, block, 0, st, prm, L, pde, qjets, target, coef, io, qbar, part, part_stride, row0, B);
    else
      hipLaunchKernelGGL((k_tt_post<N, 4>), grid, block, 0, st, prm, L, pde, qjets, target, coef, io, qbar, part, part_stride, row0, B);
  });
}
