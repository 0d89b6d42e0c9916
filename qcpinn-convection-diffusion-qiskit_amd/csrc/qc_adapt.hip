// Residual-adaptive sampling of the dataset's residual rows (RAD: Wu et al. 2023; RAR: Lu et al. 2021): the score of a
// row from the six channels of u, and scores -> the integer CDF that the CDF rules of k_gather (qc_sample.hip) search.
// The definitions are those of include/qcpinn_hip.h (qc_dataset_scores, qc_adapt_build); tests/adaptive_reference.py
// restates them in numpy.  Everything behind the fp32 power is integer arithmetic, so no result depends on the order of a
// reduction.  The scan is three launches (block totals, scan of the totals, per-block scan plus offset): no block ever
// waits for another block of its launch.
#include <float.h>

#include "qc_internal.h"
#include "../../include/qcpinn_hip.h"

static_assert(sizeof(QcAdaptRec) == 64, "adapt record");
static_assert(QC_ADAPT_ROWS == QC_ADAPT_BLOCK, "rows per coarse entry");

namespace {

constexpr int ROWS = QC_ADAPT_ROWS;   // rows per block of the first and third launch = rows per coarse entry
constexpr int TPB = 256;              // threads of those blocks
constexpr int RPT = ROWS / TPB;       // consecutive rows per thread
constexpr int TILE = 1024;            // coarse entries per pass of the second level's loop (one per thread)

// p = e^power by left-to-right fp32 multiplication; NaN or negative -> 0, above FLT_MAX -> FLT_MAX
__device__ __forceinline__ float adapt_p(float e, int power) {
  float p = e;
  for (int k = 1; k < power; ++k) p *= e;
  if (!(p > 0.f)) p = 0.f;
  return fminf(p, FLT_MAX);
}

// ilogb of a positive finite float, subnormals included
__device__ __forceinline__ int adapt_ilogb(float v) {
  const uint32_t b = __float_as_uint(v);
  const int ex = (int)((b >> 23) & 0xFF);
  return ex ? ex - 127 : (31 - __clz((int)(b & 0x7FFFFF))) - 149;
}

// floor(p * 2^s) for 0 <= p <= M, s = 23 - ilogb(M): below 2^24, exact (a shift of the significand)
__device__ __forceinline__ uint64_t adapt_q(float p, int s) {
  const uint32_t b = __float_as_uint(p);
  int ex = (int)((b >> 23) & 0xFF);
  uint32_t m = b & 0x7FFFFF;
  if (ex) m |= 0x800000;
  else ex = 1;
  const int k = 150 - ex - s;   // p = m 2^(ex - 150)
  if (k >= 32) return 0;
  return k <= 0 ? (uint64_t)m << -k : (uint64_t)(m >> k);
}

__device__ __forceinline__ uint64_t adapt_q_of(float e, int power, float M, int s) {
  return M > 0.f ? adapt_q(adapt_p(e, power), s) : 1;   // all scores zero: uniform weights
}

// inclusive scan of one value per thread over the block, in place in LDS (Hillis-Steele); returns this thread's prefix
template <int NT>
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    const uint64_t add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  return sh[t];
}

// launch 0: M = max p as the maximum of the bit patterns (non-negative floats order as unsigned integers)
__global__ void __launch_bounds__(TPB) k_adapt_max(const float* __restrict__ score, int64_t n, int power, QcAdaptRec* rec) {
  __shared__ uint32_t sh[TPB];
  uint32_t m = 0;
  for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
    const uint32_t b = __float_as_uint(adapt_p(score[j], power));
    m = b > m ? b : m;
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int d = TPB / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d && sh[threadIdx.x + d] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sh[0] > 0) atomicMax((unsigned int*)&rec->max_p, sh[0]);
}

// launch 1: coarse[b] = sum of q over block b's rows
__global__ void __launch_bounds__(TPB) k_adapt_totals(const float* __restrict__ score, int64_t n, int power,
                                                      const QcAdaptRec* __restrict__ rec, uint64_t* __restrict__ coarse) {
  __shared__ uint64_t sh[TPB];
  const float M = rec->max_p;
  const int s = M > 0.f ? 23 - adapt_ilogb(M) : 0;
  const int64_t j0 = (int64_t)blockIdx.x * ROWS + (int64_t)threadIdx.x * RPT;
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < RPT; ++k)
    if (j0 + k < n) v += adapt_q_of(score[j0 + k], power, M, s);
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int d = TPB / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) coarse[blockIdx.x] = sh[0];
}

// launch 2, ONE block: Q = sum of the block totals, the floor term a, then the inclusive scan of the blocks' weights
// total_b + a rows_b, TILE entries per pass with a running carry: coarse[b] = cdf of block b's last row
__global__ void __launch_bounds__(TILE) k_adapt_scan_totals(int64_t n, int64_t nb, float floor_c, QcAdaptRec* rec,
                                                            uint64_t* __restrict__ coarse) {
  __shared__ uint64_t sh[TILE];
  __shared__ uint64_t carry_sh;
  const int t = threadIdx.x;
  uint64_t v = 0;
  for (int64_t b = t; b < nb; b += TILE) v += coarse[b];
  sh[t] = v;
  __syncthreads();
  for (int d = TILE / 2; d > 0; d >>= 1) {
    if (t < d) sh[t] += sh[t + d];
    __syncthreads();
  }
  const uint64_t Q = sh[0];
  __syncthreads();
  uint64_t a = (uint64_t)((double)floor_c * (double)Q / (double)n);
  if (floor_c > 0.f && a == 0) a = 1;
  uint64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += TILE) {
    const int64_t b = b0 + t;
    uint64_t w = 0;
    if (b < nb) {
      const int64_t rows = (b + 1) * ROWS <= n ? ROWS : n - b * ROWS;
      w = coarse[b] + a * (uint64_t)rows;
    }
    const uint64_t incl = block_scan<TILE>(w, sh) + carry;
    if (b < nb) coarse[b] = incl;
    if (t == TILE - 1) carry_sh = incl;
    __syncthreads();
    carry = carry_sh;
  }
  if (t == 0) {
    const float M = rec->max_p;
    rec->total = carry;
    rec->q_sum = Q;
    rec->add = a;
    rec->shift = M > 0.f ? 23 - adapt_ilogb(M) : 0;
  }
}

// launch 3: cdf of block b's rows = coarse[b - 1] + inclusive scan of w = q + a
__global__ void __launch_bounds__(TPB) k_adapt_scan_blocks(const float* __restrict__ score, int64_t n, int power,
                                                           const QcAdaptRec* __restrict__ rec,
                                                           const uint64_t* __restrict__ coarse, uint64_t* __restrict__ cdf) {
  __shared__ uint64_t sh[TPB];
  const float M = rec->max_p;
  const int s = rec->shift;
  const uint64_t a = rec->add;
  const int64_t j0 = (int64_t)blockIdx.x * ROWS + (int64_t)threadIdx.x * RPT;
  uint64_t w[RPT], sum = 0;
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    w[k] = j0 + k < n ? adapt_q_of(score[j0 + k], power, M, s) + a : 0;
    sum += w[k];
  }
  uint64_t run = block_scan<TPB>(sum, sh) - sum + (blockIdx.x ? coarse[blockIdx.x - 1] : 0);
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    run += w[k];
    if (j0 + k < n) cdf[j0 + k] = run;
  }
}

// e = |res - r| of `c` dataset rows from the six channels of u ([6][c], qc_post mode 4); the operator is the step's:
// scalar (pde, c_u) or the row's own coefficients coef[c][7] with the cubic term
template <bool COEF>
__global__ void __launch_bounds__(256) k_adapt_score(const float* __restrict__ uj, int64_t c, QcPde pde, float c_u,
                                                     const float* __restrict__ coef, const float* __restrict__ tg,
                                                     float* __restrict__ score) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= c) return;
  const float u = uj[i], ut = uj[c + i], ux = uj[2 * c + i], uy = uj[3 * c + i], uxx = uj[4 * c + i], uyy = uj[5 * c + i];
  float res;
  if (COEF) {
    const float* r = coef + i * QC_COEF_N;
    res = r[0] * u + r[6] * u * u * u + r[1] * ut + r[2] * ux + r[3] * uy - (r[4] * uxx + r[5] * uyy);
  } else {
    res = c_u * u + pde.c_t * ut + pde.c_x * ux + pde.c_y * uy - (pde.d_xx * uxx + pde.d_yy * uyy);
  }
  score[i] = fabsf(res - tg[i]);
}

}  // namespace

int qc_adapt_score_launch(const float* uj, int64_t c, QcPde pde, float c_u, const float* coef_rows, const float* tg,
                          float* score, hipStream_t st) {
  if (c <= 0) return QC_OK;
  if (coef_rows)
    hipLaunchKernelGGL(k_adapt_score<true>, dim3(qc_ceil_div(c, 256)), dim3(256), 0, st, uj, c, pde, c_u, coef_rows, tg, score);
  else
    hipLaunchKernelGGL(k_adapt_score<false>, dim3(qc_ceil_div(c, 256)), dim3(256), 0, st, uj, c, pde, c_u, coef_rows, tg, score);
  return QC_OK;
}

int qc_adapt_build_launch(const float* score, int64_t n, int power, float floor_c, void* adapt, hipStream_t st) {
  QcAdaptRec* rec = (QcAdaptRec*)adapt;
  uint64_t* cdf = (uint64_t*)((char*)adapt + sizeof(QcAdaptRec));
  uint64_t* coarse = cdf + n;
  const int64_t nb = (n + ROWS - 1) / ROWS;
  if (hipMemsetAsync(rec, 0, sizeof(QcAdaptRec), st) != hipSuccess) return QC_ERR_HIP;
  hipLaunchKernelGGL(k_adapt_max, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(TPB), 0, st, score, n, power, rec);
  hipLaunchKernelGGL(k_adapt_totals, dim3((unsigned)nb), dim3(TPB), 0, st, score, n, power, rec, coarse);
  hipLaunchKernelGGL(k_adapt_scan_totals, dim3(1), dim3(TILE), 0, st, n, nb, floor_c, rec, coarse);
  hipLaunchKernelGGL(k_adapt_scan_blocks, dim3((unsigned)nb), dim3(TPB), 0, st, score, n, power, rec, coarse, cdf);
  return QC_OK;
}
