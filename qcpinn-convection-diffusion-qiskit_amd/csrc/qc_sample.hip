// Collocation-point sampler: the three uniform batches of one training step in one launch.
//
// Replaces the three torch.rand draws + affine maps of the reference step
// (trainer/diffusion_train.py:9-20 boxes, :34-36 order IC -> BC1 -> residual; data/diffusion_dataset.py:12-19
// x = lo + (hi - lo) * rand).  Counter-based Philox4x32-10 keyed by (seed, step, batch id) and indexed
// by the GLOBAL point index, so a data-parallel run draws exactly the points the single-GPU run draws
// (each rank fills its shard of the same global batch) and no generator state lives on the host.
#include "qc_internal.h"
#include "qc_philox.h"

namespace {

// segment 0: residual points in [0,1]^3; 1: IC points (t = 0); 2: boundary points: the x = 0 face
// (trainer/diffusion_train.py:13-16), or with face_pts > 0 the four faces x=0, x=1, y=0, y=1 of the second
// workload (train_hybrid_qpinn.py:166-176), face = global index / face_pts; RF (face_pts < 0): a random face per
// point (trainer/train.py:118-135, qc_philox.h)
template <bool RF>
__global__ void __launch_bounds__(256) k_sample(float* __restrict__ X_res, int64_t n_res, int64_t off_res,
                                                float* __restrict__ X_val, int64_t n_ic, int64_t off_ic,
                                                int64_t n_bc, int64_t off_bc, int64_t face_pts, uint64_t seed,
                                                uint64_t step) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int seg;
  int64_t local, gidx;
  float* dst;
  if (i < n_res) {
    seg = 0; local = i; gidx = off_res + local; dst = X_res + local * 3;
  } else if (i < n_res + n_ic) {
    seg = 1; local = i - n_res; gidx = off_ic + local; dst = X_val + local * 3;
  } else if (i < n_res + n_ic + n_bc) {
    seg = 2; local = i - n_res - n_ic; gidx = off_bc + local; dst = X_val + (n_ic + local) * 3;
  } else {
    return;
  }
  float t, x, y;
  qc_draw_point<RF>(seg, gidx, face_pts, seed, step, t, x, y);
  dst[0] = t;
  dst[1] = x;
  dst[2] = y;
}

// Dataset mode of the same launch (the tabulated step): point i of a segment copies row idx of that segment's resident
// dataset and its target, idx drawn by qc_draw_index from the counter the coordinate draw uses.  Value rows and value
// targets are laid out IC first, then BC, like X_val.
struct QcDsSeg {
  const float* X;   // [n][3]
  const float* tg;  // [n]
  int64_t n;
};

__global__ void __launch_bounds__(256) k_sample_dataset(float* __restrict__ X_res, float* __restrict__ tg_res, int64_t n_res,
                                                        int64_t off_res, float* __restrict__ X_val,
                                                        float* __restrict__ tg_val, int64_t n_ic, int64_t off_ic,
                                                        int64_t n_bc, int64_t off_bc, QcDsSeg d_res, QcDsSeg d_ic,
                                                        QcDsSeg d_bc, uint64_t seed, uint64_t step) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int seg;
  int64_t out, gidx;
  float *dstX, *dstT;
  QcDsSeg ds;
  if (i < n_res) {
    seg = 0; out = i; gidx = off_res + i; dstX = X_res; dstT = tg_res; ds = d_res;
  } else if (i < n_res + n_ic) {
    seg = 1; out = i - n_res; gidx = off_ic + out; dstX = X_val; dstT = tg_val; ds = d_ic;
  } else if (i < n_res + n_ic + n_bc) {
    seg = 2; out = i - n_res; gidx = off_bc + (out - n_ic); dstX = X_val; dstT = tg_val; ds = d_bc;
  } else {
    return;
  }
  const int64_t idx = qc_draw_index(seg, gidx, ds.n, seed, step);   // < ds.n: the product's high word
  dstX[out * 3 + 0] = ds.X[idx * 3 + 0];
  dstX[out * 3 + 1] = ds.X[idx * 3 + 1];
  dstX[out * 3 + 2] = ds.X[idx * 3 + 2];
  dstT[out] = ds.tg[idx];
}

// The same gather for the coefficient step: a residual point also copies its operator row, ds_coef[idx][7] ->
// coef_res[7][n_res] (batch-minor).  Same segments, counters and index, hence the same batches as k_sample_dataset.
__global__ void __launch_bounds__(256) k_sample_dataset_coef(float* __restrict__ X_res, float* __restrict__ tg_res,
                                                             int64_t n_res, int64_t off_res, float* __restrict__ X_val,
                                                             float* __restrict__ tg_val, int64_t n_ic, int64_t off_ic,
                                                             int64_t n_bc, int64_t off_bc, QcDsSeg d_res, QcDsSeg d_ic,
                                                             QcDsSeg d_bc, uint64_t seed, uint64_t step,
                                                             float* __restrict__ coef_res, const float* __restrict__ ds_coef) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int seg;
  int64_t out, gidx;
  float *dstX, *dstT;
  QcDsSeg ds;
  if (i < n_res) {
    seg = 0; out = i; gidx = off_res + i; dstX = X_res; dstT = tg_res; ds = d_res;
  } else if (i < n_res + n_ic) {
    seg = 1; out = i - n_res; gidx = off_ic + out; dstX = X_val; dstT = tg_val; ds = d_ic;
  } else if (i < n_res + n_ic + n_bc) {
    seg = 2; out = i - n_res; gidx = off_bc + (out - n_ic); dstX = X_val; dstT = tg_val; ds = d_bc;
  } else {
    return;
  }
  const int64_t idx = qc_draw_index(seg, gidx, ds.n, seed, step);   // < ds.n: the product's high word
  dstX[out * 3 + 0] = ds.X[idx * 3 + 0];
  dstX[out * 3 + 1] = ds.X[idx * 3 + 1];
  dstX[out * 3 + 2] = ds.X[idx * 3 + 2];
  dstT[out] = ds.tg[idx];
  if (seg == 0) {
#pragma unroll
    for (int k = 0; k < QC_COEF_N; ++k) coef_res[(int64_t)k * n_res + out] = ds_coef[idx * QC_COEF_N + k];
  }
}

// The same gather with the residual row drawn from the integer CDF of qc_adapt_build (residual-adaptive sampling):
// r64 = word 0 << 32 | word 1 of the block the uniform gather draws, t = umul64hi(r64, T) with T = cdf[N - 1], and
// idx = min{j : cdf[j] > t}: the coarse table (one entry per QC_ADAPT_ROWS rows) first, then that block of the CDF.  IC and
// BC points draw as in k_sample_dataset, so the value batches are those of the uniform step.  LDS: the blocks that hold
// residual points stage the coarse table (nb entries, at most QC_ADAPT_LDS_MAX; larger tables are searched in global memory) in shared memory first.  coef_res / ds_coef may be
// null.  T = 0 (no row has weight; qc_adapt_build never leaves that) takes the last row, in bounds.
constexpr int QC_ADAPT_LDS_MAX = 4096;   // coarse entries staged in LDS (32 KB): datasets up to 4 Mi residual rows

template <bool LDS>
__global__ void __launch_bounds__(256) k_sample_dataset_adaptive(float* __restrict__ X_res, float* __restrict__ tg_res,
                                                                 int64_t n_res, int64_t off_res, float* __restrict__ X_val,
                                                                 float* __restrict__ tg_val, int64_t n_ic, int64_t off_ic,
                                                                 int64_t n_bc, int64_t off_bc, QcDsSeg d_res, QcDsSeg d_ic,
                                                                 QcDsSeg d_bc, uint64_t seed, uint64_t step,
                                                                 float* __restrict__ coef_res, const float* __restrict__ ds_coef,
                                                                 const uint64_t* __restrict__ cdf,
                                                                 const uint64_t* __restrict__ coarse) {
  __shared__ uint64_t sh[LDS ? QC_ADAPT_LDS_MAX : 1];
  const int64_t N = d_res.n;
  const int64_t nb = (N + QC_ADAPT_ROWS - 1) / QC_ADAPT_ROWS;
  if (LDS && (int64_t)blockIdx.x * 256 < n_res) {   // block-uniform: every thread of the block reaches the barrier
    for (int64_t b = threadIdx.x; b < nb; b += 256) sh[b] = coarse[b];
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int seg;
  int64_t out, gidx;
  float *dstX, *dstT;
  QcDsSeg ds;
  if (i < n_res) {
    seg = 0; out = i; gidx = off_res + i; dstX = X_res; dstT = tg_res; ds = d_res;
  } else if (i < n_res + n_ic) {
    seg = 1; out = i - n_res; gidx = off_ic + out; dstX = X_val; dstT = tg_val; ds = d_ic;
  } else if (i < n_res + n_ic + n_bc) {
    seg = 2; out = i - n_res; gidx = off_bc + (out - n_ic); dstX = X_val; dstT = tg_val; ds = d_bc;
  } else {
    return;
  }
  int64_t idx;
  if (seg == 0) {
    const U4 ctr = {(uint32_t)gidx, (uint32_t)(gidx >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
    const U4 r = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t t = __umul64hi(((uint64_t)r.x << 32) | r.y, cdf[N - 1]);
    const uint64_t* top = LDS ? sh : coarse;
    int64_t lo = 0, hi = nb - 1;          // first block whose last CDF entry exceeds t (the last block if none does)
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (top[mid] > t) hi = mid;
      else lo = mid + 1;
    }
    hi = (lo + 1) * QC_ADAPT_ROWS < N ? (lo + 1) * QC_ADAPT_ROWS - 1 : N - 1;
    lo *= QC_ADAPT_ROWS;                  // first row of that block whose CDF entry exceeds t
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cdf[mid] > t) hi = mid;
      else lo = mid + 1;
    }
    idx = lo;
  } else {
    idx = qc_draw_index(seg, gidx, ds.n, seed, step);   // < ds.n: the product's high word
  }
  dstX[out * 3 + 0] = ds.X[idx * 3 + 0];
  dstX[out * 3 + 1] = ds.X[idx * 3 + 1];
  dstX[out * 3 + 2] = ds.X[idx * 3 + 2];
  dstT[out] = ds.tg[idx];
  if (seg == 0 && coef_res != nullptr) {
#pragma unroll
    for (int k = 0; k < QC_COEF_N; ++k) coef_res[(int64_t)k * n_res + out] = ds_coef[idx * QC_COEF_N + k];
  }
}

}  // namespace

int qc_sample_dataset_launch(float* X_res, float* tg_res, int64_t n_res, int64_t off_res, float* X_val, float* tg_val,
                             int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, const float* dsX_res,
                             const float* ds_r, int64_t ds_n_res, const float* dsX_ic, const float* ds_u_ic, int64_t ds_n_ic,
                             const float* dsX_bc, const float* ds_u_bc, int64_t ds_n_bc, uint64_t seed, uint64_t step,
                             hipStream_t st, float* coef_res, const float* ds_coef) {
  const int64_t total = n_res + n_ic + n_bc;
  if (total <= 0) return QC_OK;
  const QcDsSeg a = {dsX_res, ds_r, ds_n_res}, b = {dsX_ic, ds_u_ic, ds_n_ic}, c = {dsX_bc, ds_u_bc, ds_n_bc};
  if (coef_res != nullptr && ds_coef != nullptr) {   // the coefficient step: rows, targets and operator rows in one launch
    hipLaunchKernelGGL(k_sample_dataset_coef, dim3(qc_ceil_div(total, 256)), dim3(256), 0, st, X_res, tg_res, n_res, off_res,
                       X_val, tg_val, n_ic, off_ic, n_bc, off_bc, a, b, c, seed, step, coef_res, ds_coef);
    return QC_OK;
  }
  hipLaunchKernelGGL(k_sample_dataset, dim3(qc_ceil_div(total, 256)), dim3(256), 0, st, X_res, tg_res, n_res, off_res, X_val,
                     tg_val, n_ic, off_ic, n_bc, off_bc, a, b, c, seed, step);
  return QC_OK;
}

int qc_sample_launch(float* X_res, int64_t n_res, int64_t off_res, float* X_val, int64_t n_ic, int64_t off_ic,
                     int64_t n_bc, int64_t off_bc, int64_t bc_face_points, uint64_t seed, uint64_t step, hipStream_t st) {
  const int64_t total = n_res + n_ic + n_bc;
  if (total <= 0) return QC_OK;
  if (bc_face_points < 0)
    hipLaunchKernelGGL(k_sample<true>, dim3(qc_ceil_div(total, 256)), dim3(256), 0, st, X_res, n_res, off_res, X_val, n_ic,
                       off_ic, n_bc, off_bc, bc_face_points, seed, step);
  else
    hipLaunchKernelGGL(k_sample<false>, dim3(qc_ceil_div(total, 256)), dim3(256), 0, st, X_res, n_res, off_res, X_val, n_ic,
                       off_ic, n_bc, off_bc, bc_face_points, seed, step);
  return QC_OK;
}

// (defined last: the kernels that existed keep their places in the object file, DESIGN section 6 "Target kinds")
int qc_sample_dataset_adaptive_launch(float* X_res, float* tg_res, int64_t n_res, int64_t off_res, float* X_val, float* tg_val,
                                      int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, const float* dsX_res,
                                      const float* ds_r, int64_t ds_n_res, const float* dsX_ic, const float* ds_u_ic,
                                      int64_t ds_n_ic, const float* dsX_bc, const float* ds_u_bc, int64_t ds_n_bc, uint64_t seed,
                                      uint64_t step, hipStream_t st, float* coef_res, const float* ds_coef, const uint64_t* cdf,
                                      const uint64_t* coarse) {
  const int64_t total = n_res + n_ic + n_bc;
  if (total <= 0) return QC_OK;
  const QcDsSeg a = {dsX_res, ds_r, ds_n_res}, b = {dsX_ic, ds_u_ic, ds_n_ic}, c = {dsX_bc, ds_u_bc, ds_n_bc};
  const bool table = coef_res != nullptr && ds_coef != nullptr;
  const int64_t nb = (ds_n_res + QC_ADAPT_ROWS - 1) / QC_ADAPT_ROWS;
  if (nb <= QC_ADAPT_LDS_MAX)   // measured faster than the search from global memory alone
    hipLaunchKernelGGL(k_sample_dataset_adaptive<true>, dim3(qc_ceil_div(total, 256)), dim3(256), 0, st, X_res, tg_res, n_res,
                       off_res, X_val, tg_val, n_ic, off_ic, n_bc, off_bc, a, b, c, seed, step, table ? coef_res : nullptr,
                       table ? ds_coef : nullptr, cdf, coarse);
  else
    hipLaunchKernelGGL(k_sample_dataset_adaptive<false>, dim3(qc_ceil_div(total, 256)), dim3(256), 0, st, X_res, tg_res, n_res,
                       off_res, X_val, tg_val, n_ic, off_ic, n_bc, off_bc, a, b, c, seed, step, table ? coef_res : nullptr,
                       table ? ds_coef : nullptr, cdf, coarse);
  return QC_OK;
}
