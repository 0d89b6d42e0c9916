// Collocation-point sampler: the three uniform batches of one training step in one launch.
//
// Replaces the three torch.rand draws + affine maps of the reference step
// (trainer/diffusion_train.py:9-20 boxes, :34-36 order IC -> BC1 -> residual; data/diffusion_dataset.py:12-19
// x = lo + (hi - lo) * rand).  Counter-based Philox4x32-10 keyed by (seed, step, batch id) and indexed
// by the GLOBAL point index, so a data-parallel run draws exactly the points the single-GPU run draws
// (each rank fills its shard of the same global batch) and no generator state lives on the host.
#include "qc_internal.h"
#include "qc_philox.h"

#include <tuple>
#include <type_traits>

namespace {

// Thread i of a launch over n_res + n_ic + n_bc points: its segment (0 residual, 1 IC, 2 BC; -1: past the last point),
// its row `out` of that segment's output buffers (value rows and value targets are laid out IC first, then BC, like
// X_val), its global index, where its point goes, the targets of its batch, and in dataset mode the resident segment it
// copies from.  Returned by value: handed out through a reference, `ds` went through scratch memory in the CDF gathers.
// SEG: the segment record, QcDsSeg (one target per row) or QcDsSegW (a row of w targets, the system step's tables).
template <class SEG>
struct QcSlotOf {
  int seg;
  int64_t out, gidx;
  float *X, *tg;   // X_batch + 3 * out; the batch's target buffer (indexed by out)
  SEG ds;
};
using QcSlot = QcSlotOf<QcDsSeg>;
struct QcDsSegW {
  const float* X;   // [n][3]
  const float* tg;  // [n][w] row-major, or null: no targets to copy
  int64_t n;
  int w;
};
struct QcDsSegSlab {   // the slab rule's segment record: the residual one carries the slab count
  const float* X;   // [n][3]
  const float* tg;  // [n]
  int64_t n;
  int n_slabs;
};
template <class SEG = QcDsSeg>
__device__ __forceinline__ QcSlotOf<SEG> qc_slot(int64_t i, float* X_res, float* tg_res, int64_t n_res, int64_t off_res, float* X_val,
                                                 float* tg_val, int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc,
                                                 SEG d_res = {}, SEG d_ic = {}, SEG d_bc = {}) {
  QcSlotOf<SEG> s;
  int64_t local;
  if (i < n_res) {
    local = i;
    s = {0, local, off_res + local, X_res + local * 3, tg_res, d_res};
  } else if (i < n_res + n_ic) {
    local = i - n_res;
    s = {1, local, off_ic + local, X_val + local * 3, tg_val, d_ic};
  } else if (i < n_res + n_ic + n_bc) {
    local = i - n_res - n_ic;
    s = {2, n_ic + local, off_bc + local, X_val + (n_ic + local) * 3, tg_val, d_bc};
  } else {
    s.seg = -1;
  }
  return s;
}

// segment 0: residual points in [0,1]^3; 1: IC points (t = 0); 2: boundary points: the x = 0 face
// (trainer/diffusion_train.py:13-16), or with face_pts > 0 the four faces x=0, x=1, y=0, y=1 of the second
// workload (train_hybrid_qpinn.py:166-176), face = global index / face_pts; RF (face_pts < 0): a random face per
// point (trainer/train.py:118-135, qc_philox.h)
template <bool RF>
__global__ void __launch_bounds__(256) k_sample(float* __restrict__ X_res, int64_t n_res, int64_t off_res,
                                                float* __restrict__ X_val, int64_t n_ic, int64_t off_ic,
                                                int64_t n_bc, int64_t off_bc, int64_t face_pts, uint64_t seed,
                                                uint64_t step) {
  const QcSlot s = qc_slot((int64_t)blockIdx.x * 256 + threadIdx.x, X_res, nullptr, n_res, off_res, X_val, nullptr, n_ic,
                           off_ic, n_bc, off_bc);
  if (s.seg < 0) return;
  float t, x, y;
  qc_draw_point<RF>(s.seg, s.gidx, face_pts, seed, step, t, x, y);
  s.X[0] = t;
  s.X[1] = x;
  s.X[2] = y;
}

// The search of the CDF gather (residual-adaptive sampling, the integer CDF of qc_adapt_build): min{j : cdf[j] > t}, in the
// coarse table `top` (nb entries, one per QC_ADAPT_ROWS rows) first, then in that block of the CDF.  t >= cdf[N - 1] (only
// with cdf[N - 1] = 0, no row has weight, which qc_adapt_build never leaves) takes the last row, in bounds.
__device__ __forceinline__ int64_t qc_cdf_search(uint64_t t, const uint64_t* __restrict__ cdf, const uint64_t* top, int64_t N,
                                                 int64_t nb) {
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
  return lo;
}

// Dataset mode of the same launch (the tabulated step), ONE template for every QcSource of rows: point i of a segment
// copies row idx of that segment's resident dataset and its target.  ROWS is the rule for idx.  Uniform: qc_draw_index
// on the counter the coordinate draw uses.  The two CDF rules: a residual point searches the CDF (qc_cdf_search), IC and
// BC points draw as before, so the value batches are those of the uniform gather; the blocks that hold residual points
// first stage the coarse table in shared memory (at most QC_ADAPT_LDS_MAX entries), or with QC_ROWS_CDF_GLOBAL every
// search reads it where it lies.
// `src` is the source's optional pointers as a trailing pack, so the plain gather carries no argument for them:
// nothing; (coef_res, ds_coef): a residual point also copies its operator row, ds_coef[idx][7] -> coef_res[7][n_res]
// (batch-minor); (coef_res, ds_coef, cdf, coarse) for the CDF rules, where coef_res / ds_coef may be null.
template <int K, class... P>
__device__ __forceinline__ auto qc_src(P*... src) {   // pointer K of the pack, null behind its end
  if constexpr (K < sizeof...(P)) return std::get<K>(std::tie(src...));
  else return nullptr;
}
// The slab rule (the causal step; SEG = QcDsSegSlab, `src` = (slab_lo)): a residual point with global index g draws inside
// slab (g / 64) mod n_slabs of the residual segment, rows [slab_lo[s], slab_lo[s + 1]), with the word the uniform gather
// draws for it; IC and BC points draw as before.  An empty slab gives the row at its offset, and the index is clamped into
// the segment, so no table reads outside it.
enum QcRows { QC_ROWS_UNIFORM = 0, QC_ROWS_CDF_LDS, QC_ROWS_CDF_GLOBAL, QC_ROWS_SLABS };
constexpr int QC_ADAPT_LDS_MAX = 4096;   // coarse entries staged in LDS (32 KB): datasets up to 4 Mi residual rows

// SEG = QcDsSegW: the targets of a row are ds.w floats, written batch-minor (tg[k][batch]); a segment without a table
// (the residual targets of a system may be absent: zero) copies points only.
template <QcRows ROWS, class SEG, class... P>
__global__ void __launch_bounds__(256) k_gather(float* __restrict__ X_res, float* __restrict__ tg_res, int64_t n_res,
                                                int64_t off_res, float* __restrict__ X_val, float* __restrict__ tg_val,
                                                int64_t n_ic, int64_t off_ic, int64_t n_bc, int64_t off_bc, SEG d_res,
                                                SEG d_ic, SEG d_bc, uint64_t seed, uint64_t step,
                                                P* __restrict__... src) {
  constexpr bool SLABS = ROWS == QC_ROWS_SLABS;
  constexpr bool CDF = ROWS == QC_ROWS_CDF_LDS || ROWS == QC_ROWS_CDF_GLOBAL, LDS = ROWS == QC_ROWS_CDF_LDS;
  constexpr bool TABLE = !SLABS && sizeof...(P) >= 2;
  constexpr bool WIDE = std::is_same<SEG, QcDsSegW>::value;
  float* coef_res = nullptr;
  const float* ds_coef = nullptr;
  [[maybe_unused]] const int64_t* slab_lo = nullptr;
  if constexpr (SLABS) {
    slab_lo = qc_src<0>(src...);
  } else {
    coef_res = qc_src<0>(src...);
    ds_coef = qc_src<1>(src...);
  }
  const uint64_t *cdf = qc_src<2>(src...), *coarse = qc_src<3>(src...);
  __shared__ uint64_t sh[LDS ? QC_ADAPT_LDS_MAX : 1];
  const int64_t N = d_res.n;
  const int64_t nb = (N + QC_ADAPT_ROWS - 1) / QC_ADAPT_ROWS;
  if (LDS && (int64_t)blockIdx.x * 256 < n_res) {   // block-uniform: every thread of the block reaches the barrier
    for (int64_t b = threadIdx.x; b < nb; b += 256) sh[b] = coarse[b];
    __syncthreads();
  }
  const QcSlotOf<SEG> s = qc_slot<SEG>((int64_t)blockIdx.x * 256 + threadIdx.x, X_res, tg_res, n_res, off_res, X_val, tg_val, n_ic,
                                       off_ic, n_bc, off_bc, d_res, d_ic, d_bc);
  if (s.seg < 0) return;
  int64_t idx;
  if (CDF && s.seg == 0) {   // t = umul64hi(r64, cdf[N - 1]), r64 = word 0 << 32 | word 1 of the uniform gather's block
    const U4 ctr = {(uint32_t)s.gidx, (uint32_t)(s.gidx >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
    const U4 r = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
    idx = qc_cdf_search(__umul64hi(((uint64_t)r.x << 32) | r.y, cdf[N - 1]), cdf, LDS ? sh : coarse, N, nb);
  } else if (SLABS && s.seg == 0) {
    if constexpr (SLABS) {
      const int sl = (int)((uint64_t)(s.gidx >> 6) % (uint32_t)s.ds.n_slabs);
      const int64_t lo = slab_lo[sl], w = slab_lo[sl + 1] - lo;
      idx = lo + (w > 0 ? qc_draw_index(0, s.gidx, w, seed, step) : 0);
      idx = idx < 0 ? 0 : (idx < N ? idx : N - 1);
    }
  } else {
    idx = qc_draw_index(s.seg, s.gidx, s.ds.n, seed, step);   // < ds.n: the product's high word
  }
  s.X[0] = s.ds.X[idx * 3 + 0];
  s.X[1] = s.ds.X[idx * 3 + 1];
  s.X[2] = s.ds.X[idx * 3 + 2];
  if constexpr (WIDE) {
    if (s.ds.tg && s.tg) {
      const int64_t nb_out = s.seg == 0 ? n_res : n_ic + n_bc;
      for (int k = 0; k < s.ds.w; ++k) s.tg[(int64_t)k * nb_out + s.out] = s.ds.tg[idx * s.ds.w + k];
    }
  } else {
    s.tg[s.out] = s.ds.tg[idx];
  }
  if (TABLE && s.seg == 0 && (!CDF || coef_res != nullptr)) {
#pragma unroll
    for (int k = 0; k < QC_COEF_N; ++k) coef_res[(int64_t)k * n_res + s.out] = ds_coef[idx * QC_COEF_N + k];
  }
}

// Implicit instantiations are emitted in order of first use, and where identical kernels lie in the object has been
// measured (DESIGN section 6 "Batch sources"): the two uniform gathers are named here, ahead of qc_sample_launch, so the
// order stays uniform, uniform with a table, k_sample<true>, k_sample<false>, CDF from LDS, CDF from global memory, the slab rule.
constexpr auto k_gather_rows = k_gather<QC_ROWS_UNIFORM, QcDsSeg>;
constexpr auto k_gather_rows_coef = k_gather<QC_ROWS_UNIFORM, QcDsSeg, float, const float>;
template <QcRows ROWS>
constexpr auto k_gather_cdf = k_gather<ROWS, QcDsSeg, float, const float, const uint64_t, const uint64_t>;

}  // namespace

int qc_sample_launch(const QcBatches& b, int64_t bc_face_points, hipStream_t st) {
  const int64_t total = b.n_res + b.n_ic + b.n_bc;
  if (total <= 0) return QC_OK;
  hipLaunchKernelGGL((bc_face_points < 0 ? k_sample<true> : k_sample<false>), dim3(qc_ceil_div(total, 256)), dim3(256), 0, st,
                     b.X_res, b.n_res, b.off_res, b.X_val, b.n_ic, b.off_ic, b.n_bc, b.off_bc, bc_face_points, b.seed, b.step);
  return QC_OK;
}

// the dataset kinds of QcSource (validated with QcSource::ok): one launch, the kernel by kind, table and table size
int qc_gather_launch(const QcBatches& b, const QcSource& s, hipStream_t st) {
  const int64_t total = b.n_res + b.n_ic + b.n_bc;
  if (total <= 0) return QC_OK;
  auto launch = [&](auto kernel, auto... src) {
    hipLaunchKernelGGL(kernel, dim3(qc_ceil_div(total, 256)), dim3(256), 0, st, b.X_res, b.tg_res, b.n_res, b.off_res, b.X_val,
                       b.tg_val, b.n_ic, b.off_ic, b.n_bc, b.off_bc, s.res, s.ic, s.bc, b.seed, b.step, src...);
  };
  if (s.w_res > 0 || s.w_val > 0) {   // a system's dataset: rows of targets (uniform rows, no operator table)
    const QcDsSegW r = {s.res.X, s.res.tg, s.res.n, s.w_res}, i = {s.ic.X, s.ic.tg, s.ic.n, s.w_val},
                   c = {s.bc.X, s.bc.tg, s.bc.n, s.w_val};
    hipLaunchKernelGGL((k_gather<QC_ROWS_UNIFORM, QcDsSegW>), dim3(qc_ceil_div(total, 256)), dim3(256), 0, st, b.X_res, b.tg_res,
                       b.n_res, b.off_res, b.X_val, b.tg_val, b.n_ic, b.off_ic, b.n_bc, b.off_bc, r, i, c, b.seed, b.step);
    return QC_OK;
  }
  const bool table = s.table && b.n_res > 0;   // no residual rows: none to copy an operator row for
  float* coef_res = table ? s.coef_res : nullptr;
  const float* ds_coef = table ? s.ds_coef : nullptr;
  if (s.kind == QC_SOURCE_ROWS) {
    if (table) launch(k_gather_rows_coef, coef_res, ds_coef);   // rows, targets and operator rows in one launch
    else launch(k_gather_rows);
  } else if (s.kind == QC_SOURCE_CDF && (s.res.n + QC_ADAPT_ROWS - 1) / QC_ADAPT_ROWS <= QC_ADAPT_LDS_MAX) {
    // measured faster than the search from global memory alone
    launch(k_gather_cdf<QC_ROWS_CDF_LDS>, coef_res, ds_coef, s.cdf, s.coarse);
  } else if (s.kind == QC_SOURCE_CDF) {
    launch(k_gather_cdf<QC_ROWS_CDF_GLOBAL>, coef_res, ds_coef, s.cdf, s.coarse);
  } else {
    // the slab rule, first used here so that its kernel lies behind every other gather of the object
    const QcDsSegSlab r = {s.res.X, s.res.tg, s.res.n, s.n_slabs}, i = {s.ic.X, s.ic.tg, s.ic.n, 0}, c = {s.bc.X, s.bc.tg, s.bc.n, 0};
    hipLaunchKernelGGL((k_gather<QC_ROWS_SLABS, QcDsSegSlab, const int64_t>), dim3(qc_ceil_div(total, 256)), dim3(256), 0, st,
                       b.X_res, b.tg_res, b.n_res, b.off_res, b.X_val, b.tg_val, b.n_ic, b.off_ic, b.n_bc, b.off_bc, r, i, c, b.seed,
                       b.step, s.slab_lo);
  }
  return QC_OK;
}
