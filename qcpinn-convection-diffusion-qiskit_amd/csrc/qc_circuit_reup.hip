// Re-uploading family dispatch: run-time interpreter kernels for gate programs with EMBED / EMBED_S gates, 2 <= n <= 5.
#include "qc_circuit_reup_kernels.h"

// SCALED: the program holds EMBED_S gates (pg->embed_scaled)
template <int N, bool SCALED>
struct ReupLaunch {
  static int fwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* in, float* out, int64_t B, int nch,
                 hipStream_t st) {
    if (nch == 1)
      hipLaunchKernelGGL((k_reup_value_fwd<N, SCALED>), dim3(qc_ceil_div(B, 256)), dim3(256), 0, st, pg->d_gates, trig, umat,
                         pg->n_gates, in, out, B);
    else
      hipLaunchKernelGGL((k_reup_jets_fwd<N, SCALED>), dim3(qc_ceil_div(B, 64)), dim3(384), 0, st, pg->d_gates, trig, umat,
                         pg->n_gates, in, out, B);
    return QC_OK;
  }
  static int bwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* in, const float* cot, float* d_in,
                 float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, hipStream_t st) {
    if (nch == 1) {
      const size_t sh = (size_t)4 * pg->n_params * sizeof(float);
      if (sh > 64 * 1024) return QC_ERR_UNSUPPORTED;
      hipLaunchKernelGGL((k_reup_value_bwd<N, SCALED>), dim3(qc_ceil_div(B, 256)), dim3(256), sh, st, pg->d_gates, trig, umat,
                         pg->n_gates, pg->n_params, in, cot, d_in, part, part_stride, row0, B);
      return QC_OK;
    }
    // the six-vector exchange is sized by the template parameter: 96 KB at n = 5
    const size_t sh = ((size_t)6 * (2u << N) * 64 + (size_t)6 * pg->n_params + (SCALED ? 4 : 2) * N * 64) * sizeof(float);
    if (sh > 160 * 1024) return QC_ERR_UNSUPPORTED;
    static bool attr_set = false;   // (one process per device, as k_jets_bwd's launcher)
    if (!attr_set) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_reup_jets_bwd<N, SCALED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024) != hipSuccess)
        return QC_ERR_HIP;
      attr_set = true;
    }
    hipLaunchKernelGGL((k_reup_jets_bwd<N, SCALED>), dim3(qc_ceil_div(B, 64)), dim3(384), sh, st, pg->d_gates, trig, umat, pg->n_gates,
                       pg->n_params, in, cot, d_in, part, part_stride, row0, B);
    return QC_OK;
  }
};

// nch = 1: value kernels; 6: jet kernels.  Nothing is kept: the adjoint kernels recompute the forward sweep.
static int reup_fwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* in, float* out, int64_t B,
                    int nch, QcCircStore, hipStream_t st) {
  if (pg->amplitude) return QC_ERR_UNSUPPORTED;
  switch (pg->n_qubits) {
    case 2: return pg->embed_scaled ? ReupLaunch<2, true>::fwd(pg, trig, umat, in, out, B, nch, st)
                                    : ReupLaunch<2, false>::fwd(pg, trig, umat, in, out, B, nch, st);
    case 3: return pg->embed_scaled ? ReupLaunch<3, true>::fwd(pg, trig, umat, in, out, B, nch, st)
                                    : ReupLaunch<3, false>::fwd(pg, trig, umat, in, out, B, nch, st);
    case 4: return pg->embed_scaled ? ReupLaunch<4, true>::fwd(pg, trig, umat, in, out, B, nch, st)
                                    : ReupLaunch<4, false>::fwd(pg, trig, umat, in, out, B, nch, st);
    case 5: return pg->embed_scaled ? ReupLaunch<5, true>::fwd(pg, trig, umat, in, out, B, nch, st)
                                    : ReupLaunch<5, false>::fwd(pg, trig, umat, in, out, B, nch, st);
    default: return QC_ERR_UNSUPPORTED;
  }
}
static int reup_bwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* in, const float* cot,
                    float* d_in, float* part, int64_t part_stride, int64_t row0, int64_t B, int nch, QcCircStore,
                    hipStream_t st) {
  if (pg->amplitude) return QC_ERR_UNSUPPORTED;
  switch (pg->n_qubits) {
    case 2: return pg->embed_scaled ? ReupLaunch<2, true>::bwd(pg, trig, umat, in, cot, d_in, part, part_stride, row0, B, nch, st)
                                    : ReupLaunch<2, false>::bwd(pg, trig, umat, in, cot, d_in, part, part_stride, row0, B, nch, st);
    case 3: return pg->embed_scaled ? ReupLaunch<3, true>::bwd(pg, trig, umat, in, cot, d_in, part, part_stride, row0, B, nch, st)
                                    : ReupLaunch<3, false>::bwd(pg, trig, umat, in, cot, d_in, part, part_stride, row0, B, nch, st);
    case 4: return pg->embed_scaled ? ReupLaunch<4, true>::bwd(pg, trig, umat, in, cot, d_in, part, part_stride, row0, B, nch, st)
                                    : ReupLaunch<4, false>::bwd(pg, trig, umat, in, cot, d_in, part, part_stride, row0, B, nch, st);
    case 5: return pg->embed_scaled ? ReupLaunch<5, true>::bwd(pg, trig, umat, in, cot, d_in, part, part_stride, row0, B, nch, st)
                                    : ReupLaunch<5, false>::bwd(pg, trig, umat, in, cot, d_in, part, part_stride, row0, B, nch, st);
    default: return QC_ERR_UNSUPPORTED;
  }
}
static size_t reup_store_bytes(const qc_program*, int, int64_t) { return 0; }
QcFamily qc_family_reup = {reup_fwd, reup_bwd, reup_store_bytes};
