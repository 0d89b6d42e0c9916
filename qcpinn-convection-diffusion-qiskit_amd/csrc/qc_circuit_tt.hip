// Seven-channel circuit stages (channel 6 = d2/dt2) of the register family, 2 <= n <= 5: launchers of the run-time
// interpreter kernels of qc_circuit_tt_kernels.h.  Angle encoding, no EMBED gates; the callers (qc_api.hip) have checked.
#include "qc_circuit_tt_kernels.h"

template <int N>
struct TtLaunch {
  using PG = DynProg<N>;
  static int fwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, float* qjets, int64_t B,
                 hipStream_t st) {
    hipLaunchKernelGGL(k_jets_tt_fwd<PG>, dim3(qc_ceil_div(B, 64)), dim3(64 * QC_NCH_TT), 0, st, pg->d_gates, trig, umat,
                       pg->n_gates, ajets, qjets, B, (qc_embed_flags(pg) & 2) ? 1 : 0);
    return QC_OK;
  }
  static int bwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, const float* qbar,
                 float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B, hipStream_t st) {
    // the seven-vector exchange: 112 KB at n = 5, one block per CU
    const size_t sh = ((size_t)QC_NCH_TT * (2u << N) * 64 + (size_t)QC_NCH_TT * pg->n_params + 2 * N * 64) * sizeof(float);
    if (sh > 160 * 1024) return QC_ERR_UNSUPPORTED;
    static bool attr_set = false;   // (one process per device, as k_jets_bwd's launcher)
    if (!attr_set) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_jets_tt_bwd<PG>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024) != hipSuccess)
        return QC_ERR_HIP;
      attr_set = true;
    }
    hipLaunchKernelGGL(k_jets_tt_bwd<PG>, dim3(qc_ceil_div(B, 64)), dim3(64 * QC_NCH_TT), sh, st, pg->d_gates, trig, umat,
                       pg->n_gates, pg->n_params, ajets, qbar, abar, part, part_stride, row0, B, (qc_embed_flags(pg) & 2) ? 1 : 0);
    return QC_OK;
  }
};

int qc_tt_circ_fwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, float* qjets, int64_t B,
                   hipStream_t st) {
  switch (pg->n_qubits) {
    case 2: return TtLaunch<2>::fwd(pg, trig, umat, ajets, qjets, B, st);
    case 3: return TtLaunch<3>::fwd(pg, trig, umat, ajets, qjets, B, st);
    case 4: return TtLaunch<4>::fwd(pg, trig, umat, ajets, qjets, B, st);
    case 5: return TtLaunch<5>::fwd(pg, trig, umat, ajets, qjets, B, st);
    default: return QC_ERR_UNSUPPORTED;
  }
}

int qc_tt_circ_bwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, const float* qbar,
                   float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B, hipStream_t st) {
  switch (pg->n_qubits) {
    case 2: return TtLaunch<2>::bwd(pg, trig, umat, ajets, qbar, abar, part, part_stride, row0, B, st);
    case 3: return TtLaunch<3>::bwd(pg, trig, umat, ajets, qbar, abar, part, part_stride, row0, B, st);
    case 4: return TtLaunch<4>::bwd(pg, trig, umat, ajets, qbar, abar, part, part_stride, row0, B, st);
    case 5: return TtLaunch<5>::bwd(pg, trig, umat, ajets, qbar, abar, part, part_stride, row0, B, st);
    default: return QC_ERR_UNSUPPORTED;
  }
}
