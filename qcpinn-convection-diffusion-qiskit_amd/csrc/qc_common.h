// Shared definitions for the gfx950 QCPINN kernels (device + host side of the C-ABI library).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qc_types.h"

// Channel numbering of the derivative ("jet") channels carried through the network:
// 0 value, 1 d/dt, 2 d/dx, 3 d/dy, 4 d2/dx2, 5 d2/dy2.
#define QC_NCH 6

#define QC_WAVE 64

static inline int qc_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------------------ wave-level reductions
// ---- fused diagonal runs (register family, n <= 5; compile-time programs of the wave family: qc_wave_sched.h)
// A run of >= 2 consecutive RZ / CRZ gates is one element-wise multiply by D[k] = prod_g phase_g(k), phase =
// c -+ i s by the target bit (CRZ: only where the control bit is set).  The tables live behind the n_gates per-gate
// entries of the trig buffer ({c, s} = {Re D, Im D}), run r at [n_gates + r * 2^n, ...), and are rebuilt with it.
__host__ __device__ inline bool qc_is_diag_op(int op) { return op == 2 /* QC_RZ */ || op == 6 /* QC_CRZ */; }

struct QcDiagRuns {   // kernel-argument copy of qc_program's run list
  int n;
  int g0[QC_MAX_DIAG_RUNS], g1[QC_MAX_DIAG_RUNS];
  const int* list;    // null: run r = gates g0[r] .. g1[r]-1; else gates list[g0[r]] .. list[g1[r]-1] (qc_wave_sched.h)
};

// fills pg->n_diag_runs / diag_g0 / diag_g1 (host); more than QC_MAX_DIAG_RUNS runs: none is fused
inline void qc_find_diag_runs(qc_program* pg) {
  pg->n_diag_runs = 0;
  pg->d_diag_list = nullptr;
  if (pg->n_qubits > 5) return;
  for (int g = 0; g < pg->n_gates;) {
    if (!qc_is_diag_op(pg->h_gates[g].op)) { ++g; continue; }
    int e = g;
    while (e < pg->n_gates && qc_is_diag_op(pg->h_gates[e].op)) ++e;
    if (e - g >= 2) {
      if (pg->n_diag_runs == QC_MAX_DIAG_RUNS) { pg->n_diag_runs = 0; return; }
      pg->diag_g0[pg->n_diag_runs] = g;
      pg->diag_g1[pg->n_diag_runs] = e;
      ++pg->n_diag_runs;
    }
    g = e;
  }
}
inline QcDiagRuns qc_diag_runs_of(const qc_program* pg) {
  QcDiagRuns r;
  r.n = pg ? pg->n_diag_runs : 0;
  r.list = pg ? pg->d_diag_list : nullptr;
  for (int i = 0; i < QC_MAX_DIAG_RUNS; ++i) {
    r.g0[i] = (pg && i < r.n) ? pg->diag_g0[i] : 0;
    r.g1[i] = (pg && i < r.n) ? pg->diag_g1[i] : 0;
  }
  return r;
}

// one thread per amplitude k (tid < 2^n) after the per-gate entries of `trig` are complete and block-visible.
// (`cs`: optional LDS copy [n_gates][2] of the (cos, sin) pairs; else read back from `trig`)
__device__ inline void qc_fill_diag_tables(const QcGate* __restrict__ prog, int n_gates, int n_qubits,
                                           QcTrig* __restrict__ trig, int tid, const QcDiagRuns& runs,
                                           const float* cs = nullptr) {
  if (runs.n == 0 || n_qubits > 8 || tid >= (1 << n_qubits)) return;
  const int k = tid;
  for (int r = 0; r < runs.n; ++r) {
    float dr = 1.f, di = 0.f;
    for (int hh = runs.g0[r]; hh < runs.g1[r]; ++hh) {
      const int h = runs.list ? runs.list[hh] : hh;
      const QcGate gt = prog[h];
      const bool ctl = gt.op == 6;
      const int tb = ctl ? gt.bb : gt.ba;
      const float c = cs ? cs[2 * h] : trig[h].c, s0 = cs ? cs[2 * h + 1] : trig[h].s;
      if (ctl && !((k >> gt.ba) & 1)) continue;
      const float s = ((k >> tb) & 1) ? s0 : -s0;
      const float nr = dr * c - di * s, ni = dr * s + di * c;
      dr = nr;
      di = ni;
    }
    QcTrig t = {dr, di, 0.f, 0.f};
    trig[n_gates + r * (1 << n_qubits) + k] = t;
  }
}

// ---- the same tables in a one-block kernel that moves theta itself (k_adam_fast, k_lbfgs: T threads)
// Such a kernel is one chain of memory latencies, so everything the tables need besides theta is requested at kernel
// entry, in the round trip of the kernel's other loads (qc_gate_stage_load): the gate record whose sincosf a thread will
// compute stays in its registers, and where the program has phase tables (runs.n > 0, n <= 8) the records and the device
// run list are parked in dynamic LDS (qc_gate_stage_store, ahead of any barrier the kernel passes before
// qc_gate_stage_tables).  Behind the update the tables then come from LDS alone: no global or scalar load, and no wait
// for the per-gate stores.  A program without tables takes no LDS.
// LDS image at `lds` (16-byte aligned), in words: gate records [n_gates][4], (cos, sin) [n_gates][2], run list [n_list].
struct QcGateStage {
  QcGate mine;     // gate `tid` of the program (tid < n_gates): its sincosf is this thread's
  int list_mine;   // entry `tid` of the device run list (tid < n_list)
  int n_list;      // 0: the runs are gate ranges
  bool tables;     // the program has phase tables: the LDS image exists
  int words;       // words of the image (what follows it in a kernel's dynamic LDS starts there)
  QcGate* gates;
  float* cs;
  int* list;
};
__host__ __device__ inline bool qc_gate_stage_has_tables(const int n_qubits, const QcDiagRuns& runs) {
  return runs.n > 0 && n_qubits <= 8;   // (qc_fill_diag_tables' condition)
}
__host__ __device__ inline int qc_gate_stage_list_len(const QcDiagRuns& runs) {
  int e = 0;   // g1 of the last run (run_off of qc_wave_sched.h: ascending), without a run-time index into the arguments
#pragma unroll
  for (int q = 0; q < QC_MAX_DIAG_RUNS; ++q)
    if (q < runs.n) e = runs.g1[q];
  return runs.list != nullptr ? e : 0;
}
// words of the image: the kernels' dynamic LDS starts with them
__host__ __device__ inline int qc_gate_stage_words(const int n_gates, const int n_qubits, const QcDiagRuns& runs) {
  return qc_gate_stage_has_tables(n_qubits, runs) ? 6 * n_gates + qc_gate_stage_list_len(runs) : 0;
}
inline size_t qc_gate_stage_words(const qc_program* pg) {
  return pg ? (size_t)qc_gate_stage_words(pg->n_gates, pg->n_qubits, qc_diag_runs_of(pg)) : 0;
}
__device__ __forceinline__ QcGateStage qc_gate_stage_load(const QcGate* __restrict__ prog, const int n_gates, const int n_qubits,
                                                          const QcDiagRuns& runs, float* lds, const int tid) {
  QcGateStage sg;
  sg.mine = QcGate{0, 0, 0, -1};
  sg.list_mine = 0;
  sg.tables = prog != nullptr && qc_gate_stage_has_tables(n_qubits, runs);
  sg.n_list = sg.tables ? qc_gate_stage_list_len(runs) : 0;
  sg.words = sg.tables ? 6 * n_gates + sg.n_list : 0;   // == qc_gate_stage_words
  sg.gates = reinterpret_cast<QcGate*>(lds);
  sg.cs = lds + 4 * n_gates;
  sg.list = reinterpret_cast<int*>(lds + 6 * n_gates);
  if (prog != nullptr && tid < n_gates) sg.mine = prog[tid];
  if (tid < sg.n_list) sg.list_mine = runs.list[tid];
  return sg;
}
template <int T>
__device__ __forceinline__ void qc_gate_stage_store(const QcGateStage& sg, const QcGate* __restrict__ prog, const int n_gates,
                                                    const QcDiagRuns& runs, const int tid) {
  if (!sg.tables) return;
  if (tid < n_gates) sg.gates[tid] = sg.mine;
  if (tid < sg.n_list) sg.list[tid] = sg.list_mine;
  // (more than T gates or entries: no program with tables has them)
#pragma unroll 1
  for (int g = tid + T; g < n_gates; g += T) sg.gates[g] = prog[g];
#pragma unroll 1
  for (int e = tid + T; e < sg.n_list; e += T) sg.list[e] = runs.list[e];
}
// LDS traffic of this wave complete, then the block's barrier: what a __syncthreads() is without its wait for the
// outstanding global stores (nothing behind it reads what they wrote)
__device__ __forceinline__ void qc_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// `theta`: the NEW [n_theta], block-visible (LDS, or global behind a __syncthreads()).  Per-gate entries as k_prep_trig
// forms them; then one thread per (run, amplitude) pair, the product over the run's gates in qc_fill_diag_tables' order
// and expressions, so every entry has that function's bits.
template <int T>
__device__ __forceinline__ void qc_gate_stage_tables(const QcGateStage& sg, const QcGate* __restrict__ prog, const int n_gates,
                                                     const int n_qubits, const int n_theta, QcTrig* __restrict__ trig,
                                                     const QcDiagRuns& runs, const float* theta, const int tid) {
  const bool tables = sg.tables;
  for (int gi = tid; gi < n_gates; gi += T) {
    // (gates T, T + 1, ..: only a program without tables has them, and it has no image)
    const QcGate gt = gi == tid ? sg.mine : (tables ? sg.gates[gi] : prog[gi]);
    QcTrig tr = {1.f, 0.f, 0.f, 0.f};
    if (gt.op != QC_U4 && gt.slot >= 0 && gt.slot < n_theta) {
      tr.th = theta[gt.slot];
      sincosf(0.5f * tr.th, &tr.s, &tr.c);
    }
    trig[gi] = tr;
    if (tables) {
      sg.cs[2 * gi] = tr.c;
      sg.cs[2 * gi + 1] = tr.s;
    }
  }
  if (!tables) return;
  qc_lds_barrier();
  const int A = 1 << n_qubits;
  for (int p = tid; p < runs.n * A; p += T) {
    const int r = p >> n_qubits, k = p & (A - 1);
    int g0 = 0, g1 = 0;   // (a compile-time chain: a run-time index would fetch them from the kernel's argument segment)
#pragma unroll
    for (int q = 0; q < QC_MAX_DIAG_RUNS; ++q)
      if (r == q) {
        g0 = runs.g0[q];
        g1 = runs.g1[q];
      }
    float dr = 1.f, di = 0.f;
    for (int hh = g0; hh < g1; ++hh) {
      const int h = sg.n_list > 0 ? sg.list[hh] : hh;
      const QcGate gt = sg.gates[h];
      const bool ctl = gt.op == 6;
      const int tb = ctl ? gt.bb : gt.ba;
      const float c = sg.cs[2 * h], s0 = sg.cs[2 * h + 1];
      if (ctl && !((k >> gt.ba) & 1)) continue;
      const float s = ((k >> tb) & 1) ? s0 : -s0;
      const float nr = dr * c - di * s, ni = dr * s + di * c;
      dr = nr;
      di = ni;
    }
    QcTrig t = {dr, di, 0.f, 0.f};
    trig[n_gates + r * A + k] = t;
  }
}

// Sum over the 64 lanes of a wave with DPP row operations (no LDS traffic).  The total is
// valid in lane 63 (and only there).
__device__ __forceinline__ float qc_wave_sum_to_lane63(float v) {
  // quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror, row_bcast15, row_bcast31
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, false));
  return v;
}

// The same sum for NV independent values at once (valid in lane 63 of each): the four in-row steps interleaved over
// the values, the two row_bcast steps as ONE v_add_f32_dpp each with a row mask (the compiler expands the builtin form
// of those two steps into v_mov 0 / v_mov_dpp / v_add: ten instructions per value instead of six).
template <int NV>
__device__ __forceinline__ void qc_wave_sum_multi_to_lane63(float (&v)[NV]) {
#define QC_DPP_STEP_(CTRL)                                                                                       \
  _Pragma("unroll") for (int k = 0; k < NV; ++k)                                                                 \
    v[k] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[k]), CTRL, 0xF, 0xF, true));
  QC_DPP_STEP_(0xB1) QC_DPP_STEP_(0x4E) QC_DPP_STEP_(0x141) QC_DPP_STEP_(0x140)
#undef QC_DPP_STEP_
  // every value's last in-row step is complete before the hand-written DPP reads (the assembler does not pad the
  // VALU-write -> DPP-read hazard inside asm: two wait states, provided by the s_nop and by the other values' steps)
#pragma unroll
  for (int k = 0; k < NV; ++k) asm volatile("" : "+v"(v[k]));
  asm volatile("s_nop 1");
#pragma unroll
  for (int k = 0; k < NV; ++k) asm volatile("v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(v[k]));
  if constexpr (NV < 3) asm volatile("s_nop 1");
#pragma unroll
  for (int k = 0; k < NV; ++k) asm volatile("v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(v[k]));
}

// Sum over the wave, result broadcast to every lane (uniform value).
__device__ __forceinline__ float qc_wave_sum(float v) {
  v = qc_wave_sum_to_lane63(v);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
