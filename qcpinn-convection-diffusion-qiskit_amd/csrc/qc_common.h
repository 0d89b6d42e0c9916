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

typedef float qf2 __attribute__((ext_vector_type(2)));   // an amplitude (re, im), or two fp32 lanes of a packed instruction

// ------------------------------------------------------------------ write-through stores of stage outputs
// qc_store_wt(p, v): *p = v as a relaxed agent-scope store, global_store_dword / _dwordx2 ... sc1 on gfx950, with no
// fence and no wait.  A plain store stays dirty in the writing XCD's L2 until the release at the end of the kernel
// writes it back, after the last wave has stopped computing; an sc1 store goes through to memory when it is issued, so
// that write-back has nothing left to do for it.  The stored bits are those of the plain store.  Rules:
//   * for outputs whose consumer is a LATER launch (its plain loads are then valid: the launch boundary makes every
//     completed store visible) and where one wave instruction writes whole 128-byte lines (lane = consecutive element);
//     a partial line goes to memory as a partial write;
//   * never for a value that another block reads back within the SAME launch: the store drops the line from this XCD's
//     L2 and orders nothing;
//   * never together with nt (nt is no write-through).
// A site takes the policy only where a kernel trace shows its kernel shorter and its consumers no longer (DESIGN
// section 8.0000000): the angle jets of the pre-network forward bodies and qbar of the fused post bodies.  The
// final-state hand-off (qc_chi_write, the only 8-byte site tried), the <Z> jets and the adjoint stage's abar / d_angles
// stay plain: written through, the first made the kernels that read it longer by more than the writer gained, the
// second made its own kernel longer, the third gained no more than the control runs differ.
// The host pass sees a plain store.  tools/ubench/store_policy.hip checks both forms across launches and XCDs.
__host__ __device__ __forceinline__ void qc_store_wt(float* p, const float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p = v;
#endif
}
__host__ __device__ __forceinline__ void qc_store_wt(qf2* p, const qf2 v) {   // 8-byte aligned, as every qf2 is
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_store(reinterpret_cast<uint64_t*>(p), __builtin_bit_cast(uint64_t, v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
#else
  *p = v;
#endif
}

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

// One value, lane 63, in six VALU instructions: the chain above with both row_bcast steps as single v_add_f32_dpp.
__device__ __forceinline__ float qc_wave_sum6_to_lane63(float v) {
  float t[1] = {v};
  qc_wave_sum_multi_to_lane63<1>(t);
  return t[0];
}

// ------------------------------------------------------------------ merged wave sums
// qc_wave_sum_merged<NV>(v): the NV sums of qc_wave_sum_to_lane63 with the SAME association tree, in fewer
// instructions: from the third level on, several values share one register and the level runs once for all of them.
//
// The tree of qc_wave_sum_to_lane63, by the lane bit a level folds:
//   bit 0  quad_perm[1,0,3,2]     s1[l] = x[l] + x[l^1]
//   bit 1  quad_perm[2,3,0,1]     q  = s1[l] + s1[l^2]             (one value per quad, in all four of its lanes)
//   bit 2  row_half_mirror        h  = q(bank 2j) + q(bank 2j+1)   (one value per 8-lane half-row)
//   bit 3  row_mirror             r  = h(half-row 0) + h(half-row 1)   (one value per 16-lane row)
//   bit 4  row_bcast15, rows 1,3  p  = r(row 2j) + r(row 2j+1)
//   bit 5  row_bcast31, rows 2,3  total = p(rows 0,1) + p(rows 2,3)
// Every level adds two partial sums of the level before, and which two is all the tree fixes.  fp32 addition is
// commutative (a + b and b + a are the same bits), so neither the lane that forms a sum nor the order of its two operands
// changes it.  The merged schedule forms, at every level, sums of exactly these pairs; hence every total has the bits
// of qc_wave_sum_to_lane63's.  (tools/ubench/wave_sum_merge.hip compares them bitwise on the device for NV = 1..16.)
//
// Schedule for a chunk of up to 16 values k = 0..15 (a longer array is cut into chunks of 16):
//   bits 0, 1  per value, as above: DPP has no mask finer than a bank (4 lanes), nothing can be merged yet.
//   bit 2      value 2i: row_half_mirror add to all banks; value 2i+1: the same add with bank_mask 0xa INTO the register
//              of 2i.  Banks 0, 2 now carry h of value 2i, banks 1, 3 h of value 2i+1.
//   bit 3      row_ror:8 pairs bank 0 with 2 and bank 1 with 3, i.e. the two half-rows of the SAME value (row_mirror
//              would pair bank 0 with bank 3: two different values).  The second pair's add goes with bank_mask 0xc into
//              the first pair's register: bank b of register 4i carries r of value 4i + b.
//   bit 4      v_permlane16_swap of registers 8i and 8i+4 exchanges the odd rows of the first with the even rows of
//              the second; one plain add then leaves p of values 8i..8i+3 in rows 0, 2 and of 8i+4..8i+7 in rows 1, 3.
//   bit 5      v_permlane32_swap of registers 0 and 8 plus one add: lanes 0..31 carry the totals of values 0..7, lanes
//              32..63 those of values 8..15.
//   A register without a partner is swapped with a dead one (a value register already folded away): the lanes that
//   receive the dead register's content are not home lanes.  row_bcast15/31 cannot serve here, they broadcast one
//   lane and with it one bank's value.
// Home lanes: value k of a merged chunk ends in the four lanes 4 j .. 4 j + 3, j = k % 16, of register v[16 (k / 16)], and
// its HOME lane is the first of them for even j and the last for odd j: lane 4 j + 3 (j & 1), that is lanes 0, 7, 8, 15
// of a row.  A chunk of one or two values (NV < 3, or the tail of a longer array) is cheaper unmerged
// and keeps lane 63 of its own register.  Both maps are the constexpr functions below; callers store from there.
// Why not any lane of the bank: where the summed value is a product, -ffp-contract=fast lets the compiler contract the
// multiply into the first step, s1[l] = fma(a[l], b[l], round(a b)[l^1]), and then s1[l] != s1[l^1]: the lanes of a
// quad hold two versions of the quad sum (even lanes one, odd lanes the other), and so on up the tree.  The arguments
// above still hold lane by lane with x[l^1] replaced by "what lane l^1 holds", and they give: after bit 2 lanes l and
// l^7 agree (h[l] = q[l] + q[l^7]); lane 63's total is built from r[15] = h[15] + h[0] of each row; row_ror:8 forms
// h[l] + h[l^8], which in lanes 0, 7, 8, 15 is h[0] + h[15] (h[7] = h[0], h[8] = h[15]) and elsewhere is not.  Bits 4 and
// 5 add lane-for-lane across rows.  So the home lanes, and only they, carry the bits of lane 63 of
// qc_wave_sum_to_lane63 for contracted inputs too.
// Cost in VALU instructions: 2 NV + NV + ceil(NV/2) + 2 ceil(NV/8) + 2 per chunk; 25 for NV = 6 (36 unmerged), 18 for
// NV = 4 (24), 48 for NV = 12 (72), plus an s_nop 1 in front of each swap whose operands the step before wrote.
__host__ __device__ constexpr int qc_ws_chunk_len(int NV, int k) { return NV - k / 16 * 16 < 16 ? NV - k / 16 * 16 : 16; }
__host__ __device__ constexpr bool qc_ws_merged(int NV, int k) { return qc_ws_chunk_len(NV, k) >= 3; }
__host__ __device__ constexpr int qc_wave_sum_home_lane(int NV, int k) {
  return qc_ws_merged(NV, k) ? 4 * (k % 16) + 3 * (k & 1) : 63;
}
// the inverse map within a merged chunk: is `lane` a home lane, and of which value of the chunk
__host__ __device__ constexpr bool qc_wave_sum_is_home(int lane) { return (lane & 3) == 3 * ((lane >> 2) & 1); }
__host__ __device__ constexpr int qc_wave_sum_home_index(int lane) { return lane >> 2; }
__host__ __device__ constexpr int qc_wave_sum_home_reg(int NV, int k) { return qc_ws_merged(NV, k) ? k / 16 * 16 : k; }

// The levels from bit 2 on are hand-written instructions (a bank-masked add into another value's register has no
// builtin form), and inside asm neither the assembler nor the compiler pads the hazards: a DPP or permlane-swap read of a
// register needs two wait states behind the VALU write of it (the s_nop 0 the compiler puts between two asm statements
// that share a register answers another hazard and is one state short).  The order of a chunk's instructions and the
// s_nop in front of those that would read too early are worked out at compile time by a small list scheduler.
enum : int { QC_WS_HM, QC_WS_HMM, QC_WS_ROR, QC_WS_RORM, QC_WS_SW16, QC_WS_SW32 };
struct QcWsOp {
  int kind, a, b, pad;   // a: register written (and folded); b: second register; pad: wait states in front
};
struct QcWsPlan {
  QcWsOp op[32];
  int n;
};
__host__ __device__ constexpr QcWsPlan qc_ws_plan(int n) {
  QcWsOp prog[32] = {};
  int np = 0;
  for (int a = 0; a < n; a += 2) {
    prog[np++] = {QC_WS_HM, a, a, 0};
    if (a + 1 < n) prog[np++] = {QC_WS_HMM, a, a + 1, 0};
  }
  for (int a = 0; a < n; a += 4) {
    prog[np++] = {QC_WS_ROR, a, a, 0};
    if (a + 2 < n) prog[np++] = {QC_WS_RORM, a, a + 2, 0};
  }
  // dead registers for the swaps without a partner: 1 (read last by the bit-2 step of register 0) and 2 (bit 3)
  for (int a = 0; a < n; a += 8) prog[np++] = {QC_WS_SW16, a, a + 4 < n ? a + 4 : 1, 0};
  prog[np++] = {QC_WS_SW32, 0, 8 < n ? 8 : (n <= 4 ? 2 : 1), 0};
  QcWsPlan P = {};
  int age[16] = {};
  for (int r = 0; r < 16; ++r) age[r] = 99;
  bool done[32] = {};
  int pad = 0;
  while (P.n < np) {
    int pick = -1;
    for (int i = 0; i < np && pick < 0; ++i) {
      if (done[i]) continue;
      const QcWsOp o = prog[i];
      const bool swap = o.kind == QC_WS_SW16 || o.kind == QC_WS_SW32;
      bool ok = true;
      // every earlier instruction that touches one of this one's registers has been issued
      for (int j = 0; j < i; ++j)
        if (!done[j] && (prog[j].a == o.a || prog[j].a == o.b || prog[j].b == o.a || prog[j].b == o.b)) ok = false;
      // the registers it reads across lanes were written two wait states ago
      if (age[o.b] < 2 || ((swap || o.a == o.b) && age[o.a] < 2)) ok = false;
      if (ok) pick = i;
    }
    if (pick < 0) {
      ++pad;
      for (int r = 0; r < 16; ++r) ++age[r];
      continue;
    }
    QcWsOp o = prog[pick];
    const bool swap = o.kind == QC_WS_SW16 || o.kind == QC_WS_SW32;
    o.pad = pad;
    pad = 0;
    done[pick] = true;
    P.op[P.n++] = o;
    for (int r = 0; r < 16; ++r) age[r] += swap ? 2 : 1;   // a swap comes with its add
    age[o.a] = 0;
    if (swap) age[o.b] = 1;
  }
  return P;
}

template <int NV, int C0, int I>
__device__ __forceinline__ void qc_ws_emit(float (&v)[NV]) {
  constexpr QcWsPlan P = qc_ws_plan(qc_ws_chunk_len(NV, C0));
  if constexpr (I < P.n) {
    constexpr QcWsOp o = P.op[I];
    static_assert(o.pad >= 0 && o.pad <= 2, "a hazard is two wait states");
    float& x = v[C0 + o.a];
    float& y = v[C0 + o.b];
#define QC_WS_ASM_(INS, ...)                                                   \
  do {                                                                         \
    if constexpr (o.pad == 0) asm volatile(INS : __VA_ARGS__);                 \
    else if constexpr (o.pad == 1) asm volatile("s_nop 0\n\t" INS : __VA_ARGS__); \
    else asm volatile("s_nop 1\n\t" INS : __VA_ARGS__);                        \
  } while (0)
    if constexpr (o.kind == QC_WS_HM)
      QC_WS_ASM_("v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf", "+v"(x));
    else if constexpr (o.kind == QC_WS_HMM)
      QC_WS_ASM_("v_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa", "+v"(x) : "v"(y));
    else if constexpr (o.kind == QC_WS_ROR)
      QC_WS_ASM_("v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf", "+v"(x));
    else if constexpr (o.kind == QC_WS_RORM)
      QC_WS_ASM_("v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xc", "+v"(x) : "v"(y));
    else if constexpr (o.kind == QC_WS_SW16)
      QC_WS_ASM_("v_permlane16_swap_b32 %0, %1\n\tv_add_f32 %0, %0, %1", "+v"(x), "+v"(y));
    else
      QC_WS_ASM_("v_permlane32_swap_b32 %0, %1\n\tv_add_f32 %0, %0, %1", "+v"(x), "+v"(y));
#undef QC_WS_ASM_
    qc_ws_emit<NV, C0, I + 1>(v);
  }
}
template <int NV, int C0>
__device__ __forceinline__ void qc_ws_chunks(float (&v)[NV]) {
  if constexpr (C0 < NV) {
    if constexpr (qc_ws_merged(NV, C0)) {
      qc_ws_emit<NV, C0, 0>(v);
    } else {
      constexpr int R = NV - C0;
      float t[R];
#pragma unroll
      for (int k = 0; k < R; ++k) t[k] = v[C0 + k];
      qc_wave_sum_multi_to_lane63<R>(t);
#pragma unroll
      for (int k = 0; k < R; ++k) v[C0 + k] = t[k];
    }
    qc_ws_chunks<NV, C0 + 16>(v);
  }
}
// On return value k's total is in lane qc_wave_sum_home_lane(NV, k) of v[qc_wave_sum_home_reg(NV, k)]; every other
// lane and register of v holds no defined value.
template <int NV>
__device__ __forceinline__ void qc_wave_sum_merged(float (&v)[NV]) {
  if constexpr (NV < 3) {
    qc_wave_sum_multi_to_lane63<NV>(v);
  } else {
    constexpr int NM = NV - (qc_ws_merged(NV, NV - 1) ? 0 : NV % 16);   // values in merged chunks
#pragma unroll
    for (int k = 0; k < NM; ++k)
      v[k] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[k]), 0xB1, 0xF, 0xF, true));
#pragma unroll
    for (int k = 0; k < NM; ++k)
      v[k] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[k]), 0x4E, 0xF, 0xF, true));
    // every value's quad sum is complete, and two wait states old, before the first hand-written DPP read
#pragma unroll
    for (int k = 0; k < NM; ++k) asm volatile("" : "+v"(v[k]));
    asm volatile("s_nop 1");
    qc_ws_chunks<NV, 0>(v);
  }
}

// Sum over the wave, result broadcast to every lane (uniform value).
__device__ __forceinline__ float qc_wave_sum(float v) {
  v = qc_wave_sum_to_lane63(v);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
