// Variational-circuit kernels, "reg" family: 2 <= n <= 5 qubits, one lane = one statevector
// held entirely in VGPRs (qc_gates.h).  Replaces the PennyLane default.qubit simulation behind
// DVQuantumLayer.forward (reference nn/DVQuantumLayer.py:151-154,176-214) and the torch
// double-backward through it that nn/pde.py:59-70 + loss.backward() trigger.
//
// Four kernels per qubit count:
//   value_fwd : angles[n][B]            -> <Z_w>[n][B]                       (1 channel)
//   value_bwd : angles, cot[n][B]       -> d_angles[n][B], d_theta partial rows
//   jets_fwd  : angle jets[6][n][B]     -> <Z_w> jets[6][n][B]               (6 channels)
//   jets_bwd  : angle jets, cot jets    -> d(angle jets)[6][n][B], d_theta partial rows
// Channels: 0 value, 1 d/dt, 2 d/dx, 3 d/dy, 4 d2/dx2, 5 d2/dy2 (forward-mode derivatives of the
// circuit output w.r.t. the collocation coordinates; the gates are linear so every channel runs
// the same gate program on its own initial vector).  In the jet kernels a block is 6 waves x 64
// points: wave c carries channel c of the block's 64 points, channels meet through LDS only
// where the bilinear <Z> forms and their cotangents couple them.
//
// Batch-minor ([feature][B]) layouts make every global access 64 consecutive floats per wave.
#pragma once
#include "qc_gates.h"
#include "qc_internal.h"

#include <stdlib.h>

#include <utility>

namespace {

// A run-time flag of the stand-alone kernels that a merged step kernel knows when it is compiled: AB = 0 / 1 fixes it
// (no register, no branch, no select where it is read), AB = -1 forwards the run-time argument.
template <int AB>
__device__ __forceinline__ bool qc_flag(int rt) {
  if constexpr (AB < 0) return rt != 0;
  else return AB != 0;
}

// Hides a pointer's provenance from the optimiser: loads through the result are not merged with
// earlier loads, so values recomputed from them do not stay live in registers in between.
template <class T>
__device__ __forceinline__ const T* qc_launder(const T* p) {
  asm volatile("" : "+s"(p));
  return p;
}
// The same for wave-uniform read-only tables (trig, phase tables, U4 blocks), through the constant address space:
// always scalar loads, requested where the result is used - never hoisted out of a loop around the caller and held
// (or spilled to VGPR lanes) across it.
template <class T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* qc_const(const T* p) {
  return (const __attribute__((address_space(4))) T*)qc_launder(p);
}
// ... and not before the state the table is applied to exists, every amplitude of it: the request cannot move up past
// the gate in front of it either (one anchored amplitude would only pull that amplitude's arithmetic up with it)
template <class T, int N>
__device__ __forceinline__ const __attribute__((address_space(4))) T* qc_const_at(const T* p, const SV<N>& v) {
#define QC_A4_(o) "v"(v.a[o]), "v"(v.a[o + 1]), "v"(v.a[o + 2]), "v"(v.a[o + 3])
  if constexpr (N == 2) asm volatile("" : "+s"(p) : QC_A4_(0));
  if constexpr (N == 3) asm volatile("" : "+s"(p) : QC_A4_(0), QC_A4_(4));
  if constexpr (N >= 4) asm volatile("" : "+s"(p) : QC_A4_(0), QC_A4_(4), QC_A4_(8), QC_A4_(12));
  if constexpr (N == 5) asm volatile("" : "+s"(p) : QC_A4_(16), QC_A4_(20), QC_A4_(24), QC_A4_(28));
#undef QC_A4_
  static_assert(N >= 2 && N <= 5, "register family");
  return (const __attribute__((address_space(4))) T*)p;
}
// a wave-uniform / per-lane integer as an opaque value: what is derived from it is recomputed at its use instead of
// being hoisted out of a loop and held
__device__ __forceinline__ int64_t qc_opaque_s(int64_t v) {
  asm volatile("" : "+s"(v));
  return v;
}
__device__ __forceinline__ int qc_opaque_v(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ------------------------------------------------------------------ program policies
// DynProg<N>: the gate program is run-time data (scalar switch per gate, any ansatz).
template <int NQ>
struct DynProg {
  static constexpr int N = NQ;
  static constexpr bool lead_rx = true;   // (run-time data: either form of the embedding may be asked for)
  __device__ static __forceinline__ int lead_slot(const QcGate* __restrict__ prog, int w) { return prog[w].slot; }
  template <int AB = -1, bool PIN = false>
  __device__ static __forceinline__ void fwd(SV<NQ> (&v)[1], const QcGate* __restrict__ prog,
                                             const QcTrig* __restrict__ trig, const float* __restrict__ umat,
                                             int n_gates, int absorb) {
    for (int g = qc_flag<AB>(absorb) ? NQ : 0; g < n_gates; ++g) {
      const QcGate gt = prog[g];
      const QcTrig tr = trig[g];
      qc_apply_gate<NQ, 1, false>(v, gt, tr.c, tr.s, umat);
    }
  }
  // Reverse sweep for one (chi, lam) pair: accumulates Im<lam|G|chi> per parameter slot into
  // acc_wave[slot] (LDS, one row per wave), then un-applies the gate on both.
  template <int AB = -1>
  __device__ static __forceinline__ void bwd(SV<NQ> (&cl)[2], const QcGate* __restrict__ prog,
                                             const QcTrig* __restrict__ trig, const float* __restrict__ umat,
                                             int n_gates, float* __restrict__ acc_wave, int lane, int absorb) {
    const int g_first = qc_flag<AB>(absorb) ? NQ : 0;
    for (int g = n_gates - 1; g >= g_first; --g) {
      const QcGate gt = prog[g];
      const QcTrig tr = trig[g];
      if (gt.op != QC_U4 && gt.slot >= 0) {
        const float gr = qc_wave_sum6_to_lane63(qc_gate_grad<NQ>(cl[1], cl[0], gt));
        if (lane == 63) acc_wave[gt.slot] += gr;
      }
      qc_apply_gate<NQ, 2, true>(cl, gt, tr.c, tr.s, umat);
    }
  }
};

// StatProg<SP>: the gate list is a compile-time constant (SP::g[], generated from circuits.py by
// gen_static.py), so the whole circuit is straight-line code: no dispatch, no register shuffling
// at control-flow merges, trig table entries at constant offsets (scalar loads).
struct SGate {
  int op, ba, bb, slot;
};

template <int NQ, int K, bool ADJ, int OP, int BA, int BB, int SLOT>
__device__ __forceinline__ void qc_static_gate(SV<NQ> (&v)[K], const float c, const float s_in) {
  const float s = ADJ ? -s_in : s_in;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    if constexpr (OP == QC_RX) g_rx<NQ, BA>(v[q], c, s);
    else if constexpr (OP == QC_RY) g_ry<NQ, BA>(v[q], c, s);
    else if constexpr (OP == QC_RZ) g_rz<NQ, BA>(v[q], c, s);
    else if constexpr (OP == QC_H) g_h<NQ, BA>(v[q]);
    else if constexpr (OP == QC_CNOT) g_cnot<NQ, BA, BB>(v[q]);
    else if constexpr (OP == QC_CRX) g_crx<NQ, BA, BB>(v[q], c, s);
    else if constexpr (OP == QC_CRZ) g_crz<NQ, BA, BB>(v[q], c, s);   // (QC_U4: StatProg::gate)
  }
}

template <int NQ, int OP, int BA, int BB>
__device__ __forceinline__ float qc_static_grad(const SV<NQ>& lam, const SV<NQ>& chi) {
  if constexpr (OP == QC_RX) return ip_x<NQ, BA>(lam, chi);
  else if constexpr (OP == QC_RY) return ip_y<NQ, BA>(lam, chi);
  else if constexpr (OP == QC_RZ) return ip_z<NQ, BA>(lam, chi);
  else if constexpr (OP == QC_CRX) return ip_cx<NQ, BA, BB>(lam, chi);
  else if constexpr (OP == QC_CRZ) return ip_cz<NQ, BA, BB>(lam, chi);
  else return 0.f;
}

template <class SP>
struct StatProg {
  static constexpr int N = SP::N;
  // The (cos, sin) pairs of every parametric gate are fetched before the first gate (they are wave-uniform:
  // scalar loads into SGPRs, batched by the compiler), so no gate starts by waiting on a scalar load.
  struct Trig {
    float c[SP::G], s[SP::G];
  };
  using CMat = const __attribute__((address_space(4))) float*;
  // the first N gates are RX(theta_w) on wire w with N distinct slots: the layer the embedding can absorb (qc_api.hip)
  static constexpr bool lead_rx_layer() {
    if (SP::G < N) return false;
    for (int w = 0; w < N; ++w) {
      if (SP::g[w].op != QC_RX || SP::g[w].ba != N - 1 - w || SP::g[w].slot < 0) return false;
      for (int u = 0; u < w; ++u)
        if (SP::g[u].slot == SP::g[w].slot) return false;
    }
    return true;
  }
  static constexpr bool lead_rx = lead_rx_layer();
  __device__ static __forceinline__ int lead_slot(const QcGate* __restrict__, int w) { return SP::g[w < SP::G ? w : 0].slot; }
  // AB = 1: the absorbed layer's gates are not run, so their entries are not fetched either
  template <int I, int AB, class TP>
  __device__ static __forceinline__ void load_one(Trig& t, TP trig) {
    constexpr SGate g = SP::g[I];
    t.c[I] = 1.f;
    t.s[I] = 0.f;
    if constexpr (g.op != QC_U4 && g.slot >= 0 && !fused(I) && !(AB == 1 && I < N)) {
      t.c[I] = trig[I].c;
      t.s[I] = trig[I].s;
    }
  }
  template <int AB, class TP, int... Is>
  __device__ static __forceinline__ void load_all(Trig& t, TP trig, std::integer_sequence<int, Is...>) {
    (load_one<Is, AB>(t, trig), ...);
    __builtin_amdgcn_sched_barrier(0);
  }
  // ---- runs of >= 2 consecutive diagonal gates (RZ / CRZ) are ONE table multiply (tables: qc_fill_diag_tables)
  static constexpr bool is_diag(int i) { return i >= 0 && i < SP::G && (SP::g[i].op == QC_RZ || SP::g[i].op == QC_CRZ); }
  static constexpr int run_begin(int i) { while (is_diag(i - 1)) --i; return i; }
  static constexpr int run_end(int i) { while (is_diag(i)) ++i; return i; }          // one past the last gate
  static constexpr bool fused(int i) { return is_diag(i) && run_end(i) - run_begin(i) >= 2; }
  static constexpr int run_ordinal(int i) {
    int r = 0;
    for (int g = 0; g < run_begin(i);) {
      if (!is_diag(g)) { ++g; continue; }
      const int e = run_end(g);
      if (e - g >= 2) ++r;
      g = e;
    }
    return r;
  }
  static_assert(run_ordinal(SP::G) <= QC_MAX_DIAG_RUNS, "more fused diagonal runs than the host records (qc_find_diag_runs)");
  // PIN: the table is requested here, inside the run that consumes it, and not before the state it is applied to
  // exists (2^N SGPR pairs: not held across the neighbouring gates).  The forward-only kernels, with room for every
  // table at once, leave the requests to the compiler (!PIN): it issues them in front of the sweep.
  template <int I, bool ADJ, int K, bool PIN = true>
  __device__ static __forceinline__ void apply_table(SV<N> (&v)[K], const QcTrig* __restrict__ trig) {
    constexpr int off = SP::G + run_ordinal(I) * (1 << N);
    auto run = [&](auto tab) {
#pragma unroll
      for (int k = 0; k < (1 << N); ++k) {
        const float dr = tab[k].c, di = ADJ ? -tab[k].s : tab[k].s;   // adjacent in the table: one SGPR pair
#pragma unroll
        for (int q = 0; q < K; ++q) v[q].a[k] = qc_cmul(dr, di, v[q].a[k]);
      }
    };
    if constexpr (PIN) run(qc_const_at(trig, v[0]) + off);
    else run(trig + off);
  }
  // gradient terms of the gates H, H+1, ..., E-1 of one run from t[k] = Im(conj(lam_k) chi_k) (invariant under
  // the other diagonal gates of the run): signed by the target bit, masked by the control bit
  // (the run's terms, one per gate, come from the same t and are reduced over the wave together: the six steps of
  // every value in their own order, interleaved, the totals in lane 63)
  template <int H, int E>
  __device__ static __forceinline__ void run_terms(const QcPk<(1 << N)>& t, float (&term)[E - run_begin(E - 1)]) {
    if constexpr (H < E) {
      constexpr SGate g = SP::g[H];
      constexpr bool ctl = g.op == QC_CRZ;
      constexpr int tb = ctl ? g.bb : g.ba;
      constexpr int cb = ctl ? g.ba : -1;
      qf2 a2 = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < (1 << (N - 1)); ++j) {
        if (cb >= 1 && !((j >> (cb >= 1 ? cb - 1 : 0)) & 1)) continue;
        if (tb >= 1 && ((j >> (tb >= 1 ? tb - 1 : 0)) & 1)) a2 -= t.p[j];
        else a2 += t.p[j];
      }
      // target on bit 0: the halves carry opposite signs; control on bit 0: only the upper halves count
      term[H - run_begin(H)] = tb == 0 ? a2.x - a2.y : (cb == 0 ? a2.y : a2.x + a2.y);
      run_terms<H + 1, E>(t, term);
    }
  }
  template <int H, int E, int... Is>
  __device__ static __forceinline__ void run_grads(const QcPk<(1 << N)>& t, float (&gacc)[SP::P > 0 ? SP::P : 1],
                                                   std::integer_sequence<int, Is...>) {
    float term[E - H];
    run_terms<H, E>(t, term);
    qc_wave_sum_multi_to_lane63<E - H>(term);
    (run_add<H + Is>(gacc, term[Is]), ...);   // in gate order, as the sums were added one by one
  }
  template <int I>
  __device__ static __forceinline__ void run_add(float (&gacc)[SP::P > 0 ? SP::P : 1], const float tot) {
    if constexpr (SP::g[I].slot >= 0) gacc[SP::g[I].slot] += tot;
  }
  // one non-diagonal gate; PIN: the 32 scalars of a U4 block are requested here, inside the gate that consumes them
  template <int I, int K, bool ADJ, bool PIN = true>
  __device__ static __forceinline__ void gate(SV<N> (&v)[K], const Trig& t, const float* __restrict__ umat) {
    constexpr SGate g = SP::g[I];
    if constexpr (g.op == QC_U4) {
      constexpr int off = (g.slot * 2 + (ADJ ? 1 : 0)) * 32;
      if constexpr (PIN) {
        const CMat u = qc_const_at(umat, v[0]) + off;
#pragma unroll
        for (int q = 0; q < K; ++q) g_u4<N, g.ba, g.bb>(v[q], u);
      } else {
#pragma unroll
        for (int q = 0; q < K; ++q) g_u4<N, g.ba, g.bb>(v[q], umat + off);
      }
    } else {
      qc_static_gate<N, K, ADJ, g.op, g.ba, g.bb, g.slot>(v, t.c[I], t.s[I]);
    }
  }
  template <int I, int AB, bool PIN>
  __device__ static __forceinline__ void fwd_one(SV<N> (&v)[1], const Trig& t, const float* __restrict__ umat,
                                                 int absorb, const QcTrig* __restrict__ trig) {
    if constexpr (I < N) {
      if (qc_flag<AB>(absorb)) return;   // leading RX layer folded into the embedding angles
    }
    if constexpr (fused(I)) {
      if constexpr (I == run_begin(I)) {
        apply_table<I, false, 1, PIN>(v, trig);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      gate<I, 1, false, PIN>(v, t, umat);
      __builtin_amdgcn_sched_barrier(0);   // keep the scheduler from interleaving whole gates (register pressure)
    }
  }
  template <int AB, bool PIN, int... Is>
  __device__ static __forceinline__ void fwd_all(SV<N> (&v)[1], const Trig& t, const float* __restrict__ umat,
                                                 int absorb, const QcTrig* __restrict__ trig,
                                                 std::integer_sequence<int, Is...>) {
    (fwd_one<Is, AB, PIN>(v, t, umat, absorb, trig), ...);
  }
  template <int AB = -1, bool PIN = false>
  __device__ static __forceinline__ void fwd(SV<N> (&v)[1], const QcGate* __restrict__, const QcTrig* __restrict__ trig,
                                             const float* __restrict__ umat, int, int absorb) {
    Trig t;
    if constexpr (PIN) load_all<AB>(t, qc_const(trig), std::make_integer_sequence<int, SP::G>{});
    else load_all<AB>(t, trig, std::make_integer_sequence<int, SP::G>{});
    fwd_all<AB, PIN>(v, t, umat, absorb, trig, std::make_integer_sequence<int, SP::G>{});
  }
  // Reverse sweep.  Parameter slots are compile-time constants here, so the wave totals of the
  // gradient terms stay in registers (gacc[slot], valid in lane 63) and reach LDS once, after the
  // sweep, instead of one LDS read-modify-write round trip per gate.
  template <int J, int AB>
  __device__ static __forceinline__ void bwd_one(SV<N> (&cl)[2], const Trig& t, const float* __restrict__ umat,
                                                 float (&gacc)[SP::P > 0 ? SP::P : 1], int absorb,
                                                 const QcTrig* __restrict__ trig) {
    constexpr int I = SP::G - 1 - J;
    constexpr SGate g = SP::g[I];
    if constexpr (I < N) {
      if (qc_flag<AB>(absorb)) return;
    }
    if constexpr (fused(I)) {
      if constexpr (I == run_end(I) - 1) {   // first gate of the run met by the reverse sweep
        QcPk<(1 << N)> tk;   // Im(conj(lam_k) chi_k), two k per pair for the signed sums
#pragma unroll
        for (int k = 0; k < (1 << N); ++k) {
          const qf2 m = cl[1].a[k] * qc_swp(cl[0].a[k]);
          tk[k] = m.x - m.y;
        }
        run_grads<run_begin(I), run_end(I)>(tk, gacc, std::make_integer_sequence<int, run_end(I) - run_begin(I)>{});
        apply_table<I, true, 2>(cl, trig);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      if constexpr (g.op != QC_U4 && g.slot >= 0)
        gacc[g.slot] += qc_wave_sum6_to_lane63(qc_static_grad<N, g.op, g.ba, g.bb>(cl[1], cl[0]));
      gate<I, 2, true>(cl, t, umat);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  template <int AB, int... Js>
  __device__ static __forceinline__ void bwd_all(SV<N> (&cl)[2], const Trig& t, const float* __restrict__ umat,
                                                 float (&gacc)[SP::P > 0 ? SP::P : 1], int absorb,
                                                 const QcTrig* __restrict__ trig, std::integer_sequence<int, Js...>) {
    (bwd_one<Js, AB>(cl, t, umat, gacc, absorb, trig), ...);
  }
  template <int AB = -1>
  __device__ static __forceinline__ void bwd(SV<N> (&cl)[2], const QcGate* __restrict__, const QcTrig* __restrict__ trig,
                                             const float* __restrict__ umat, int, float* __restrict__ acc_wave,
                                             int lane, int absorb) {
    float gacc[SP::P > 0 ? SP::P : 1];
#pragma unroll
    for (int k = 0; k < (SP::P > 0 ? SP::P : 1); ++k) gacc[k] = 0.f;
    Trig t;
    load_all<AB>(t, qc_const(trig), std::make_integer_sequence<int, SP::G>{});
    bwd_all<AB>(cl, t, umat, gacc, absorb, trig, std::make_integer_sequence<int, SP::G>{});
    const int k0 = qc_opaque_v(0);   // (one address, constant offsets; the lane test rebuilt here, not held as a mask)
    const bool last = qc_opaque_v(lane) == 63;
#pragma unroll
    for (int k = 0; k < SP::P; ++k)
      if (last) acc_wave[k0 + k] += gacc[k];   // lane 63 holds the wave totals
  }
};

// half-angle (cos, sin) of wire w's embedding rotation for one point
template <int AB = -1>
__device__ __forceinline__ void qc_wire_sincos(float& c, float& s, const float* __restrict__ a, int64_t B, int64_t p, int w,
                                               const QcTrig* __restrict__ trig, int absorb) {
  // absorb: gate w is RX(theta_w) on wire w, applied right after RX(a_w): one rotation by a_w + theta_w
  const float h = 0.5f * (a[(int64_t)w * B + p] + (qc_flag<AB>(absorb) ? trig[w].th : 0.f));
  sincosf(h, &s, &c);
}
// `cs` != nullptr: the block already holds them in LDS as [cos | sin][N][64] (each of the jet kernels' six waves
// needs the same 2N values for its 64 points: waves 0..N-1 compute one wire each instead of all six computing all)
template <int N, int AB = -1>
__device__ __forceinline__ void load_sincos(float (&ca)[N], float (&sa)[N], const float* __restrict__ a,
                                            int64_t B, int64_t p, const QcTrig* __restrict__ trig, int absorb,
                                            const float* cs = nullptr) {
#pragma unroll
  for (int w = 0; w < N; ++w) {
    if (cs != nullptr) {
      ca[w] = cs[w * 64 + (threadIdx.x & 63)];
      sa[w] = cs[(N + w) * 64 + (threadIdx.x & 63)];
    } else {
      qc_wire_sincos<AB>(ca[w], sa[w], a, B, p, w, trig, absorb);
    }
  }
}

// the block's [cos | sin][N][64] table in LDS, unconditionally (no second, computing path in the caller's code)
template <int N>
__device__ __forceinline__ void load_sincos_lds(float (&ca)[N], float (&sa)[N], const float* cs) {
#pragma unroll
  for (int w = 0; w < N; ++w) {
    ca[w] = cs[w * 64 + (threadIdx.x & 63)];
    sa[w] = cs[(N + w) * 64 + (threadIdx.x & 63)];
  }
}

// Embedding series of channel `ch`'s direction for this lane's point: P0 = phi, P1 = d phi,
// P2 = d2 phi (only as far as the channel needs).
template <int N, int AB = -1>
__device__ __forceinline__ void channel_series(QcPk<(1 << N)>& P0, QcPk<(1 << N)>& P1, QcPk<(1 << N)>& P2,
                                               int ch, const float* __restrict__ ajets, int64_t B, int64_t pc,
                                               const QcTrig* __restrict__ trig, int absorb, const float* cs = nullptr) {
  float ca[N], sa[N], da[N], dda[N];
  load_sincos<N, AB>(ca, sa, ajets, B, pc, trig, absorb, cs);
  const int dirch = ch == 0 ? 0 : (ch <= 3 ? ch : ch - 2);  // channel holding the first derivative
#pragma unroll
  for (int w = 0; w < N; ++w) {
    da[w] = ch >= 1 ? ajets[((int64_t)dirch * N + w) * B + pc] : 0.f;
    dda[w] = ch >= 4 ? ajets[((int64_t)ch * N + w) * B + pc] : 0.f;
  }
  if (ch == 0) qc_embed_series<N, 0>(P0, P1, P2, ca, sa, da, dda);
  else if (ch <= 3) qc_embed_series<N, 1>(P0, P1, P2, ca, sa, da, dda);
  else qc_embed_series<N, 2>(P0, P1, P2, ca, sa, da, dda);
}

// Initial vector of channel `ch`.  amp != 0: amplitude encoding — `ajets` then holds the jets of the
// (normalised, zero-padded) initial amplitudes themselves (qc_amp.hip): amplitude k = feature k, real.
template <int N, int AB = -1>
__device__ __forceinline__ void build_channel(SV<N>& v, int ch, const float* __restrict__ ajets, int64_t B,
                                              int64_t pc, int amp, const QcTrig* __restrict__ trig, int absorb,
                                              const float* cs = nullptr) {
  if (amp) {
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) {
      v.a[k].x = k < N ? ajets[((int64_t)ch * N + k) * B + pc] : 0.f;
      v.a[k].y = 0.f;
    }
    return;
  }
  QcPk<(1 << N)> P0, P1, P2;
  channel_series<N, AB>(P0, P1, P2, ch, ajets, B, pc, trig, absorb, cs);
  if (ch == 0) qc_phase_load<N>(v, P0);
  else if (ch <= 3) qc_phase_load<N>(v, P1);
  else qc_phase_load<N>(v, P2);
}

// ================================================================== value channel only
template <class PG, int WPB>
__device__ __forceinline__ void k_value_fwd_body(const int64_t bid, const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                   const float* __restrict__ umat, int n_gates,
                                                   const float* __restrict__ angles, float* __restrict__ expval,
                                                   int64_t B, int amp) {
  constexpr int N = PG::N;
  const int64_t p = (int64_t)bid * (64 * WPB) + threadIdx.x;
  const int64_t pc = p < B ? p : B - 1;
  SV<N> v[1];
  build_channel<N>(v[0], 0, angles, B, pc, amp & 1, trig, amp >> 1);
  PG::fwd(v, prog, trig, umat, n_gates, amp >> 1);
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

template <class PG>
__global__ void __launch_bounds__(256) k_value_fwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                   const float* __restrict__ umat, int n_gates,
                                                   const float* __restrict__ angles, float* __restrict__ expval,
                                                   int64_t B, int amp) {
  k_value_fwd_body<PG, 4>(blockIdx.x, prog, trig, umat, n_gates, angles, expval, B, amp);
}

// AB >= 0 (the merged step's 3-wave stage): angle encoding, the absorb flag = AB at compile time, `amp` not read
template <class PG, int WPB, int AB = -1>
__device__ __forceinline__ void k_value_bwd_body(const int64_t bid, const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                   const float* __restrict__ umat, int n_gates, int n_params,
                                                   const float* __restrict__ angles, const float* __restrict__ cot,
                                                   float* __restrict__ d_angles, float* __restrict__ part,
                                                   int64_t part_stride, int64_t row0, int64_t B, int amp) {
  constexpr int N = PG::N;
  const bool ampl = AB < 0 && (amp & 1);
  const int absorb = AB < 0 ? amp >> 1 : AB;
  extern __shared__ float smem[];  // [WPB waves][n_params]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < WPB * n_params; i += 64 * WPB) smem[i] = 0.f;
  __syncthreads();

  const int64_t p = (int64_t)bid * (64 * WPB) + threadIdx.x;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  SV<N> cl[2];  // [0] = chi, [1] = lambda
  {
    SV<N> v[1];
    build_channel<N, AB>(v[0], 0, angles, B, pc, ampl, trig, absorb);
    PG::template fwd<AB, true>(v, prog, trig, umat, n_gates, absorb);   // (pinned requests: the adjoint kernels have no room)
    cl[0] = v[0];
  }
  float qb[N];
#pragma unroll
  for (int w = 0; w < N; ++w) qb[w] = live ? cot[(int64_t)w * B + pc] : 0.f;
  {
    QcPk<(1 << N)> d;
    qc_sign_sums<N>(d, qb);
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_dup(d[k]) * cl[0].a[k];
  }
  PG::template bwd<AB>(cl, prog, trig, umat, n_gates, smem + wave * n_params, lane, absorb);
  float T[N];
  if (ampl) {   // d L / d(initial amplitude k) = 2 Re Lambda_k  (the initial amplitudes are real)
#pragma unroll
    for (int w = 0; w < N; ++w) T[w] = 2.f * cl[1].a[w].x;
  } else {
    QcPk<(1 << N)> Q0, Q1, Q2;
    channel_series<N, AB>(Q0, Q1, Q2, 0, qc_launder(angles), B, pc, trig, absorb);
    qc_embed_ip<N>(T, cl[1], Q0);
  }
  if (live) {
#pragma unroll
    for (int w = 0; w < N; ++w) d_angles[(int64_t)w * B + p] = T[w];
  }
  if (qc_flag<AB>(absorb)) {   // folded RX layer: d L / d theta_w = sum over points of d L / d angle_w
#pragma unroll
    for (int w = 0; w < N; ++w) {
      const float tot = qc_wave_sum6_to_lane63(live ? T[w] : 0.f);
      if (lane == 63) smem[wave * n_params + (AB < 0 ? prog[w].slot : PG::lead_slot(prog, w))] += tot;
    }
  }
  __syncthreads();
  // one partial row per wave = per 64-point tile (same tiling as the MLP kernels)
  const int64_t tile = (int64_t)bid * WPB + wave;
  if (tile * 64 < B)
    for (int i = lane; i < n_params; i += 64) part[(row0 + tile) * part_stride + i] = smem[wave * n_params + i];
}

template <class PG>
__global__ void __launch_bounds__(256) k_value_bwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                   const float* __restrict__ umat, int n_gates, int n_params,
                                                   const float* __restrict__ angles, const float* __restrict__ cot,
                                                   float* __restrict__ d_angles, float* __restrict__ part,
                                                   int64_t part_stride, int64_t row0, int64_t B, int amp) {
  k_value_bwd_body<PG, 4>(blockIdx.x, prog, trig, umat, n_gates, n_params, angles, cot, d_angles, part, part_stride, row0, B, amp);
}

// Final-state store handed from k_jets_fwd to k_jets_bwd: tile-major, so the 6 x A2 x 64 floats one
// block touches are one contiguous 6*A2*256-byte region (DRAM-page friendly), not A2 streams B apart.
// Units are amplitudes = (re, im) register pairs: 8 bytes per lane, one global_load/store_dwordx2 = 512 contiguous
// bytes per wave.
template <int A2>
__device__ __forceinline__ int64_t qc_chi_pair(int ch, int k, int64_t p) {
  return ((((p >> 6) * 6 + ch) * (A2 / 2) + k) << 6) | (p & 63);
}
template <int N>
__device__ __forceinline__ void qc_chi_write(float* __restrict__ chi_store, int ch, int64_t p, const SV<N>& v) {
  qf2* cs = reinterpret_cast<qf2*>(chi_store);
#pragma unroll
  for (int k = 0; k < (1 << N); ++k) cs[qc_chi_pair<(2 << N)>(ch, k, p)] = v.a[k];
}
template <int N>
__device__ __forceinline__ void qc_chi_read(SV<N>& v, const float* __restrict__ chi_store, int ch, int64_t p) {
  const qf2* cs = reinterpret_cast<const qf2*>(chi_store);
#pragma unroll
  for (int k = 0; k < (1 << N); ++k) v.a[k] = cs[qc_chi_pair<(2 << N)>(ch, k, p)];
}

// ================================================================== six derivative channels
template <class PG>
__device__ __forceinline__ void k_jets_fwd_body(const int64_t bid, const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                  const float* __restrict__ umat, int n_gates,
                                                  const float* __restrict__ ajets, float* __restrict__ qjets,
                                                  int64_t B, float* __restrict__ chi_store, int amp) {
  constexpr int N = PG::N;
  constexpr int A2 = 2 << N;                 // floats per statevector
  __shared__ float s_chi0[A2 * 64];          // [amp*2+{re,im}][lane]
  __shared__ float s_sq[2 * N * 64];         // 2<chi_k|Z_w|chi_k> for k = x, y
  const int lane = threadIdx.x & 63;
  const int ch = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave index = channel (scalar)
  const int64_t p = (int64_t)bid * 64 + lane;
  const int64_t pc = p < B ? p : B - 1;

  __shared__ float s_cs[2 * N * 64];         // half-angle cos | sin of the block's 64 points, one wire per wave
  if (!(amp & 1)) {
    if (ch < N) qc_wire_sincos(s_cs[ch * 64 + lane], s_cs[(N + ch) * 64 + lane], ajets, B, pc, ch, trig, amp >> 1);
    __syncthreads();
  }
  SV<N> v[1];
  build_channel<N>(v[0], ch, ajets, B, pc, amp & 1, trig, amp >> 1, s_cs);
  PG::fwd(v, prog, trig, umat, n_gates, amp >> 1);
  if (chi_store != nullptr && p < B) qc_chi_write<N>(chi_store, ch, p, v[0]);   // final states for the adjoint kernel

  QcPk<(1 << N)> t;
  float q[N];
  qf2* s_x0 = reinterpret_cast<qf2*>(s_chi0);   // [amplitude][lane]
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

template <class PG>
__global__ void __launch_bounds__(384) k_jets_fwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                  const float* __restrict__ umat, int n_gates,
                                                  const float* __restrict__ ajets, float* __restrict__ qjets,
                                                  int64_t B, float* __restrict__ chi_store, int amp) {
  k_jets_fwd_body<PG>(blockIdx.x, prog, trig, umat, n_gates, ajets, qjets, B, chi_store, amp);
}

#ifndef QC_JB_WAVES
#define QC_JB_WAVES 3
#endif
// LOAD: the final states come from chi_store (written by k_jets_fwd in the same step) instead of being
// recomputed from the angle jets: 12 instead of 18 circuit-equivalents per point.
template <class PG, bool LOAD>
__device__ __forceinline__ void k_jets_bwd_body(const int64_t bid, const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                  const float* __restrict__ umat, int n_gates, int n_params,
                                                  const float* __restrict__ ajets, const float* __restrict__ qbar,
                                                  float* __restrict__ abar, float* __restrict__ part,
                                                  int64_t part_stride, int64_t row0, int64_t B,
                                                  const float* __restrict__ chi_store, int amp) {
  constexpr int N = PG::N;
  constexpr int A2 = 2 << N;
  extern __shared__ float smem[];
  constexpr int XCH = LOAD ? 6 * 3 * N * 64 : 6 * A2 * 64;   // exchange region (floats)
  float* s_chi = smem;                       // !LOAD: [6][A2][64]; always reused as [6 waves][3][N][64] at the end
  float* s_acc = smem + XCH;                 // [6 waves][n_params]
  const int lane = threadIdx.x & 63;
  const int ch = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* s_cs = s_acc + 6 * n_params;        // [cos | sin][N][64] of the embedding half-angles, for the tail
  for (int i = threadIdx.x; i < 6 * n_params; i += 384) s_acc[i] = 0.f;
  const int64_t p = (int64_t)bid * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  if (!(amp & 1) && ch < N)
    qc_wire_sincos(s_cs[ch * 64 + lane], s_cs[(N + ch) * 64 + lane], ajets, B, pc, ch, trig, amp >> 1);
  if constexpr (LOAD) __syncthreads();   // (the !LOAD path has its barrier after the state exchange)


  SV<N> cl[2];
  if constexpr (LOAD) {
    qc_chi_read<N>(cl[0], chi_store, ch, pc);
  } else {
    SV<N> v[1];
    build_channel<N>(v[0], ch, ajets, B, pc, amp & 1, trig, amp >> 1);
    PG::template fwd<-1, true>(v, prog, trig, umat, n_gates, amp >> 1);
    cl[0] = v[0];
  }
  // The other channels' final states: through LDS when this launch computed them, straight from the
  // forward kernel's store (L2-resident) when LOAD -- then no exchange buffer and no barrier is needed
  // before the sweep, and the block's LDS shrinks to the small tail buffers.
  if constexpr (!LOAD) {
    qf2* mine = reinterpret_cast<qf2*>(s_chi) + ch * (A2 / 2) * 64;
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) mine[k * 64 + lane] = cl[0].a[k];
    __syncthreads();
  }
  // amplitude k of channel c's final state
  auto other = [&](int c, int k) -> qf2 {
    return LOAD ? reinterpret_cast<const qf2*>(chi_store)[qc_chi_pair<A2>(c, k, pc)]
                : reinterpret_cast<const qf2*>(s_chi)[(c * (A2 / 2) + k) * 64 + lane];
  };

  // ---- cotangent of this channel's final state (bilinear <Z> forms)
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
    for (int c = 1; c < QC_NCH; ++c) {   // one channel at a time: keeps the live set at one vector
      dvec(c, d);
#pragma unroll
      for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_pk_fma(qc_dup(d[k]), other(c, k), cl[1].a[k]);
    }
  } else {
    dvec(ch, d);
#pragma unroll
    for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_dup(d[k]) * other(0, k);
    if (ch == 2 || ch == 3) {
      dvec(ch + 2, d);
#pragma unroll
      for (int k = 0; k < (1 << N); ++k) cl[1].a[k] = qc_pk_fma(qc_dup(2.f * d[k]), cl[0].a[k], cl[1].a[k]);
    }
  }
  if constexpr (!LOAD) __syncthreads();  // everyone is done reading s_chi

  PG::bwd(cl, prog, trig, umat, n_gates, s_acc + ch * n_params, lane, amp >> 1);

  if (amp & 1) {
    // amplitude encoding: the channel's initial vector IS the input jet, so its cotangent is read off
    // the swept lambda directly: d L / d u_c[k] = 2 Re Lambda_c[k] (no coupling between channels here)
    if (live) {
#pragma unroll
      for (int w = 0; w < N; ++w) abar[((int64_t)ch * N + w) * B + p] = 2.f * cl[1].a[w].x;
    }
    __syncthreads();
  } else {
    // ---- cotangents of the angle jets: Im<Lambda| X_w |phi_c>, evaluated in the frame pulled back through
    // the embedding (qc_gates.h): un-apply the n embedding rotations on Lambda, then sparse reads
    const float* aj = qc_launder(ajets);
    float ca[N], sa[N], da[N], dda[N];
    load_sincos<N>(ca, sa, aj, B, pc, trig, amp >> 1, s_cs);
    qc_unembed<N>(cl[1], ca, sa);
    const int dirch = ch == 0 ? 0 : (ch <= 3 ? ch : ch - 2);  // channel holding the first derivative
#pragma unroll
    for (int w = 0; w < N; ++w) {
      da[w] = ch >= 1 ? aj[((int64_t)dirch * N + w) * B + pc] : 0.f;
      dda[w] = ch >= 4 ? aj[((int64_t)ch * N + w) * B + pc] : 0.f;
    }
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
        r = ((at(0, 0, w) + at(1, 0, w)) + (at(2, 0, w) + at(3, 0, w))) + (at(4, 0, w) + at(5, 0, w));
      else if (ch == 1)
        r = at(1, 1, w);
      else if (ch <= 3)
        r = at(ch, 1, w) + at(ch + 2, 1, w);
      else
        r = at(ch, 2, w);
      if (live) abar[((int64_t)ch * N + w) * B + p] = r;
      if ((amp >> 1) && ch == 0) {   // folded RX layer: d L / d theta_w = sum over points of d L / d angle_w
        const float tot = qc_wave_sum6_to_lane63(live ? r : 0.f);
        if (lane == 63) s_acc[prog[w].slot] += tot;
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < n_params; i += 384) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < 6; ++wv) s += s_acc[wv * n_params + i];
    part[(row0 + bid) * part_stride + i] = s;
  }
}

template <class PG, bool LOAD>
__global__ void __launch_bounds__(384, QC_JB_WAVES) k_jets_bwd(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                  const float* __restrict__ umat, int n_gates, int n_params,
                                                  const float* __restrict__ ajets, const float* __restrict__ qbar,
                                                  float* __restrict__ abar, float* __restrict__ part,
                                                  int64_t part_stride, int64_t row0, int64_t B,
                                                  const float* __restrict__ chi_store, int amp) {
  k_jets_bwd_body<PG, LOAD>(blockIdx.x, prog, trig, umat, n_gates, n_params, ajets, qbar, abar, part, part_stride, row0, B, chi_store, amp);
}

// ---- the fused step's adjoint sweep, second form: block = 3 waves on one 64-point tile, wave = TWO channels
// handled one after the other ({t, value}, {x, xx}, {y, yy}).  Against the six-wave form above:
//   * 5 blocks per CU (15 waves at <= 128 VGPRs) hold the whole grid of BASELINE config 2 (1 024 residual + 228
//     value blocks <= 1 280 slots) in ONE round instead of 2.2 rounds of 512;
//   * no straggler: every wave forms its share D_a chi_a + D_b chi_b of the value channel's cotangent from the two
//     final states it loads anyway and leaves it in LDS; the value channel's wave adds the three shares when its
//     turn comes (second in its wave), instead of 160 extra global loads and five extra D-vector builds up front;
//   * 2 block barriers instead of 3, per-gate wave reductions accumulate over both channels in registers of the
//     same wave, cross-wave traffic in the tail shrinks to the one row that sums over all channels.
// Angle encoding only; ABSORB (leading RX layer folded into the embedding) is fixed when the kernel is compiled.
// `row_of()` returns the tile's partial row and n_params; it is asked for after the last barrier, so that what it is
// computed from (part, its stride, the first row, the tile index) is not held through the sweeps.
struct QcPartRow {
  float* row;
  int n_params;
};
template <class PG, bool ABSORB, class ROW>
__device__ __forceinline__ void k_jets_bwd2_body(const int64_t bid, const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                   const float* __restrict__ umat, int n_gates, int n_params,
                                                   const float* __restrict__ ajets, const float* __restrict__ qbar,
                                                   float* __restrict__ abar, const ROW row_of, int64_t B,
                                                   const float* __restrict__ chi_store) {
  constexpr int N = PG::N;
  constexpr int A2 = 2 << N;
  constexpr int NA = 1 << N;
  constexpr int AB = ABSORB ? 1 : 0;
  extern __shared__ float smem[];
  float* s_l0 = smem;                          // [3 waves][A2][64]: shares of lam_0
  float* s_t0 = s_l0 + 3 * A2 * 64;            // [2][N][64]: waves 1, 2: their channels' terms of abar[0]
  float* s_cs = s_t0 + 2 * N * 64;             // [cos | sin][N][64] of the embedding half-angles
  float* s_acc = s_cs + 2 * N * 64;            // [3 waves][n_params]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t p = (int64_t)bid * 64 + lane;
  const bool live = p < B;
  const int64_t pc = live ? p : B - 1;
  for (int i = threadIdx.x; i < 3 * n_params; i += 192) s_acc[i] = 0.f;
  // wires wv, wv + 3, ... of the embedding half-angles
  for (int w = wv; w < N; w += 3) qc_wire_sincos<AB>(s_cs[w * 64 + lane], s_cs[(N + w) * 64 + lane], ajets, B, pc, w, trig, AB);
  // the point index as an opaque value: addresses derived from it are recomputed at their use instead of being hoisted
  // above the two-channel loop and held (or spilled) for the whole kernel
  auto pcf = [&]() {
    int64_t v = pc;
    asm volatile("" : "+v"(v));
    return v;
  };
  // the wave index as an opaque value, for the same reason (it and the channel numbers are rebuilt per sweep and in
  // the tail from the thread index, a register that lives anyway)
  auto wvf = [&]() { return __builtin_amdgcn_readfirstlane(qc_opaque_v((int)threadIdx.x) >> 6); };
  const int cha = wv == 0 ? 1 : wv + 1;        // first channel of this wave: t, x, y
  const int chb = wv == 0 ? 0 : wv + 3;        // second: value, xx, yy

  const qf2* chi2 = reinterpret_cast<const qf2*>(chi_store);
  qf2* s_l02 = reinterpret_cast<qf2*>(s_l0);     // [3 waves][amplitude][64]
  auto load_chi = [&](SV<N>& v, int c) { qc_chi_read<N>(v, chi_store, c, pcf()); };
  auto dvec = [&](int c, QcPk<NA>& d) {
    float qb[N];
    const int64_t pq = pcf(), Bq = qc_opaque_s(B);   // (row addresses rebuilt per call, not held between calls)
#pragma unroll
    for (int w = 0; w < N; ++w) qb[w] = live ? qbar[((int64_t)c * N + w) * Bq + pq] : 0.f;
    qc_sign_sums<N>(d, qb);
  };

  SV<N> cl[2];
  QcPk<NA> d;
  {
    // this wave's share of lam_0 = sum_c D_c chi_c (to LDS), and lam of its first channel; the second channel's final
    // state and chi_0 stream through (they are reloaded when their turn comes) to keep the live set at two vectors
    QcPk<NA> da_;
    qf2* mine = s_l02 + wv * NA * 64;
    load_chi(cl[0], cha);
    dvec(cha, da_);
    dvec(chb, d);
    if (wv == 0) {            // second channel = the value channel: lam_t = D_t chi_0
      load_chi(cl[1], 0);
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        mine[k * 64 + lane] = qc_pk_fma(qc_dup(da_[k]), cl[0].a[k], qc_dup(d[k]) * cl[1].a[k]);
        cl[1].a[k] *= qc_dup(da_[k]);
      }
    } else {                  // lam_x = D_x chi_0 + 2 D_xx chi_x (the same for y)
      const int64_t pqs = pcf();
#pragma unroll
      for (int k = 0; k < NA; ++k)
        mine[k * 64 + lane] = qc_pk_fma(qc_dup(da_[k]), cl[0].a[k], qc_dup(d[k]) * chi2[qc_chi_pair<A2>(chb, k, pqs)]);
#pragma unroll
      for (int k = 0; k < NA; ++k)
        cl[1].a[k] = qc_pk_fma(qc_dup(2.f * d[k]), cl[0].a[k], qc_dup(da_[k]) * chi2[qc_chi_pair<A2>(0, k, pqs)]);
    }
  }
  __syncthreads();   // shares of lam_0, s_cs, s_acc

  float t_own[N];    // this wave's channels' terms of abar[0] (against their own embedded state)
  float t_a1[N];     // first channel, against phi: abar[cha]'s first term
#pragma unroll
  for (int w = 0; w < N; ++w) t_own[w] = t_a1[w] = 0.f;
  const float* aj = qc_launder(ajets);

#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const int wq = wvf();
    const int chb = wq == 0 ? 0 : wq + 3;
    const int ch = half == 0 ? (wq == 0 ? 1 : wq + 1) : chb;
    if (half == 1) {
      load_chi(cl[0], chb);
      if (wq == 0) {          // lam_0: the three shares
#pragma unroll
        for (int k = 0; k < NA; ++k)
          cl[1].a[k] = (s_l02[k * 64 + lane] + s_l02[(NA + k) * 64 + lane]) + s_l02[(2 * NA + k) * 64 + lane];
      } else {                // lam_xx = D_xx chi_0
        dvec(chb, d);
        const int64_t pqs = pcf();
#pragma unroll
        for (int k = 0; k < NA; ++k) cl[1].a[k] = qc_dup(d[k]) * chi2[qc_chi_pair<A2>(0, k, pqs)];
      }
    }
    PG::template bwd<AB>(cl, prog, trig, umat, n_gates, s_acc + wq * n_params, lane, AB);

    // cotangents of the angle jets in the frame pulled back through the embedding (qc_gates.h)
    float ca[N], sa[N], da[N], dda[N];
    const int64_t pq = pcf(), Bq = qc_opaque_s(B);
    load_sincos_lds<N>(ca, sa, s_cs);
    qc_unembed<N>(cl[1], ca, sa);
    const int dirch = ch == 0 ? 0 : (ch <= 3 ? ch : ch - 2);
#pragma unroll
    for (int w = 0; w < N; ++w) {
      da[w] = ch >= 1 ? aj[((int64_t)dirch * N + w) * Bq + pq] : 0.f;
      dda[w] = ch >= 4 ? aj[((int64_t)ch * N + w) * Bq + pq] : 0.f;
    }
    float T[N];
    if (ch == 0) {
      qc_pull_ip0<N>(T, cl[1]);
#pragma unroll
      for (int w = 0; w < N; ++w) t_own[w] += T[w];
    } else if (ch <= 3) {
      qc_pull_ip1<N>(T, cl[1], da);
#pragma unroll
      for (int w = 0; w < N; ++w) t_own[w] += T[w];
      qc_pull_ip0<N>(T, cl[1]);
#pragma unroll
      for (int w = 0; w < N; ++w) t_a1[w] = T[w];
    } else {
      qc_pull_ip2<N>(T, cl[1], da, dda);
#pragma unroll
      for (int w = 0; w < N; ++w) t_own[w] += T[w];
      qc_pull_ip1<N>(T, cl[1], da);
#pragma unroll
      for (int w = 0; w < N; ++w) t_a1[w] = fmaf(2.f, T[w], t_a1[w]);   // abar[x] = ip0(mu_x) + 2 ip1(mu_xx)
      qc_pull_ip0<N>(T, cl[1]);
      if (live) {
#pragma unroll
        for (int w = 0; w < N; ++w) abar[((int64_t)ch * N + w) * Bq + p] = T[w];   // abar[xx] = ip0(mu_xx)
      }
    }
  }
  const int wt = wvf();
  if (live) {
#pragma unroll
    for (int w = 0; w < N; ++w) abar[((int64_t)(wt == 0 ? 1 : wt + 1) * N + w) * B + p] = t_a1[w];
  }
  if (wt != 0) {
#pragma unroll
    for (int w = 0; w < N; ++w) s_t0[((wt - 1) * N + w) * 64 + lane] = t_own[w];
  }
  __syncthreads();
  if (wt == 0) {
    float tot[N];
#pragma unroll
    for (int w = 0; w < N; ++w) {
      const float r = (t_own[w] + s_t0[w * 64 + lane]) + s_t0[(N + w) * 64 + lane];
      if (live) abar[(int64_t)w * B + p] = r;
      tot[w] = live ? r : 0.f;
    }
    if constexpr (ABSORB) {   // folded RX layer: d L / d theta_w = sum over points of d L / d angle_w
      qc_wave_sum_merged<N>(tot);   // the N sums together; each total in its home lane
#pragma unroll
      for (int w = 0; w < N; ++w)
        if (lane == qc_wave_sum_home_lane(N, w)) s_acc[PG::lead_slot(prog, w)] += tot[qc_wave_sum_home_reg(N, w)];
    }
  }
  __syncthreads();
  const QcPartRow pr = row_of();
  float* __restrict__ row = pr.row;
  for (int i = threadIdx.x; i < pr.n_params; i += 192) row[i] = (s_acc[i] + s_acc[pr.n_params + i]) + s_acc[2 * pr.n_params + i];
}

// ---- residual + value tiles in one launch (see qc_mlp.hip): blocks [0, n_val) run the value-channel kernel on
// 6 x 64 boundary / initial points, the rest the six-channel kernel on a 64-point residual tile
template <class PG>
__global__ void __launch_bounds__(384) k_circ_fwd_both(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                       const float* __restrict__ umat, int n_gates,
                                                       const float* __restrict__ ajets, float* __restrict__ qjets, int64_t Br,
                                                       float* __restrict__ chi_store, const float* __restrict__ angles,
                                                       float* __restrict__ expval, int64_t Bv, int amp, int n_val) {
  if ((int)blockIdx.x >= n_val) k_jets_fwd_body<PG>(blockIdx.x - n_val, prog, trig, umat, n_gates, ajets, qjets, Br, chi_store, amp);
  else k_value_fwd_body<PG, 6>(blockIdx.x, prog, trig, umat, n_gates, angles, expval, Bv, amp);
}

template <class PG>
__global__ void __launch_bounds__(384, QC_JB_WAVES) k_circ_bwd_both(
    const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig, const float* __restrict__ umat, int n_gates, int n_params,
    const float* __restrict__ ajets, const float* __restrict__ qbar, float* __restrict__ abar, int64_t row0_r, int64_t Br,
    const float* __restrict__ chi_store, const float* __restrict__ angles, const float* __restrict__ cot,
    float* __restrict__ d_angles, int64_t row0_v, int64_t Bv, float* __restrict__ part, int64_t part_stride, int amp, int n_val) {
  if ((int)blockIdx.x >= n_val)
    k_jets_bwd_body<PG, true>(blockIdx.x - n_val, prog, trig, umat, n_gates, n_params, ajets, qbar, abar, part, part_stride, row0_r, Br,
                              chi_store, amp);
  else
    k_value_bwd_body<PG, 6>(blockIdx.x, prog, trig, umat, n_gates, n_params, angles, cot, d_angles, part, part_stride,
                            row0_v, Bv, amp);
}

// the same stage with 3-wave blocks (k_jets_bwd2_body); angle encoding only (the merged step's precondition), the
// absorb flag a template parameter.  The arguments of the two bodies travel as two by-value records inside the one
// kernel argument, and a block reads only what its own body needs, inside its branch: the argument is read through the
// kernel-argument segment itself (explicit arguments start at its offset 0, AMDGPU ABI) behind an opaque pointer, so
// the requests cannot be merged into one wide load at the kernel's entry and held (or spilled) by both bodies.
struct QcBwdResArgs {
  const float* ajets;
  const float* qbar;
  float* abar;
  const float* chi_store;
  int64_t row0, B;
};
struct QcBwdValArgs {
  const float* angles;
  const float* cot;
  float* d_angles;
  int64_t row0, B;
};
struct QcBwd2Args {
  const QcGate* prog;
  const QcTrig* trig;
  const float* umat;
  int n_gates, n_params;
  float* part;
  int64_t part_stride;
  int n_val;
  QcBwdResArgs res;
  QcBwdValArgs val;
};
template <class PG, bool ABSORB>
__global__ void __launch_bounds__(192, 4) k_circ_bwd_both2(const QcBwd2Args) {
  using Args = const __attribute__((address_space(4))) QcBwd2Args*;
  const Args a0 = (Args)__builtin_amdgcn_kernarg_segment_ptr();
  auto args = [&]() {
    Args a = a0;
    asm volatile("" : "+s"(a));
    return a;
  };
  const int n_val = a0->n_val;
  if ((int)blockIdx.x >= n_val) {
    const Args a = args();
    k_jets_bwd2_body<PG, ABSORB>(
        blockIdx.x - n_val, a->prog, a->trig, a->umat, a->n_gates, a->n_params, a->res.ajets, a->res.qbar, a->res.abar,
        [&]() {
          const Args t = args();
          return QcPartRow{t->part + (t->res.row0 + ((int)blockIdx.x - t->n_val)) * t->part_stride, t->n_params};
        },
        a->res.B, a->res.chi_store);
  } else {
    const Args a = args();
    k_value_bwd_body<PG, 3, ABSORB ? 1 : 0>(blockIdx.x, a->prog, a->trig, a->umat, a->n_gates, a->n_params, a->val.angles,
                                            a->val.cot, a->val.d_angles, a->part, a->part_stride, a->val.row0, a->val.B, 0);
  }
}

// ---- ensembles (qc_internal.h, QcEns): the two merged circuit stages over the tiles of M members, grid (tiles of one
// member, M).  Member blockIdx.y reads its own trig buffer (per-gate entries and phase tables), jets, cotangents, final-state
// store and partial rows; the program and umat are shared.  The tile runs the bodies of k_circ_fwd_both and of
// k_circ_bwd_both2, whose argument record travels inside this one with the strides behind it (read, like it, through the
// kernel-argument segment inside the branch that needs it).
template <class PG>
__global__ void __launch_bounds__(384) k_circ_fwd_ens(const QcGate* __restrict__ prog, const QcTrig* __restrict__ trig,
                                                      const float* __restrict__ umat, int n_gates,
                                                      const float* __restrict__ ajets, float* __restrict__ qjets, int64_t Br,
                                                      float* __restrict__ chi_store, const float* __restrict__ angles,
                                                      float* __restrict__ expval, int64_t Bv, int amp, int n_val, QcEns e) {
  const int64_t m = blockIdx.y;
  trig = (const QcTrig*)((const char*)trig + m * e.trig);
  if ((int)blockIdx.x >= n_val)
    k_jets_fwd_body<PG>(blockIdx.x - n_val, prog, trig, umat, n_gates, ajets + m * e.jets_res, qjets + m * e.jets_res, Br,
                        (float*)((char*)chi_store + m * e.ws), amp);
  else
    k_value_fwd_body<PG, 6>(blockIdx.x, prog, trig, umat, n_gates, angles + m * e.jets_val, expval + m * e.jets_val, Bv, amp);
}

struct QcBwd2EnsArgs {
  QcBwd2Args a;
  QcEns e;
};
template <class PG, bool ABSORB>
__global__ void __launch_bounds__(192, 4) k_circ_bwd_ens2(const QcBwd2EnsArgs) {
  using Args = const __attribute__((address_space(4))) QcBwd2EnsArgs*;
  const Args a0 = (Args)__builtin_amdgcn_kernarg_segment_ptr();
  auto args = [&]() {
    Args a = a0;
    asm volatile("" : "+s"(a));
    return a;
  };
  const int n_val = a0->a.n_val;
  const int64_t m = blockIdx.y;
  if ((int)blockIdx.x >= n_val) {
    const Args t = args();
    const int64_t jr = m * t->e.jets_res;
    k_jets_bwd2_body<PG, ABSORB>(
        blockIdx.x - n_val, t->a.prog, (const QcTrig*)((const char*)t->a.trig + m * t->e.trig), t->a.umat, t->a.n_gates,
        t->a.n_params, t->a.res.ajets + jr, t->a.res.qbar + jr, t->a.res.abar + jr,
        [&]() {
          const Args u = args();
          return QcPartRow{u->a.part + (int64_t)blockIdx.y * u->e.part +
                               (u->a.res.row0 + ((int)blockIdx.x - u->a.n_val)) * u->a.part_stride,
                           u->a.n_params};
        },
        t->a.res.B, (const float*)((const char*)t->a.res.chi_store + m * t->e.ws));
  } else {
    const Args t = args();
    const int64_t jv = m * t->e.jets_val;
    k_value_bwd_body<PG, 3, ABSORB ? 1 : 0>(blockIdx.x, t->a.prog, (const QcTrig*)((const char*)t->a.trig + m * t->e.trig),
                                            t->a.umat, t->a.n_gates, t->a.n_params, t->a.val.angles + jv, t->a.val.cot + jv,
                                            t->a.val.d_angles + jv, t->a.part + m * t->e.part, t->a.part_stride, t->a.val.row0,
                                            t->a.val.B, 0);
  }
}

}  // namespace

// bit 0: amplitude encoding; bit 1: leading RX layer folded into the embedding (QC_NO_ABSORB=1 disables)
static inline int qc_embed_flags(const qc_program* pg) {
  static const bool off = [] { const char* e = getenv("QC_NO_ABSORB"); return e && e[0] == '1'; }();
  const int absorb = (pg->lead_rx && !pg->amplitude && !off) ? 2 : 0;
  return (pg->amplitude ? 1 : 0) | absorb;
}

// ------------------------------------------------------------------ launch helpers (per policy)
struct QcRegLaunchers {
  int (*value_fwd)(const qc_program*, const QcTrig*, const float*, const float*, float*, int64_t, hipStream_t);
  int (*value_bwd)(const qc_program*, const QcTrig*, const float*, const float*, const float*, float*, float*,
                   int64_t, int64_t, int64_t, hipStream_t);
  int (*jets_fwd)(const qc_program*, const QcTrig*, const float*, const float*, float*, int64_t, float*, hipStream_t);
  int (*jets_bwd)(const qc_program*, const QcTrig*, const float*, const float*, const float*, float*, float*,
                  int64_t, int64_t, int64_t, const float*, hipStream_t);
  // residual (six channels, chi_store required) + value tiles in one launch
  int (*circ_fwd_both)(const qc_program*, const QcTrig*, const float*, const float*, float*, int64_t, float*, const float*,
                       float*, int64_t, hipStream_t);
  int (*circ_bwd_both)(const qc_program*, const QcTrig*, const float*, const float*, const float*, float*, int64_t, int64_t,
                       const float*, const float*, const float*, float*, int64_t, int64_t, float*, int64_t, hipStream_t);
  // the same two stages over the tiles of an ensemble's members (angle encoding only)
  int (*circ_fwd_ens)(const qc_program*, const QcTrig*, const float*, const float*, float*, int64_t, float*, const float*,
                      float*, int64_t, hipStream_t, const QcEns&);
  int (*circ_bwd_ens)(const qc_program*, const QcTrig*, const float*, const float*, const float*, float*, int64_t, int64_t,
                      const float*, const float*, const float*, float*, int64_t, int64_t, float*, int64_t, hipStream_t,
                      const QcEns&);
};

template <class PG>
struct RegLaunch {
  static int value_fwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* angles,
                       float* expval, int64_t B, hipStream_t st) {
    hipLaunchKernelGGL(k_value_fwd<PG>, dim3(qc_ceil_div(B, 256)), dim3(256), 0, st, pg->d_gates, trig, umat,
                       pg->n_gates, angles, expval, B, qc_embed_flags(pg));
    return QC_OK;
  }
  static int value_bwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* angles,
                       const float* cot, float* d_angles, float* part, int64_t part_stride, int64_t row0,
                       int64_t B, hipStream_t st) {
    const size_t sh = (size_t)4 * pg->n_params * sizeof(float);
    hipLaunchKernelGGL(k_value_bwd<PG>, dim3(qc_ceil_div(B, 256)), dim3(256), sh, st, pg->d_gates, trig, umat,
                       pg->n_gates, pg->n_params, angles, cot, d_angles, part, part_stride, row0, B, qc_embed_flags(pg));
    return QC_OK;
  }
  static int jets_fwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets,
                      float* qjets, int64_t B, float* chi_store, hipStream_t st) {
    hipLaunchKernelGGL(k_jets_fwd<PG>, dim3(qc_ceil_div(B, 64)), dim3(384), 0, st, pg->d_gates, trig, umat,
                       pg->n_gates, ajets, qjets, B, chi_store, qc_embed_flags(pg));
    return QC_OK;
  }
  static int jets_bwd(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets,
                      const float* qbar, float* abar, float* part, int64_t part_stride, int64_t row0, int64_t B,
                      const float* chi_store, hipStream_t st) {
    const size_t sh = ((size_t)6 * (2u << PG::N) * 64 + (size_t)6 * pg->n_params + 2 * PG::N * 64) * sizeof(float);
    const size_t sh_load = ((size_t)6 * 3 * PG::N * 64 + (size_t)6 * pg->n_params + 2 * PG::N * 64) * sizeof(float);
    if (sh > 160 * 1024) return QC_ERR_UNSUPPORTED;
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_jets_bwd<PG, false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_jets_bwd<PG, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      attr_set = true;
    }
    if (chi_store != nullptr)
      hipLaunchKernelGGL((k_jets_bwd<PG, true>), dim3(qc_ceil_div(B, 64)), dim3(384), sh_load, st, pg->d_gates, trig, umat,
                         pg->n_gates, pg->n_params, ajets, qbar, abar, part, part_stride, row0, B, chi_store, qc_embed_flags(pg));
    else
      hipLaunchKernelGGL((k_jets_bwd<PG, false>), dim3(qc_ceil_div(B, 64)), dim3(384), sh, st, pg->d_gates, trig, umat,
                         pg->n_gates, pg->n_params, ajets, qbar, abar, part, part_stride, row0, B, chi_store, qc_embed_flags(pg));
    return QC_OK;
  }
  static int circ_fwd_both(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, float* qjets,
                           int64_t Br, float* chi_store, const float* angles, float* expval, int64_t Bv, hipStream_t st) {
    const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 384);
    hipLaunchKernelGGL(k_circ_fwd_both<PG>, dim3(nr + nv), dim3(384), 0, st, pg->d_gates, trig, umat, pg->n_gates, ajets,
                       qjets, Br, chi_store, angles, expval, Bv, qc_embed_flags(pg), nv);
    return QC_OK;
  }
  static int circ_bwd_both(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets,
                           const float* qbar, float* abar, int64_t row0_r, int64_t Br, const float* chi_store,
                           const float* angles, const float* cot, float* d_angles, int64_t row0_v, int64_t Bv, float* part,
                           int64_t part_stride, hipStream_t st) {
    static const bool six = [] { const char* e = getenv("QC_BWD6"); return e && e[0] == '1'; }();   // A/B: the six-wave form
    if (!six && !pg->amplitude) {
      const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 192);
      const size_t sh = ((size_t)3 * (2u << PG::N) * 64 + (size_t)4 * PG::N * 64 + (size_t)3 * pg->n_params) * sizeof(float);
      const QcBwd2Args args = {pg->d_gates, trig, umat, pg->n_gates, pg->n_params, part, part_stride, nv,
                               {ajets, qbar, abar, chi_store, row0_r, Br}, {angles, cot, d_angles, row0_v, Bv}};
      const bool absorb = (qc_embed_flags(pg) & 2) != 0;
      if constexpr (PG::lead_rx) {   // (a program without the layer never asks for the absorbed form)
        if (absorb) {
          hipLaunchKernelGGL((k_circ_bwd_both2<PG, true>), dim3(nr + nv), dim3(192), sh, st, args);
          return QC_OK;
        }
      } else if (absorb) {
        return QC_ERR_UNSUPPORTED;
      }
      hipLaunchKernelGGL((k_circ_bwd_both2<PG, false>), dim3(nr + nv), dim3(192), sh, st, args);
      return QC_OK;
    }
    const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 384);
    const size_t sh = ((size_t)6 * 3 * PG::N * 64 + (size_t)6 * pg->n_params + 2 * PG::N * 64) * sizeof(float);   // >= the value blocks' 6 rows
    hipLaunchKernelGGL(k_circ_bwd_both<PG>, dim3(nr + nv), dim3(384), sh, st, pg->d_gates, trig, umat, pg->n_gates,
                       pg->n_params, ajets, qbar, abar, row0_r, Br, chi_store, angles, cot, d_angles, row0_v, Bv, part,
                       part_stride, qc_embed_flags(pg), nv);
    return QC_OK;
  }
  static int circ_fwd_ens(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets, float* qjets,
                          int64_t Br, float* chi_store, const float* angles, float* expval, int64_t Bv, hipStream_t st,
                          const QcEns& e) {
    if (pg->amplitude) return QC_ERR_UNSUPPORTED;
    const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 384);
    hipLaunchKernelGGL(k_circ_fwd_ens<PG>, dim3(nr + nv, e.M), dim3(384), 0, st, pg->d_gates, trig, umat, pg->n_gates, ajets,
                       qjets, Br, chi_store, angles, expval, Bv, qc_embed_flags(pg), nv, e);
    return QC_OK;
  }
  static int circ_bwd_ens(const qc_program* pg, const QcTrig* trig, const float* umat, const float* ajets,
                          const float* qbar, float* abar, int64_t row0_r, int64_t Br, const float* chi_store,
                          const float* angles, const float* cot, float* d_angles, int64_t row0_v, int64_t Bv, float* part,
                          int64_t part_stride, hipStream_t st, const QcEns& e) {
    if (pg->amplitude) return QC_ERR_UNSUPPORTED;
    const int nr = qc_ceil_div(Br, 64), nv = qc_ceil_div(Bv, 192);
    const size_t sh = ((size_t)3 * (2u << PG::N) * 64 + (size_t)4 * PG::N * 64 + (size_t)3 * pg->n_params) * sizeof(float);
    const QcBwd2EnsArgs args = {{pg->d_gates, trig, umat, pg->n_gates, pg->n_params, part, part_stride, nv,
                                 {ajets, qbar, abar, chi_store, row0_r, Br}, {angles, cot, d_angles, row0_v, Bv}}, e};
    const bool absorb = (qc_embed_flags(pg) & 2) != 0;
    if constexpr (PG::lead_rx) {
      if (absorb) {
        hipLaunchKernelGGL((k_circ_bwd_ens2<PG, true>), dim3(nr + nv, e.M), dim3(192), sh, st, args);
        return QC_OK;
      }
    } else if (absorb) {
      return QC_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL((k_circ_bwd_ens2<PG, false>), dim3(nr + nv, e.M), dim3(192), sh, st, args);
    return QC_OK;
  }
  static constexpr QcRegLaunchers table() {
    return {&value_fwd, &value_bwd, &jets_fwd, &jets_bwd, &circ_fwd_both, &circ_bwd_both, &circ_fwd_ens, &circ_bwd_ens};
  }
};
