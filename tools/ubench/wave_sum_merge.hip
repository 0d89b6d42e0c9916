// Lane-exactness check of qc_wave_sum_merged<NV> (csrc/qc_common.h) for NV = 1..16: every value's total, read from its
// home lane and home register, must have the BITS of qc_wave_sum_to_lane63 of the same data.
//   random trials : finite floats of mixed sign and magnitude (a changed association tree shows as changed rounding)
//   one-hot trials: value j is zero except for one lane, which holds a power of two that no other value of the trial
//                   holds; trial t puts it in lane (t + 5 j) % 64, so that every lane of every value is the hot one once
//                   (a lane left out, counted twice or credited to another value shows as a wrong power of two)
// (Inputs come from memory here.  Where a kernel sums a product, the compiler may contract the multiply into the first step
// of either form, and whether it does is its choice per call site: a comparison of two call sites in one program would test
// that choice, not the lanes.  That case is covered by comparing a step's outputs byte for byte with the parent build's.)
// Built by csrc/Makefile next to the library; prints one line per NV and exits non-zero on any mismatch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <utility>
#include <vector>

#include "qc_common.h"

constexpr int N_RANDOM = 192, N_HOT = 64, N_TRIALS = N_RANDOM + N_HOT;

template <int NV>
__global__ void __launch_bounds__(64) k_sums(const float* __restrict__ in, float* __restrict__ merged, float* __restrict__ ref) {
  const int lane = threadIdx.x, t = blockIdx.x;
  float v[NV], r[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = in[((size_t)t * NV + k) * 64 + lane];
#pragma unroll
  for (int k = 0; k < NV; ++k) r[k] = qc_wave_sum_to_lane63(v[k]);
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < NV; ++k) ref[t * NV + k] = r[k];
  }
  qc_wave_sum_merged<NV>(v);
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (lane == qc_wave_sum_home_lane(NV, k)) merged[t * NV + k] = v[qc_wave_sum_home_reg(NV, k)];
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}
static float hot_value(int t, int j) { return ldexpf(1.f, 2 * j - 16 + t % 7) * ((t + j) & 1 ? -1.f : 1.f); }

template <int NV>
static int one() {
  std::vector<float> h((size_t)N_TRIALS * NV * 64, 0.f);
  for (int t = 0; t < N_RANDOM; ++t)
    for (int k = 0; k < NV; ++k)
      for (int l = 0; l < 64; ++l) {
        // sign, a mantissa of 24 random bits, an exponent spread over 2^-12 .. 2^12 (every third trial: narrow, so that
        // most additions round)
        const int span = t % 3 == 0 ? 3 : 25;
        const float m = 1.f + (float)(rng() & 0x7FFFFF) / 8388608.f;
        const float x = ldexpf(m, (int)(rng() % span) - span / 2);
        h[((size_t)t * NV + k) * 64 + l] = (rng() & 1) ? -x : x;
      }
  for (int t = 0; t < N_HOT; ++t)
    for (int k = 0; k < NV; ++k) h[((size_t)(N_RANDOM + t) * NV + k) * 64 + (t + 5 * k) % 64] = hot_value(t, k);
  float *d_in, *d_m, *d_r;
  const size_t nb = h.size() * sizeof(float), ob = (size_t)N_TRIALS * NV * sizeof(float);
  if (hipMalloc(&d_in, nb) != hipSuccess || hipMalloc(&d_m, ob) != hipSuccess || hipMalloc(&d_r, ob) != hipSuccess) return 1;
  (void)hipMemcpy(d_in, h.data(), nb, hipMemcpyHostToDevice);
  (void)hipMemset(d_m, 0xFF, ob);
  (void)hipMemset(d_r, 0xFF, ob);
  hipLaunchKernelGGL((k_sums<NV>), dim3(N_TRIALS), dim3(64), 0, 0, d_in, d_m, d_r);
  std::vector<float> m((size_t)N_TRIALS * NV), r((size_t)N_TRIALS * NV);
  const hipError_t e1 = hipMemcpy(m.data(), d_m, ob, hipMemcpyDeviceToHost);
  const hipError_t e2 = hipMemcpy(r.data(), d_r, ob, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_m);
  (void)hipFree(d_r);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    printf("NV=%2d FAIL (%s)\n", NV, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return 1;
  }
  int bad = 0;
  for (int t = 0; t < N_TRIALS; ++t)
    for (int k = 0; k < NV; ++k) {
      const float got = m[(size_t)t * NV + k], want = r[(size_t)t * NV + k];
      bool wrong = memcmp(&got, &want, 4) != 0;
      if (t >= N_RANDOM) {
        const float hv = hot_value(t - N_RANDOM, k);
        wrong = wrong || memcmp(&want, &hv, 4) != 0;
      }
      if (wrong && ++bad <= 4)
        printf("  NV=%d trial %d (%s) value %d: home lane %d of register %d holds %a, lane 63 of the reference %a\n", NV, t,
               t < N_RANDOM ? "random" : "one-hot", k, qc_wave_sum_home_lane(NV, k), qc_wave_sum_home_reg(NV, k), got, want);
    }
  printf("NV=%2d %s: %d random + %d one-hot trials x %d values, %d mismatches; home lanes", NV, bad ? "FAIL" : "PASS",
         N_RANDOM, N_HOT, NV, bad);
  for (int k = 0; k < NV; ++k) printf(" %d", qc_wave_sum_home_lane(NV, k));
  printf("\n");
  return bad != 0;
}

template <int... NVs>
static int all(std::integer_sequence<int, NVs...>) {
  return (one<NVs + 1>() + ...);
}

int main() {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
    printf("no device\n");
    return 2;
  }
  const int bad = all(std::make_integer_sequence<int, 16>{});
  printf("bad=%d\n", bad);
  return bad != 0;
}
