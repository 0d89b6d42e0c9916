// Check of qc_store_wt (csrc/qc_common.h), the write-through store of stage outputs, across launches and XCDs: what a
// later launch reads with PLAIN loads from another XCD must be, word for word, what the store wrote, also where the
// policy of a line changes between launches.
//   k_write<true>   1280 blocks of 192 threads write the buffer with qc_store_wt: per block ROWS rows of 64 floats
//                   (4-byte form) and ROWS rows of 64 (re, im) pairs (8-byte form); row r of block b is written by a
//                   full wave, by lane 0 alone or by lanes 0..62 (a partial last line), by (r + b) % 3.  Entries no lane
//                   writes keep the fill word.
//   k_read          a separate launch on the same stream: block b reads the region of block (b + 3) % gridDim.x, another
//                   XCD under round-robin placement, with plain loads and leaves one checksum.
//   k_write<false>  the same buffer rewritten with other values by plain stores, read by k_read again.
//   k_write<true>   rewritten once more by qc_store_wt, read again: write-through onto lines a plain store left dirty.
// The data are integers exact in fp32.  After every pass the checksums AND a copy of the whole buffer are compared with
// the host's expectation.  Built by csrc/Makefile next to the library; prints one line per pass, exits non-zero on any
// mismatch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "qc_common.h"

constexpr int GRID = 1280, THREADS = 192, WAVES = THREADS / 64;
constexpr int ROWS = 12;                              // per form and block; every wave writes ROWS / WAVES of each
constexpr int WORDS4 = ROWS * 64, WORDS8 = ROWS * 128; // words of a block's float rows, of its pair rows
constexpr int WORDS = WORDS4 + WORDS8;                // words of a block's region (pairs start 8-byte aligned)
constexpr uint32_t FILL = 0xFFFFFFFFu;
static_assert(ROWS % WAVES == 0 && WORDS4 % 2 == 0, "rows per wave; alignment of the pair rows");

__host__ __device__ inline bool lane_writes(const int b, const int r, const int lane) {
  const int mode = (r + b) % 3;   // 0: full wave, 1: lane 0 alone, 2: lanes 0..62
  return mode == 0 || (mode == 1 ? lane == 0 : lane < 63);
}
// integers below 2^24, different for every (pass, form, block, row, lane)
__host__ __device__ inline float value_of(const int pass, const int form, const int b, const int r, const int lane) {
  const uint32_t x = (uint32_t)pass * 2654435761u + (uint32_t)form * 40503u + (uint32_t)b * 9973u + (uint32_t)r * 641u +
                     (uint32_t)lane * 17u;
  return (float)((x ^ (x >> 13)) & 0xFFFFFFu);
}

template <bool WT>
__global__ void __launch_bounds__(THREADS) k_write(float* __restrict__ buf, const int pass) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  float* f4 = buf + (size_t)b * WORDS;
  qf2* f8 = reinterpret_cast<qf2*>(f4 + WORDS4);
  for (int r = wave; r < ROWS; r += WAVES) {
    if (!lane_writes(b, r, lane)) continue;
    const float v = value_of(pass, 0, b, r, lane), w = value_of(pass, 1, b, r, lane);
    const qf2 pair = {w, -w - 1.f};
    if constexpr (WT) {
      qc_store_wt(&f4[r * 64 + lane], v);
      qc_store_wt(&f8[r * 64 + lane], pair);
    } else {
      f4[r * 64 + lane] = v;
      f8[r * 64 + lane] = pair;
    }
  }
}

__host__ __device__ inline uint32_t mix(const uint32_t word, const int i) { return word * (2u * (uint32_t)i + 1u); }

__global__ void __launch_bounds__(THREADS) k_read(const uint32_t* __restrict__ buf, uint32_t* __restrict__ sums) {
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const int rb = (blockIdx.x + 3) % gridDim.x;
  const uint32_t* src = buf + (size_t)rb * WORDS;
  uint32_t acc = 0;
  for (int i = threadIdx.x; i < WORDS; i += THREADS) acc += mix(src[i], i);
  atomicAdd(&s_sum, acc);
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = s_sum;
}

static void expect(std::vector<uint32_t>& e, const int pass) {
  for (int b = 0; b < GRID; ++b)
    for (int r = 0; r < ROWS; ++r)
      for (int lane = 0; lane < 64; ++lane) {
        if (!lane_writes(b, r, lane)) continue;
        float* f4 = reinterpret_cast<float*>(e.data()) + (size_t)b * WORDS;
        qf2* f8 = reinterpret_cast<qf2*>(f4 + WORDS4);
        const float w = value_of(pass, 1, b, r, lane);
        qc_store_wt(&f4[r * 64 + lane], value_of(pass, 0, b, r, lane));   // the host pass of the primitive: a plain store
        qc_store_wt(&f8[r * 64 + lane], (qf2){w, -w - 1.f});
      }
}

int main() {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
    printf("no device\n");
    return 2;
  }
  const size_t n_words = (size_t)GRID * WORDS, nb = n_words * 4;
  float* d_buf = nullptr;
  uint32_t* d_sums = nullptr;
  if (hipMalloc(&d_buf, nb) != hipSuccess || hipMalloc(&d_sums, GRID * 4) != hipSuccess) return 1;
  (void)hipMemset(d_buf, 0xFF, nb);
  std::vector<uint32_t> want(n_words, FILL), got(n_words), sums(GRID);
  const char* names[3] = {"write-through", "plain over write-through", "write-through over plain"};
  int bad_total = 0;
  for (int pass = 1; pass <= 3; ++pass) {
    if (pass == 2) hipLaunchKernelGGL(k_write<false>, dim3(GRID), dim3(THREADS), 0, 0, d_buf, pass);
    else hipLaunchKernelGGL(k_write<true>, dim3(GRID), dim3(THREADS), 0, 0, d_buf, pass);
    (void)hipMemsetAsync(d_sums, 0xFF, GRID * 4, 0);
    hipLaunchKernelGGL(k_read, dim3(GRID), dim3(THREADS), 0, 0, reinterpret_cast<const uint32_t*>(d_buf), d_sums);
    const hipError_t e1 = hipMemcpy(sums.data(), d_sums, GRID * 4, hipMemcpyDeviceToHost);
    const hipError_t e2 = hipMemcpy(got.data(), d_buf, nb, hipMemcpyDeviceToHost);
    if (e1 != hipSuccess || e2 != hipSuccess) {
      printf("pass %d FAIL (%s)\n", pass, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
      return 1;
    }
    expect(want, pass);
    int bad_words = 0, bad_sums = 0;
    for (size_t i = 0; i < n_words; ++i)
      if (got[i] != want[i] && ++bad_words <= 4)
        printf("  pass %d: word %zu (block %zu, word %zu of its region) is %08x, expected %08x\n", pass, i, i / WORDS, i % WORDS,
               got[i], want[i]);
    for (int b = 0; b < GRID; ++b) {
      const int rb = (b + 3) % GRID;
      uint32_t s = 0;
      for (int i = 0; i < WORDS; ++i) s += mix(want[(size_t)rb * WORDS + i], i);
      if (sums[b] != s && ++bad_sums <= 4)
        printf("  pass %d: block %d read the region of block %d as checksum %08x, expected %08x\n", pass, b, rb, sums[b], s);
    }
    printf("pass %d %s (%s): %d blocks x %d words, %d wrong words in the copy, %d wrong checksums of the next launch\n", pass,
           bad_words || bad_sums ? "FAIL" : "PASS", names[pass - 1], GRID, WORDS, bad_words, bad_sums);
    bad_total += bad_words + bad_sums;
  }
  (void)hipFree(d_buf);
  (void)hipFree(d_sums);
  printf("bad=%d\n", bad_total);
  return bad_total != 0;
}
