// dq_split.hip -- the row-level train / test draw of ConstraintSuggestionRunner's split
// (suggestions/ConstraintSuggestionRunner.scala:127-148), on the device and -- the same arithmetic -- on the host.
//
// The draw of a row is a pure function of (seed, global row index g): h = XXH64 of g's 8 little-endian bytes under
// `seed` (dq_hash.h's hashLong formulation with the seed a parameter), u = (h >> 11) * 2^-53 in [0, 1), test iff
// u < test_ratio.  Both steps are exact in fp64 (a 53-bit integer times a power of two), so host and device agree
// bit for bit and a table splits the same way however it is chunked.  Spark's randomSplit cannot be restated: its
// rows depend on the partitioning ("Constraint suggestion").
//
// Kernel (dq_split_kernel): one row per lane, one 64-row bitmap word per wave and iteration, a grid-stride loop
// over the words in 64-bit indices.  The wave's ballot of "test" is the test word, its complement over the rows in
// range the train word (bits past n_rows are 0); lane 0 stores both with plain stores.  A wave sums the popcounts
// of its test words, the workgroup's waves meet in LDS and thread 0 adds the workgroup's sum with one integer
// atomic: no float atomics, the counts do not depend on arrival order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dq_hash.h"
#include "dq_hip_host.h"

namespace dq {
namespace {

constexpr int kSplitBlock = 256;
constexpr int kSplitWaves = kSplitBlock / 64;
constexpr int64_t kSplitMaxGrid = 2048;  // 8 workgroups per CU of 256; the loop strides over the rest

// XXH64 of the 8 little-endian bytes of v under `seed` (XXH64.hashLong: one 8-byte round, then the avalanche)
DQ_HD uint64_t xxh64_long_seeded(uint64_t v, uint64_t seed) {
  const uint64_t k = rotl64(mul_c(v, XP2), 31);
  const uint64_t h = mul_c(k, XP1) ^ (seed + XP5 + 8);
  return fmix64(mul_add_c(rotl64(h, 27), XP1, XP4));
}

DQ_HD bool split_is_test(uint64_t g, uint64_t seed, double test_ratio) {
  const double u = (double)(xxh64_long_seeded(g, seed) >> 11) * 0x1.0p-53;
  return u < test_ratio;
}

__global__ __launch_bounds__(kSplitBlock) void dq_split_kernel(int64_t n_rows, uint64_t row0, uint64_t seed,
                                                               double test_ratio, uint64_t* __restrict__ train,
                                                               uint64_t* __restrict__ test,
                                                               unsigned long long* n_test_total) {
  __shared__ unsigned long long wave_tests[kSplitWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_words = (n_rows + 63) >> 6;
  const int64_t stride = (int64_t)gridDim.x * kSplitWaves;
  unsigned long long n_test = 0;  // wave-uniform
  for (int64_t w = (int64_t)blockIdx.x * kSplitWaves + wave; w < n_words; w += stride) {
    const int64_t r = w * 64 + lane;
    const bool in = r < n_rows;
    const bool is_test = in && split_is_test(row0 + (uint64_t)r, seed, test_ratio);
    const uint64_t tm = __builtin_amdgcn_ballot_w64(is_test);
    const uint64_t im = __builtin_amdgcn_ballot_w64(in);
    if (lane == 0) {
      test[w] = tm;
      train[w] = im & ~tm;
    }
    n_test += (unsigned long long)__builtin_popcountll(tm);
  }
  if (lane == 0) wave_tests[wave] = n_test;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int k = 0; k < kSplitWaves; ++k) s += wave_tests[k];
    if (s != 0) atomicAdd(n_test_total, s);
  }
}

// the argument checks both entry points share; rows are numbered row0 .. row0 + n_rows - 1 in int64
dq_status split_check(const char* me, int64_t n_rows, int64_t row0, double test_ratio) {
  if (n_rows < 0 || row0 < 0 || row0 > INT64_MAX - n_rows) return set_error(DQ_E_INVALID, "%s: bad row range", me);
  if (!(test_ratio > 0.0 && test_ratio < 1.0))  // (NaN fails both comparisons)
    return set_error(DQ_E_INVALID, "%s: test_ratio %g is not in ]0, 1[", me, test_ratio);
  return DQ_OK;
}

}  // namespace
}  // namespace dq

extern "C" {

dq_status dq_split_rows(int64_t n_rows, int64_t row0, uint64_t seed, double test_ratio, uint64_t* train_bitmap,
                        uint64_t* test_bitmap, int32_t device, void* hip_stream, int64_t* num_train,
                        int64_t* num_test) {
  using namespace dq;
  const char* me = "dq_split_rows";
  if (dq_status s = split_check(me, n_rows, row0, test_ratio)) return s;
  if (num_train) *num_train = 0;
  if (num_test) *num_test = 0;
  if (n_rows == 0) return DQ_OK;
  if (!train_bitmap || !test_bitmap || ((uintptr_t)train_bitmap & 7) || ((uintptr_t)test_bitmap & 7))
    return set_error(DQ_E_INVALID, "%s: NULL or misaligned bitmap", me);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  DevPtr<unsigned long long> counter;
  DQ_HIP(counter.alloc(1));
  DQ_HIP(hipMemsetAsync(counter.get(), 0, 8, st));
  const int64_t n_words = (n_rows + 63) >> 6;
  const int64_t blocks = (n_words + kSplitWaves - 1) / kSplitWaves;
  const unsigned grid = (unsigned)(blocks < kSplitMaxGrid ? blocks : kSplitMaxGrid);
  hipLaunchKernelGGL(dq_split_kernel, dim3(grid), dim3(kSplitBlock), 0, st, n_rows, (uint64_t)row0, seed, test_ratio,
                     train_bitmap, test_bitmap, counter.get());
  DQ_HIP(hipGetLastError());
  unsigned long long h = 0;
  DQ_HIP(hipMemcpyAsync(&h, counter.get(), 8, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (num_test) *num_test = (int64_t)h;
  if (num_train) *num_train = n_rows - (int64_t)h;
  return DQ_OK;
}

dq_status dq_split_rows_host(int64_t n_rows, int64_t row0, uint64_t seed, double test_ratio, uint8_t* is_test) {
  using namespace dq;
  const char* me = "dq_split_rows_host";
  if (dq_status s = split_check(me, n_rows, row0, test_ratio)) return s;
  if (n_rows == 0) return DQ_OK;
  if (!is_test) return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
  for (int64_t r = 0; r < n_rows; ++r) is_test[r] = split_is_test((uint64_t)row0 + (uint64_t)r, seed, test_ratio) ? 1 : 0;
  return DQ_OK;
}

}  // extern "C"
