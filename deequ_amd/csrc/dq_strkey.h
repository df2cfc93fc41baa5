// dq_strkey.h -- the 64-bit tuple hash's pieces and the exact string compare that go with it, shared by the
// grouping pass (dq_group.hip) and the fused categorical histograms (dq_cathist.hip): a string hashed by this file
// has the same key in both, and DQ_TEST_GROUP_HASH_MASK narrows both.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "dq_hash.h"

namespace dq {

typedef uint64_t strkey_u64u __attribute__((aligned(1)));
typedef uint32_t strkey_u32u __attribute__((aligned(1)));

__device__ __forceinline__ uint64_t mix8(uint64_t h, uint64_t k) {
  return mul_add_c(rotl64(h ^ mul_add_c(k, XP2, 0), 27), XP1, XP4);
}

// the bytes of row r of a string column (int64 offsets when large)
__device__ __forceinline__ void str_of(const void* values, const void* offsets, bool large, int64_t r, const uint8_t*& p,
                                       int64_t& len) {
  int64_t o0, o1;
  if (large) {
    o0 = reinterpret_cast<const int64_t*>(offsets)[r];
    o1 = reinterpret_cast<const int64_t*>(offsets)[r + 1];
  } else {
    o0 = reinterpret_cast<const int32_t*>(offsets)[r];
    o1 = reinterpret_cast<const int32_t*>(offsets)[r + 1];
  }
  p = reinterpret_cast<const uint8_t*>(values) + o0;
  len = o1 - o0;
}

// one string folded into the running tuple hash h: its bytes and its length
__device__ __forceinline__ uint64_t mix_str(uint64_t h, const uint8_t* p, int64_t len) {
  // little-endian words by (unaligned) 8- / 4-byte loads -- the same k as assembling the bytes one by one
  int64_t i = 0;
  for (; i + 8 <= len; i += 8) h = mix8(h, *reinterpret_cast<const strkey_u64u*>(p + i));
  uint64_t k = 0;
  int b = 0;
  if (i + 4 <= len) {
    k = *reinterpret_cast<const strkey_u32u*>(p + i);
    b = 4;
  }
  for (; i + b < len; ++b) k |= (uint64_t)p[i + b] << (8 * b);
  return mix8(h, k ^ ((uint64_t)len << 56) ^ 0xA5);
}

// the tuple hash of a single string column's value (what dq_group.hip's tuple_hash gives a one-column tuple)
__device__ __forceinline__ uint64_t str_tuple_hash(const uint8_t* p, int64_t len, uint64_t seed = kSeed) {
  return fmix64(mix_str(seed + XP5, p, len));
}

// 8 bytes, then 4, then single bytes per step (gfx950 global loads take any byte address; none reads past
// either string): 8x fewer scattered loads than a byte loop (verify_runs over 1e8 C5 strings 17.4 ms, r4g3)
__device__ __forceinline__ bool bytes_equal(const uint8_t* pa, const uint8_t* pb, int64_t len) {
  int64_t i = 0;
  for (; i + 8 <= len; i += 8)
    if (*reinterpret_cast<const strkey_u64u*>(pa + i) != *reinterpret_cast<const strkey_u64u*>(pb + i)) return false;
  if (i + 4 <= len) {
    if (*reinterpret_cast<const strkey_u32u*>(pa + i) != *reinterpret_cast<const strkey_u32u*>(pb + i)) return false;
    i += 4;
  }
  for (; i < len; ++i)
    if (pa[i] != pb[i]) return false;
  return true;
}

// test hook: keep only some bits of the primary tuple hash, to force collisions between distinct tuples
inline uint64_t test_hash_mask() {
  if (const char* e = std::getenv("DQ_TEST_GROUP_HASH_MASK")) return std::strtoull(e, nullptr, 16);
  return ~0ull;
}

}  // namespace dq
