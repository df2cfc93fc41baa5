// dq_lane.h -- small gfx950 device helpers shared by the scan kernels (lane-per-row layouts: lane l of a
// wave holds row base + l, so the selection of 64 rows is one 64-bit scalar mask).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dq {

// Hardware v_min_f64 / v_max_f64 (IEEE mode: a NaN operand yields the other operand).  Inline asm
// keeps the compiler from canonicalising both inputs first (two extra v_max_f64 per call).
__device__ __forceinline__ double hw_min(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double hw_max(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// scalar (constant address space) loads: a bitmap word read with s_load into SGPRs
typedef const __attribute__((address_space(4))) uint32_t* const_u32s;

__device__ __forceinline__ uint64_t load_word64(const uint32_t* p, int64_t w) {
  return ((uint64_t)((const_u32s)p)[w + 1] << 32) | ((const_u32s)p)[w];
}

// this lane's bit of a wave-uniform 64-bit row mask (inverse ballot: no VALU work)
__device__ __forceinline__ bool lane_bit(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

// The selection word of a 64-row group: bits of rows [base, base + 64) of validity & mask, clipped to the rows
// below row1.  w = base / 32, the group's first dword (base % 64 == 0); left = row1 - base > 0, a 32-bit value
// where the caller has one (the scalar unit has no 64-bit ordered compare).  A null bitmap is all ones; a dword
// that holds no row below row1 is not read.  VEC: per-lane w (vector loads); else wave-uniform w (scalar loads).
template <bool VEC = false, typename L>
__device__ __forceinline__ uint64_t sel_word(const uint32_t* validity, const uint32_t* mask, int64_t w, L left) {
  const bool two = left > 32;  // the second dword holds rows below row1
  auto word = [&](const uint32_t* bm) -> uint64_t {
    if (!bm) return ~0ull;
    if constexpr (VEC) return ((uint64_t)(two ? bm[w + 1] : 0u) << 32) | bm[w];
    else return ((uint64_t)(two ? ((const_u32s)bm)[w + 1] : 0u) << 32) | ((const_u32s)bm)[w];
  };
  uint64_t x = word(validity) & word(mask);
  if (left < 64) x &= (1ull << left) - 1ull;
  return x;
}
template <bool VEC = false, typename L>
__device__ __forceinline__ uint64_t sel_word(const uint32_t* bm, int64_t w, L left) {
  return sel_word<VEC>(bm, nullptr, w, left);
}

// Wave reductions (xor butterfly 32 .. 1: a fixed order, every lane ends with the result) and a wave-uniform
// double as an SGPR pair.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {  // wrapping
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = (int64_t)((uint64_t)v + (uint64_t)__shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = hw_min(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = hw_max(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ double wave_uniform(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

}  // namespace dq
