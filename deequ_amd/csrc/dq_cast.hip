// dq_cast.hip -- dq_cast_utf8: Spark 2.2's Cast(StringType -> LongType | DoubleType) of a UTF8 column, materialised
// as an I64 / F64 column with its validity bitmap (what the ColumnProfiler's castNumericStringColumns hands its
// second pass: profiles/ColumnProfiler.scala:133-141, 330-339, 399-417).  The per-value rules are dq_cast.h's
// (UTF8String.toLong; java.lang.Double.parseDouble).
//
// One row per lane, wave w of a block takes kGroupsPerWave consecutive 64-row groups.  A lane reads its two
// offsets, walks its string through aligned dwords (only dwords that hold a byte of the string: the data buffer
// is readable up to the 4-byte boundary past its last string) and stores its 8-byte value; the wave's ballot of
// "not NULL" is the group's validity word, stored by lane 0 (bits past n_rows are 0).  No atomics touch values or
// validity: the only atomics are the two counters (NULL rows, one add per wave; hard rows, one add per group that
// has any).
//
// Double conversion, hard tier: a valid value outside dq_cast.h's fast tier (more than 38 significant digits, a
// net exponent outside [-38, 0] whose integer does not fit 38 digits, a hex float) appends its row index to a
// device list (capacity-checked; a list that overflows is sized for the reported count and the cast rerun).  The
// host gathers those rows' bytes, converts each with glibc's strtod in the C locale -- correctly rounded for
// decimal and hex input; dq_cast.h has already enforced Java's grammar and delimited the text strtod reads --
// and scatters the values back.  Hard rows are valid rows, so the validity words need no patch.
#include <hip/hip_runtime.h>

#include <clocale>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <locale.h>

#include "dq_cast.h"
#include "dq_hip_host.h"

#define DQ_DEC_TABLE static __constant__ const
#include "dq_dec_tables.inc"
#undef DQ_DEC_TABLE

namespace dq {
namespace {

constexpr int kCastBlock = 256;
constexpr int kGroupsPerWave = 8;                                 // 64-row groups per wave
constexpr int kRowsPerBlock = kCastBlock * kGroupsPerWave;        // 2048
constexpr int64_t kHardCapDefault = 4096;                         // rows of the first hard list

// the bytes of one string through the aligned dwords that hold them (one dword cached: the walks are sequential)
template <typename I>
struct CastDevBytes {
  using idx = I;
  const uint32_t* words;
  I base;  // the string's first byte, from `words`
  I cur;
  uint32_t w;
  __device__ __forceinline__ uint32_t at(I i) {
    const I p = base + i;
    const I k = p >> 2;
    if (k != cur) {
      w = words[k];
      cur = k;
    }
    return (w >> (((uint32_t)p & 3u) * 8u)) & 0xFFu;
  }
};

// counters[0]: NULL rows of the result; counters[1]: hard rows (may exceed hard_cap: the caller reruns)
template <typename OffT, bool F64>
__global__ __launch_bounds__(kCastBlock) void dq_cast_kernel(const uint32_t* __restrict__ data,
                                                             const OffT* __restrict__ offsets,
                                                             const uint32_t* __restrict__ validity, int64_t n_rows,
                                                             uint64_t* __restrict__ out_values,
                                                             uint64_t* __restrict__ out_validity,
                                                             unsigned long long* counters, int64_t* hard_rows,
                                                             int64_t hard_cap) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_groups = (n_rows + 63) >> 6;
  const int64_t g0 = ((int64_t)blockIdx.x * (kCastBlock / 64) + wave) * kGroupsPerWave;
  const DecTab tab{kDecP10Lo, kDecP10Hi, kDecRcpHi, kDecRcpLo};
  uint32_t nulls = 0;  // wave-uniform
  for (int j = 0; j < kGroupsPerWave; ++j) {
    const int64_t g = g0 + j;
    if (g >= n_groups) break;
    const int64_t row = g * 64 + lane;
    const bool in = row < n_rows;
    bool valid = in;
    if (validity != nullptr && in) valid = (validity[row >> 5] >> ((uint32_t)row & 31u)) & 1u;
    uint64_t bits = 0;
    int kind = CAST_NULL;
    if (valid) {
      const OffT o0 = offsets[row], o1 = offsets[row + 1];
      if (o0 >= 0 && o1 > o0) {  // (an empty string is NULL for both targets)
        CastDevBytes<OffT> rd{data, o0, (OffT)-1, 0u};
        const OffT len = o1 - o0;
        if constexpr (F64) {
          OffT cb, ce;
          kind = cast_to_double(rd, len, tab, bits, cb, ce);
          if (kind != CAST_VALUE) bits = 0;
        } else {
          int64_t v = 0;
          kind = cast_to_long(rd, len, v) ? CAST_VALUE : CAST_NULL;
          bits = kind == CAST_VALUE ? (uint64_t)v : 0;
        }
      }
    }
    const uint64_t okm = __builtin_amdgcn_ballot_w64(kind != CAST_NULL);
    const uint64_t inm = __builtin_amdgcn_ballot_w64(in);
    if (lane == 0) out_validity[g] = okm;
    if (in) out_values[row] = bits;
    nulls += (uint32_t)__builtin_popcountll(inm & ~okm);
    if constexpr (F64) {
      const uint64_t hm = __builtin_amdgcn_ballot_w64(kind == CAST_HARD);
      if (hm != 0) {
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(&counters[1], (unsigned long long)__builtin_popcountll(hm));
        const uint32_t alo = __builtin_amdgcn_readfirstlane((uint32_t)at);
        const uint32_t ahi = __builtin_amdgcn_readfirstlane((uint32_t)(at >> 32));
        if (kind == CAST_HARD) {
          const int64_t k = (int64_t)(((uint64_t)ahi << 32) | alo) + __builtin_popcountll(hm & ((1ull << lane) - 1));
          if (k < hard_cap) hard_rows[k] = row;
        }
      }
    }
  }
  if (lane == 0 && nulls != 0) atomicAdd(&counters[0], (unsigned long long)nulls);
}

// hard tier: [start, end) of each listed row's bytes
template <typename OffT>
__global__ void dq_cast_hard_spans(const OffT* __restrict__ offsets, const int64_t* __restrict__ rows, int64_t count,
                                   int64_t* __restrict__ spans) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  spans[2 * i] = (int64_t)offsets[rows[i]];
  spans[2 * i + 1] = (int64_t)offsets[rows[i] + 1];
}
// ... their bytes packed at dst[i]
__global__ void dq_cast_hard_gather(const uint8_t* __restrict__ data, const int64_t* __restrict__ spans,
                                    const int64_t* __restrict__ dst, int64_t count, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t a = spans[2 * i], n = spans[2 * i + 1] - a;
  for (int64_t k = 0; k < n; ++k) out[dst[i] + k] = data[a + k];
}
// ... and their converted values back into the column
__global__ void dq_cast_hard_scatter(const int64_t* __restrict__ rows, const uint64_t* __restrict__ vals, int64_t count,
                                     uint64_t* __restrict__ out_values) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out_values[rows[i]] = vals[i];
}

// the exact conversion of one hard value: Java's grammar first (dq_cast.h), then strtod on the delimited text
bool hard_to_double(const uint8_t* p, int64_t n, locale_t c_loc, uint64_t& bits) {
  static const DecTab& t = dec_host_tab();
  CastHostBytes rd{p};
  int64_t cb = 0, ce = 0;
  if (cast_to_double(rd, n, t, bits, cb, ce) != CAST_HARD) return false;  // (the device said hard: a disagreement)
  const std::string text(reinterpret_cast<const char*>(p) + cb, (size_t)(ce - cb));
  char* end = nullptr;
  const double d = strtod_l(text.c_str(), &end, c_loc);
  if (end != text.c_str() + text.size()) return false;
  bits = dec_bits(d);
  return true;
}

template <typename OffT, bool F64>
void launch_cast(const dq_column_view* src, int64_t n_rows, void* out_values, uint8_t* out_validity,
                 unsigned long long* counters, int64_t* hard_rows, int64_t hard_cap, hipStream_t st) {
  const unsigned grid = (unsigned)((n_rows + kRowsPerBlock - 1) / kRowsPerBlock);
  hipLaunchKernelGGL((dq_cast_kernel<OffT, F64>), dim3(grid), dim3(kCastBlock), 0, st,
                     static_cast<const uint32_t*>(src->values), static_cast<const OffT*>(src->offsets),
                     reinterpret_cast<const uint32_t*>(src->validity), n_rows, static_cast<uint64_t*>(out_values),
                     reinterpret_cast<uint64_t*>(out_validity), counters, hard_rows, hard_cap);
}

}  // namespace
}  // namespace dq

extern "C" dq_status dq_cast_utf8(int32_t src_type, const dq_column_view* src, int64_t n_rows, int32_t to_type,
                                  void* out_values, uint8_t* out_validity, int32_t device, void* hip_stream,
                                  int64_t* null_count) {
  using namespace dq;
  if (src_type != DQ_TYPE_UTF8 && src_type != DQ_TYPE_LARGE_UTF8)
    return set_error(DQ_E_TYPE, "dq_cast_utf8: source type %d is not UTF8 / LARGE_UTF8", src_type);
  if (to_type != DQ_TYPE_I64 && to_type != DQ_TYPE_F64)
    return set_error(DQ_E_TYPE, "dq_cast_utf8: target type %d is not I64 / F64", to_type);
  if (n_rows < 0 || !src || src->reserved != 0) return set_error(DQ_E_INVALID, "dq_cast_utf8: bad argument");
  if (null_count) *null_count = 0;
  if (n_rows == 0) return DQ_OK;
  if (!src->values || !src->offsets || !out_values || !out_validity)
    return set_error(DQ_E_INVALID, "dq_cast_utf8: NULL buffer");
  if (((uintptr_t)out_values & 15) || ((uintptr_t)out_validity & 7) || ((uintptr_t)src->values & 3) ||
      ((uintptr_t)src->validity & 3))
    return set_error(DQ_E_INVALID, "dq_cast_utf8: misaligned buffer");
  if (src_type == DQ_TYPE_UTF8 && n_rows >= INT32_MAX) return set_error(DQ_E_INVALID, "dq_cast_utf8: UTF8 chunk of %lld rows", (long long)n_rows);
  const bool large = src_type == DQ_TYPE_LARGE_UTF8, f64 = to_type == DQ_TYPE_F64;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));

  int64_t hard_cap = f64 ? kHardCapDefault : 0;
  if (const char* e = std::getenv("DQ_CAST_HARD_CAP"))  // the first list's capacity (tests force the rerun with it)
    if (f64 && std::atoll(e) > 0) hard_cap = std::atoll(e);
  DevPtr<unsigned long long> counters;
  DevPtr<int64_t> hard;
  DQ_HIP(counters.alloc(2));
  unsigned long long h_counters[2] = {0, 0};
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (f64) DQ_HIP(hard.alloc((size_t)hard_cap));
    DQ_HIP(hipMemsetAsync(counters.get(), 0, 16, st));
    auto* dc = counters.get();
    auto* dh = hard.get();
    if (large) {
      if (f64) launch_cast<int64_t, true>(src, n_rows, out_values, out_validity, dc, dh, hard_cap, st);
      else launch_cast<int64_t, false>(src, n_rows, out_values, out_validity, dc, dh, hard_cap, st);
    } else {
      if (f64) launch_cast<int32_t, true>(src, n_rows, out_values, out_validity, dc, dh, hard_cap, st);
      else launch_cast<int32_t, false>(src, n_rows, out_values, out_validity, dc, dh, hard_cap, st);
    }
    DQ_HIP(hipGetLastError());
    DQ_HIP(hipMemcpyAsync(h_counters, counters.get(), 16, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
    if ((int64_t)h_counters[1] <= hard_cap) break;
    if (attempt == 1) return set_error(DQ_E_HIP, "dq_cast_utf8: hard-row count changed between runs");
    // the list overflowed: size it for the reported count and cast again
    hard_cap = (int64_t)h_counters[1];
    hard.reset();
  }
  if (null_count) *null_count = (int64_t)h_counters[0];
  const int64_t nh = (int64_t)h_counters[1];
  if (nh == 0) return DQ_OK;

  // hard tier: gather the rows' bytes, convert on the host, scatter the values
  const unsigned hgrid = (unsigned)((nh + 255) / 256);
  DevPtr<int64_t> spans, dst;
  DevPtr<uint8_t> bytes;
  DevPtr<uint64_t> vals;
  DQ_HIP(spans.alloc((size_t)nh * 2));
  if (large) hipLaunchKernelGGL(dq_cast_hard_spans<int64_t>, dim3(hgrid), dim3(256), 0, st, static_cast<const int64_t*>(src->offsets), hard.get(), nh, spans.get());
  else hipLaunchKernelGGL(dq_cast_hard_spans<int32_t>, dim3(hgrid), dim3(256), 0, st, static_cast<const int32_t*>(src->offsets), hard.get(), nh, spans.get());
  DQ_HIP(hipGetLastError());
  std::vector<int64_t> h_spans((size_t)nh * 2), h_dst((size_t)nh);
  DQ_HIP(hipMemcpyAsync(h_spans.data(), spans.get(), (size_t)nh * 16, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  int64_t total = 0;
  for (int64_t i = 0; i < nh; ++i) {
    h_dst[(size_t)i] = total;
    total += h_spans[(size_t)(2 * i + 1)] - h_spans[(size_t)(2 * i)];
  }
  DQ_HIP(dst.alloc((size_t)nh));
  DQ_HIP(bytes.alloc((size_t)total));
  DQ_HIP(hipMemcpyAsync(dst.get(), h_dst.data(), (size_t)nh * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dq_cast_hard_gather, dim3(hgrid), dim3(256), 0, st, static_cast<const uint8_t*>(src->values),
                     spans.get(), dst.get(), nh, bytes.get());
  DQ_HIP(hipGetLastError());
  std::vector<uint8_t> h_bytes((size_t)total);
  DQ_HIP(hipMemcpyAsync(h_bytes.data(), bytes.get(), (size_t)total, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  std::vector<uint64_t> h_vals((size_t)nh);
  locale_t c_loc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
  if (c_loc == (locale_t)0) return set_error(DQ_E_INVALID, "dq_cast_utf8: newlocale(\"C\") failed");
  bool ok = true;
  for (int64_t i = 0; i < nh && ok; ++i)
    ok = hard_to_double(h_bytes.data() + h_dst[(size_t)i], h_spans[(size_t)(2 * i + 1)] - h_spans[(size_t)(2 * i)], c_loc,
                        h_vals[(size_t)i]);
  freelocale(c_loc);
  if (!ok) return set_error(DQ_E_HIP, "dq_cast_utf8: host and device disagree on a hard row");
  DQ_HIP(vals.alloc((size_t)nh));
  DQ_HIP(hipMemcpyAsync(vals.get(), h_vals.data(), (size_t)nh * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dq_cast_hard_scatter, dim3(hgrid), dim3(256), 0, st, hard.get(), vals.get(), nh, static_cast<uint64_t*>(out_values));
  DQ_HIP(hipGetLastError());
  DQ_HIP(hipStreamSynchronize(st));
  return DQ_OK;
}
