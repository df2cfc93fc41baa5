// dq_bin.hip -- a numeric column counted into declared bins (Histogram's `binning`) on gfx950.
//
//   dq_bins_create   k + 1 finite, strictly increasing binary64 edges (1 <= k <= 4096), checked on the host and kept
//                    on the device.
//   dq_bin_count     counts[slot] += rows of that slot, slots [below, bin 0 .. bin k-1, above, nan].  A value is
//                    converted to binary64 as Spark's cast does (f32 widens exactly, integers round to nearest-even,
//                    a decimal through dec_to_double) and its slot comes from comparisons against the stored edges
//                    alone:  e[i] <= x < e[i+1] -> bin i;  x == e[k] -> the last bin (closed on the right);
//                    x < e[0], -inf included -> below;  x > e[k], +inf included -> above;  NaN -> nan.  -0.0 compares as
//                    0.0; a NULL row is in no slot.
//
// The frequency table is dq_freq_build_weighted over the k + 3 labels with these counts as weights.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <type_traits>

#include "dq_decimal.h"
#include "dq_device.h"
#include "dq_hip_host.h"
#include "dq_lane.h"

struct dq_bins {
  int32_t n_edges = 0;
  int32_t device = 0;
  int32_t guess = 0;  // the evenly-spaced first guess is within one bin of the truth for every value (checked)
  double inv = 0.0;   // k / (e[k] - e[0])
  dq::DevPtr<double> edges;
};

namespace dq {

constexpr int32_t kBinMaxBins = 4096;
constexpr int32_t kBinCountMaxWG = 2048;  // row ranges per launch (dq_dict_count's)

// LDS of a workgroup: the k + 1 edges (8 bytes each) and k + 3 uint32 counters -- 12 k + 20 bytes, sized per launch.
// k = 4096: 49172 bytes, three workgroups (12 waves) on a CU's 160 KB; k <= 1000: all eight workgroups of the CU's 32
// waves.  (Counters in 16 bits would not hold a range; edges in 32 bits would not be the stored edges.)
inline size_t bin_lds_bytes(int32_t k) { return (size_t)(k + 1) * 8 + (size_t)(k + 3) * 4; }

// The first guess of an in-range value's bin, for evenly spaced edges: truncation of (x - e0) inv, clamped.  The same
// two operations in the same order on host and device (a subtraction and a multiplication: nothing to contract).
__host__ __device__ __forceinline__ int32_t bin_guess(double x, double e0, double inv, int32_t k) {
  double t = (x - e0) * inv;
  t = t < (double)(k - 1) ? t : (double)(k - 1);  // (NaN -> k - 1 -> corrected like any guess)
  t = t > 0.0 ? t : 0.0;
  return (int32_t)t;
}

#define DQ_DEC_TABLE static __constant__ const
#include "dq_dec_tables.inc"
#undef DQ_DEC_TABLE

// row r of a column of TYPE as binary64 (Spark's Cast(child, DoubleType))
template <int TYPE>
__device__ __forceinline__ double bin_load(const void* __restrict__ values, int64_t r, int32_t scale, bool narrow) {
  if constexpr (TYPE == DQ_TYPE_F64) return __builtin_nontemporal_load(static_cast<const double*>(values) + r);
  else if constexpr (TYPE == DQ_TYPE_F32) return (double)__builtin_nontemporal_load(static_cast<const float*>(values) + r);
  else if constexpr (TYPE == DQ_TYPE_I64) return (double)__builtin_nontemporal_load(static_cast<const int64_t*>(values) + r);
  else if constexpr (TYPE == DQ_TYPE_I32) return (double)__builtin_nontemporal_load(static_cast<const int32_t*>(values) + r);
  else if constexpr (TYPE == DQ_TYPE_I16) return (double)__builtin_nontemporal_load(static_cast<const int16_t*>(values) + r);
  else if constexpr (TYPE == DQ_TYPE_I8) return (double)__builtin_nontemporal_load(static_cast<const int8_t*>(values) + r);
  else {
    const DecTab tab{kDecP10Lo, kDecP10Hi, kDecRcpHi, kDecRcpLo};
    const uint64_t* v = static_cast<const uint64_t*>(values) + 2 * r;
    return dec_to_double(__builtin_nontemporal_load(v), __builtin_nontemporal_load(v + 1), scale, tab, narrow);
  }
}

// the slot of x among [below, bin 0 .. bin k-1, above, nan]: comparisons against the edges in LDS only
__device__ __forceinline__ uint32_t bin_slot(double x, const double* e, int32_t k, bool guess, double inv) {
  if (x != x) return (uint32_t)k + 2u;
  if (x < e[0]) return 0u;
  if (x >= e[k]) return x == e[k] ? (uint32_t)k : (uint32_t)k + 1u;
  // e[0] <= x < e[k]: the largest i with e[i] <= x
  if (guess) {
    // the guess is at most one bin off (dq_bins_create checked both ends of every bin, and it is monotone in x), so
    // one compare against each neighbouring edge settles it; g - 1 >= 0 and g + 1 <= k - 1 follow from the range
    int32_t g = bin_guess(x, e[0], inv, k);
    if (x < e[g]) --g;
    else if (x >= e[g + 1]) ++g;
    return (uint32_t)g + 1u;
  }
  int32_t lo = 0, hi = k;  // e[lo] <= x < e[hi]
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (e[mid] <= x) lo = mid;
    else hi = mid;
  }
  return (uint32_t)lo + 1u;
}

// Workgroup b counts rows [b rows_per_range, (b + 1) rows_per_range) as dq_dict_count_kernel<true> does: lane l of a
// wave takes row base + 64 j + l, a 64-row group's validity is one scalar word, the counters are workgroup-private
// uint32 words in LDS (a range is below 2^31 rows: they cannot wrap) and each non-zero one is added to counts[] once,
// with one 64-bit global add, at the end.  Before the LDS add the lanes that share the slot of the group's first
// selected row are combined into one add of their number: a column that falls into one bin costs one LDS add per
// group, not 64 adds to one address; the other lanes add 1 each.
// SEL: `mask` is the selection bitmap -- a group's word is validity & mask -- and the selected rows (NULL ones too)
// are counted per wave and added to *n_selected (when wanted) with one global add per wave at the end.
template <int TYPE, bool SEL>
__global__ __launch_bounds__(kBlock) void dq_bin_count_kernel(const void* __restrict__ values, const uint32_t* validity,
                                                              const uint32_t* mask,
                                                              unsigned long long* __restrict__ n_selected,
                                                              const double* __restrict__ gedges, int32_t k,
                                                              int32_t guess, double inv, int32_t scale, int32_t narrow,
                                                              int64_t n_rows, int64_t rows_per_range,
                                                              unsigned long long* __restrict__ counts) {
  extern __shared__ double bin_lds[];
  double* const edges = bin_lds;                                      // k + 1
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(bin_lds + k + 1);  // k + 3
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_range;
  int64_t row1 = row0 + rows_per_range;
  if (row1 > n_rows) row1 = n_rows;
  for (int32_t i = threadIdx.x; i <= k; i += kBlock) edges[i] = gedges[i];
  for (int32_t i = threadIdx.x; i < k + 3; i += kBlock) cnt[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t nr = (int32_t)(row1 - row0);
  uint32_t nsel = 0;  // SEL: this wave's selected rows (wave-uniform; a range is below 2^31 rows)
  for (int32_t rb = wave * 512; rb < nr; rb += kRowsPerIter) {
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
      const int32_t left = nr - rb - 64 * j;  // rows of this group below row1
      if (left <= 0) break;
      const int64_t gbase = row0 + rb + 64 * j;
      uint64_t m;
      if constexpr (SEL) {
        const uint64_t s = sel_word(mask, gbase >> 5, left);
        nsel += (uint32_t)__builtin_popcountll(s);
        if (s == 0) continue;
        m = s & sel_word(validity, gbase >> 5, left);
      } else {
        m = sel_word(validity, gbase >> 5, left);
      }
      if (m == 0) continue;
      const bool sel = lane_bit(m);
      uint32_t slot = 0;
      if (sel) slot = bin_slot(bin_load<TYPE>(values, gbase + lane, scale, narrow != 0), edges, k, guess != 0, inv);
      const int lead = __builtin_ctzll(m);  // (wave-uniform: m is)
      const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)slot, lead);
      const uint64_t same = __builtin_amdgcn_ballot_w64(sel && slot == first);
      if (lane == lead) atomicAdd(&cnt[first], (uint32_t)__builtin_popcountll(same));
      else if (sel && slot != first) atomicAdd(&cnt[slot], 1u);
    }
  }
  __syncthreads();
  for (int32_t s = threadIdx.x; s < k + 3; s += kBlock) {
    const uint32_t c = cnt[s];
    if (c) atomicAdd(&counts[s], (unsigned long long)c);
  }
  if constexpr (SEL) {
    if (n_selected && lane == 0 && nsel) atomicAdd(n_selected, (unsigned long long)nsel);
  }
}

__global__ void bin_add_rows(unsigned long long* __restrict__ n_selected, unsigned long long n) {
  atomicAdd(n_selected, n);
}

const char* bin_type_name(int32_t type) {
  switch (type) {
    case DQ_TYPE_UTF8: return "UTF8";
    case DQ_TYPE_LARGE_UTF8: return "LARGE_UTF8";
    case DQ_TYPE_BOOL: return "BOOL";
    case DQ_TYPE_DATE32: return "DATE32";
    case DQ_TYPE_TIMESTAMP: return "TIMESTAMP";
    case DQ_TYPE_DICT_UTF8: return "DICT_UTF8";
    default: return "unknown";
  }
}

}  // namespace dq

extern "C" {

dq_status dq_bins_create(const double* edges, int32_t n_edges, int32_t device, dq_bins** out) {
  using namespace dq;
  const char* me = "dq_bins_create";
  if (!out) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  *out = nullptr;
  if (!edges || n_edges < 2) return set_error(DQ_E_INVALID, "%s: at least 2 edges (1 bin) are needed", me);
  if (n_edges - 1 > kBinMaxBins)
    return set_error(DQ_E_UNSUPPORTED, "%s: %d bins, at most %d", me, n_edges - 1, kBinMaxBins);
  for (int32_t i = 0; i < n_edges; ++i) {
    if (!std::isfinite(edges[i])) return set_error(DQ_E_INVALID, "%s: edges[%d] is not finite", me, i);
    if (i > 0 && !(edges[i] > edges[i - 1]))
      return set_error(DQ_E_INVALID, "%s: edges[%d] is not greater than edges[%d]", me, i, i - 1);
  }
  dq_bins* b = new (std::nothrow) dq_bins;
  if (!b) return set_error(DQ_E_OOM, "%s: out of host memory", me);
  b->n_edges = n_edges;
  b->device = device;
  // the first guess is used when it lands within one bin of the truth at both ends of every bin (it is monotone in
  // x, so then it does for every value in between)
  const int32_t k = n_edges - 1;
  const double span = edges[k] - edges[0];
  if (std::isfinite(span)) {
    const double inv = (double)k / span;
    bool ok = std::isfinite(inv);
    for (int32_t i = 0; i < k && ok; ++i) {
      const int32_t g0 = bin_guess(edges[i], edges[0], inv, k);
      const int32_t g1 = bin_guess(std::nextafter(edges[i + 1], edges[i]), edges[0], inv, k);
      ok = g0 >= i - 1 && g0 <= i + 1 && g1 >= i - 1 && g1 <= i + 1;
    }
    b->guess = ok ? 1 : 0;
    b->inv = ok ? inv : 0.0;
  }
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = b->edges.alloc((size_t)n_edges);
  if (e == hipSuccess) e = hipMemcpy(b->edges.get(), edges, (size_t)n_edges * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete b;
    return set_error(e == hipErrorOutOfMemory ? DQ_E_OOM : DQ_E_HIP, "%s: %s", me, hipGetErrorString(e));
  }
  *out = b;
  return DQ_OK;
}

void dq_bins_destroy(dq_bins* bins) { delete bins; }

static dq_status bin_count_impl(const char* me, const dq_bins* bins, int32_t type, const dq_column_view* col,
                                int64_t n_rows, const uint64_t* selection, int64_t* counts, int64_t* n_selected,
                                int32_t device, void* hip_stream) {
  using namespace dq;
  if (((uintptr_t)selection & 7) || ((uintptr_t)n_selected & 7))
    return set_error(DQ_E_INVALID, "%s: the selection / n_selected is not 8-byte aligned", me);
  if (!bins) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  const int32_t base = type_valid(type) || type == DQ_TYPE_DICT_UTF8 ? DQ_TYPE_BASE(type) : 0;
  int32_t width = 0;
  switch (base) {
    case DQ_TYPE_F64: case DQ_TYPE_I64: width = 8; break;
    case DQ_TYPE_F32: case DQ_TYPE_I32: width = 4; break;
    case DQ_TYPE_I16: width = 2; break;
    case DQ_TYPE_I8: width = 1; break;
    case DQ_TYPE_DECIMAL128: width = 8; break;  // (two 8-byte loads per value)
    default:
      return set_error(DQ_E_UNSUPPORTED, "%s: column type %d (%s) has no bins: F64 / F32 / I64 / I32 / I16 / I8 / "
                       "DECIMAL128 only", me, type, bin_type_name(type));
  }
  if (!col || col->reserved != 0 || n_rows < 0 || device != bins->device)
    return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (n_rows > INT32_MAX) return set_error(DQ_E_UNSUPPORTED, "%s: at most 2^31 - 1 rows per call", me);
  if (n_rows == 0) return DQ_OK;
  if (!col->values || !counts) return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
  if (((uintptr_t)col->values & (uintptr_t)(width - 1)) || ((uintptr_t)col->validity & 3) || ((uintptr_t)counts & 7))
    return set_error(DQ_E_INVALID, "%s: misaligned buffer", me);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  // row ranges: whole kRowsPerIter blocks, at most kBinCountMaxWG of them
  const int64_t blocks = (n_rows + kRowsPerIter - 1) / kRowsPerIter;
  const int64_t rows_per_range = (blocks + kBinCountMaxWG - 1) / kBinCountMaxWG * kRowsPerIter;
  const unsigned grid = (unsigned)((n_rows + rows_per_range - 1) / rows_per_range);
  const int32_t k = bins->n_edges - 1;
  const int32_t scale = base == DQ_TYPE_DECIMAL128 ? DQ_DECIMAL_SCALE(type) : 0;
  const int32_t narrow = base == DQ_TYPE_DECIMAL128 && DQ_DECIMAL_PRECISION(type) <= 18;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), bin_lds_bytes(k), st, col->values,
                       reinterpret_cast<const uint32_t*>(col->validity), reinterpret_cast<const uint32_t*>(selection),
                       reinterpret_cast<unsigned long long*>(n_selected), bins->edges.get(), k, bins->guess, bins->inv,
                       scale, narrow, n_rows, rows_per_range, reinterpret_cast<unsigned long long*>(counts));
  };
  auto launch_type = [&](auto filtered) {
    constexpr bool F = decltype(filtered)::value;
    switch (base) {
      case DQ_TYPE_F64: launch(dq_bin_count_kernel<DQ_TYPE_F64, F>); break;
      case DQ_TYPE_F32: launch(dq_bin_count_kernel<DQ_TYPE_F32, F>); break;
      case DQ_TYPE_I64: launch(dq_bin_count_kernel<DQ_TYPE_I64, F>); break;
      case DQ_TYPE_I32: launch(dq_bin_count_kernel<DQ_TYPE_I32, F>); break;
      case DQ_TYPE_I16: launch(dq_bin_count_kernel<DQ_TYPE_I16, F>); break;
      case DQ_TYPE_I8: launch(dq_bin_count_kernel<DQ_TYPE_I8, F>); break;
      default: launch(dq_bin_count_kernel<DQ_TYPE_DECIMAL128, F>); break;
    }
  };
  if (selection) {
    launch_type(std::true_type{});
  } else {
    launch_type(std::false_type{});
    if (n_selected) {  // every row is selected
      hipLaunchKernelGGL(bin_add_rows, dim3(1), dim3(1), 0, st, reinterpret_cast<unsigned long long*>(n_selected),
                         (unsigned long long)n_rows);
    }
  }
  DQ_HIP(hipGetLastError());
  return DQ_OK;
}

dq_status dq_bin_count(const dq_bins* bins, int32_t type, const dq_column_view* col, int64_t n_rows, int64_t* counts,
                       int32_t device, void* hip_stream) {
  return bin_count_impl("dq_bin_count", bins, type, col, n_rows, nullptr, counts, nullptr, device, hip_stream);
}

dq_status dq_bin_count_where(const dq_bins* bins, int32_t type, const dq_column_view* col, int64_t n_rows,
                             const uint64_t* selection, int64_t* counts, int64_t* n_selected, int32_t device,
                             void* hip_stream) {
  return bin_count_impl("dq_bin_count_where", bins, type, col, n_rows, selection, counts, n_selected, device, hip_stream);
}

}  // extern "C"
