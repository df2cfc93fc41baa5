// dq_dist.hip -- distances between two frequency tables on the GPU: distribution drift.
//
// dq_freq_distance joins two self-contained frequency tables a and b (dq_group.hip builds them; dq_freq_table.h holds
// them) by group and reduces the join to L-infinity, total variation and Jensen-Shannon distances between the two
// relative-frequency distributions, the sizes of the join's three parts and the group that attains L-infinity.
// dq_freq_ks is the exact two-sample Kolmogorov-Smirnov statistic of two unhashed single-column tables.  These
// semantics are this project's (include/dqscan.h states them); tests/test_drift_gpu.py pins them.
//
// The join: both tables keep their groups' keys ascending as unsigned 64-bit words, so one thread per group of a
// binary-searches b's keys; a hashed table's hit is a hit only when the stored tuples are equal by value
// (tuple_equal_rows: dq_freq_contains_rows' comparison), so two tuples under one hash are two groups, one on each side.
// A second sweep, b's groups against a's keys, takes the groups a lacks.  Both sweeps are one launch over
// G_a + G_b items.
//
// Reproducible bits: binary64 throughout, compiled with contraction off (the Makefile), IEEE division, no
// floating-point atomics.  A thread sums its items in index order, a wave sums its lanes with dq_lane.h's fixed
// butterfly, a workgroup its four waves in wave order, and one final wave sums the workgroups' partials in a fixed
// order; the grid is a function of the group counts alone.  L-infinity is a maximum under a total order (the
// difference, then the smaller key word, then side a), which no reduction order changes.  KS reduces a maximum of
// non-negative doubles, taken as an integer maximum of their bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "dq_freq_table.h"
#include "dq_lane.h"
#include "dq_prim.h"

namespace dq {
namespace {

constexpr int kDistThreads = 256;   // groups per workgroup and grid-loop step
constexpr int kDistMaxGrid = 1024;  // workgroups at most: the partials the final pass merges

// what a thread, a wave, a workgroup or the whole launch has accumulated (tv / js before their factor 1/2)
struct DistPart {
  double tv, js, linf;  // linf < 0: no group seen yet
  uint64_t key;
  int64_t n_common, n_only_a, n_only_b, count_only_a, count_only_b;
  int32_t side, pad;
};

__device__ __forceinline__ DistPart dist_zero() {
  DistPart z;
  z.tv = 0.0, z.js = 0.0, z.linf = -1.0;
  z.key = ~0ull;
  z.n_common = z.n_only_a = z.n_only_b = z.count_only_a = z.count_only_b = 0;
  z.side = 1, z.pad = 0;
  return z;
}

// (d, k, s) comes before (d0, k0, s0) as the group attaining L-infinity: the larger difference, then the smaller
// unsigned key word, then side a (0)
__device__ __forceinline__ bool linf_before(double d, uint64_t k, int32_t s, double d0, uint64_t k0, int32_t s0) {
  return d > d0 || (d == d0 && (k < k0 || (k == k0 && s < s0)));
}

__device__ __forceinline__ void dist_add(DistPart& t, const DistPart& o) {
  t.tv += o.tv, t.js += o.js;
  t.n_common += o.n_common, t.n_only_a += o.n_only_a, t.n_only_b += o.n_only_b;
  t.count_only_a += o.count_only_a, t.count_only_b += o.count_only_b;
  if (linf_before(o.linf, o.key, o.side, t.linf, t.key, t.side)) t.linf = o.linf, t.key = o.key, t.side = o.side;
}

// every lane ends with the wave's DistPart: the sums by dq_lane.h's butterflies, the maximum by the same butterfly
__device__ __forceinline__ DistPart dist_wave(DistPart t) {
  t.tv = wave_sum_f64(t.tv), t.js = wave_sum_f64(t.js);
  t.n_common = wave_sum_i64(t.n_common), t.n_only_a = wave_sum_i64(t.n_only_a), t.n_only_b = wave_sum_i64(t.n_only_b);
  t.count_only_a = wave_sum_i64(t.count_only_a), t.count_only_b = wave_sum_i64(t.count_only_b);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double d = __shfl_xor(t.linf, m);
    const uint64_t k = (uint64_t)__shfl_xor((unsigned long long)t.key, m);
    const int32_t s = __shfl_xor(t.side, m);
    if (linf_before(d, k, s, t.linf, t.key, t.side)) t.linf = d, t.key = k, t.side = s;
  }
  return t;
}

// the index of k among keys[0 .. G) (ascending, distinct), or -1
__device__ __forceinline__ int64_t find_key(const uint64_t* __restrict__ keys, int64_t G, uint64_t k) {
  int64_t lo = 0, hi = G;  // the first index whose key is >= k lies in [lo, hi]
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo < G && keys[lo] == k ? lo : -1;
}

// one term of 2 * JS: p ln(p / m) + q ln(q / m) with m = (p + q) / 2, a zero probability contributing 0
__device__ __forceinline__ double js_term(double p, double q) {
  const double m = (p + q) / 2.0;
  double t = 0.0;
  if (p > 0.0) t += p * log(p / m);
  if (q > 0.0) t += q * log(q / m);
  return t;
}

// Item i < GA is group i of a, looked up in b; item GA + j is group j of b, looked up in a and counted only when a
// lacks it.  sa / sb: the tables' value stores (HASHED).  part[blockIdx.x] = the workgroup's DistPart.
template <bool HASHED>
__global__ __launch_bounds__(kDistThreads) void freq_distance_part(
    const uint64_t* __restrict__ keys_a, const int64_t* __restrict__ counts_a, int64_t GA, double NA,
    const uint64_t* __restrict__ keys_b, const int64_t* __restrict__ counts_b, int64_t GB, double NB, GroupCols sa,
    GroupCols sb, DistPart* __restrict__ part) {
  __shared__ DistPart sw[kDistThreads / 64];
  DistPart t = dist_zero();
  const int64_t total = GA + GB;
  for (int64_t i = (int64_t)blockIdx.x * kDistThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kDistThreads) {
    const bool of_a = i < GA;
    const int64_t g = of_a ? i : i - GA;
    const uint64_t k = of_a ? keys_a[g] : keys_b[g];
    int64_t o = of_a ? find_key(keys_b, GB, k) : find_key(keys_a, GA, k);
    if constexpr (HASHED) {  // an equal hash is the same group only with an equal tuple
      if (o >= 0 && !(of_a ? tuple_equal_rows(sa, sb, g, o) : tuple_equal_rows(sa, sb, o, g))) o = -1;
    }
    if (!of_a && o >= 0) continue;  // a common group: the first sweep took it
    const int64_t c = of_a ? counts_a[g] : counts_b[g];
    double p = 0.0, q = 0.0;
    if (of_a) {
      p = (double)c / NA;
      if (o >= 0) {
        q = (double)counts_b[o] / NB;
        ++t.n_common;
      } else {
        ++t.n_only_a;
        t.count_only_a += c;
      }
    } else {
      q = (double)c / NB;
      ++t.n_only_b;
      t.count_only_b += c;
    }
    const double d = fabs(p - q);
    t.tv += d;
    t.js += js_term(p, q);
    const int32_t side = of_a ? 0 : 1;
    if (linf_before(d, k, side, t.linf, t.key, t.side)) t.linf = d, t.key = k, t.side = side;
  }
  t = dist_wave(t);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    DistPart w = sw[0];
    for (int i = 1; i < kDistThreads / 64; ++i) dist_add(w, sw[i]);
    part[blockIdx.x] = w;
  }
}

// one wave: lane l sums partials l, l + 64, ... in that order, the wave sums its lanes
__global__ __launch_bounds__(64) void freq_distance_final(const DistPart* __restrict__ part, int nparts,
                                                          DistPart* __restrict__ out) {
  DistPart t = dist_zero();
  for (int i = threadIdx.x; i < nparts; i += 64) dist_add(t, part[i]);
  t = dist_wave(t);
  if (threadIdx.x == 0) *out = t;
}

// ---- Kolmogorov-Smirnov ---------------------------------------------------------------------------------------------
// A table's keys ascend as unsigned words: the values with a clear sign bit first, ascending, then those with the sign
// bit set -- negative integers ascending, negative floats by ascending magnitude, i.e. descending.  ks_order writes the
// table in the values' order without a sort: position o of the order reads one fixed position of the table.
enum KsKind { kKsInt = 0, kKsF64 = 1, kKsF32 = 2 };

// an order-preserving word of a key: integers and dates numerically; floats numerically with -0.0 immediately below
// 0.0 and the canonical NaN (sign clear) above +inf
__device__ __forceinline__ uint64_t ks_word(int kind, uint64_t k) {
  if (kind == kKsInt) return k ^ (1ull << 63);
  if (kind == kKsF64) return (k >> 63) ? ~k : (k | (1ull << 63));
  return (k & 0x80000000ull) ? (~k & 0xFFFFFFFFull) : (k | 0x80000000ull);  // f32: the bits zero-extended
}

// ordered[o] / count[o] = the o-th smallest value's word and count; count[G] = 0 (the scan's last slot)
__global__ __launch_bounds__(256) void ks_order(const uint64_t* __restrict__ keys, const int64_t* __restrict__ counts,
                                                int64_t G, int kind, uint64_t* __restrict__ ordered,
                                                int64_t* __restrict__ count) {
  __shared__ int64_t s_pos;  // the number of keys with a clear sign bit
  if (threadIdx.x == 0) {
    const uint64_t sign = kind == kKsF32 ? 0x80000000ull : (1ull << 63);
    int64_t lo = 0, hi = G;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < sign) lo = mid + 1;
      else hi = mid;
    }
    s_pos = lo;
  }
  __syncthreads();
  const int64_t P = s_pos, neg = G - P;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o <= G; o += (int64_t)gridDim.x * 256) {
    if (o == G) {
      count[G] = 0;
      continue;
    }
    const int64_t at = o >= neg ? o - neg : (kind == kKsInt ? P + o : G - 1 - o);
    ordered[o] = ks_word(kind, keys[at]);
    count[o] = counts[at];
  }
}

// the number of words[0 .. G) that are <= x (ascending)
__device__ __forceinline__ int64_t count_le(const uint64_t* __restrict__ words, int64_t G, uint64_t x) {
  int64_t lo = 0, hi = G;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (words[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// cum_x[i] = the counts of x's i smallest values (cum_x[G] = N_x).  Every value of either table is a point:
// |F_a - F_b| there, F = an exact cumulative count divided once.  *out_bits = the maximum's bits (zeroed by the caller;
// the differences are non-negative, so their order is their bits' order as integers).
__global__ __launch_bounds__(256) void ks_points(const uint64_t* __restrict__ wa, const int64_t* __restrict__ cum_a,
                                                 int64_t GA, double NA, const uint64_t* __restrict__ wb,
                                                 const int64_t* __restrict__ cum_b, int64_t GB, double NB,
                                                 unsigned long long* __restrict__ out_bits) {
  double best = 0.0;
  const int64_t total = GA + GB;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const bool of_a = i < GA;
    const int64_t o = of_a ? i : i - GA;
    const uint64_t x = of_a ? wa[o] : wb[o];
    const int64_t ca = of_a ? cum_a[o + 1] : cum_a[count_le(wa, GA, x)];
    const int64_t cb = of_a ? cum_b[count_le(wb, GB, x)] : cum_b[o + 1];
    const double d = fabs((double)ca / NA - (double)cb / NB);
    best = d > best ? d : best;
  }
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0) atomicMax(out_bits, (unsigned long long)__builtin_bit_cast(uint64_t, best));
}

bool is_str_code(int32_t ty) { return ty == DQ_TYPE_UTF8 || ty == DQ_TYPE_LARGE_UTF8; }

int dist_grid(int64_t items) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(kDistMaxGrid, (items + kDistThreads - 1) / kDistThreads));
}

}  // namespace
}  // namespace dq

using namespace dq;

extern "C" {

dq_status dq_freq_distance(const dq_freq_table* a, const dq_freq_table* b, void* hip_stream,
                           dq_freq_distance_result* out) {
  const char* me = "dq_freq_distance";
  // everything the arguments and the tables say, before anything touches the device
  if (!out) return set_error(DQ_E_INVALID, "%s: out is NULL", me);
  if (!a || !b) return set_error(DQ_E_INVALID, "%s: table is NULL", me);
  std::memset(out, 0, sizeof(*out));
  for (const dq_freq_table* t : {a, b})
    if (t->hashed && !t->has_store)
      return set_error(DQ_E_STATE, "%s: table %s does not own its values (dq_freq_materialize it first): groups of "
                                   "equal hash are compared by their stored tuples", me, t == a ? "a" : "b");
  if (a->types.size() != b->types.size())
    return set_error(DQ_E_INVALID, "%s: table a has %zu columns, table b has %zu", me, a->types.size(), b->types.size());
  for (size_t c = 0; c < a->types.size(); ++c)
    // the same type (a decimal's precision and scale are part of its code), or two string columns; nothing is widened
    if (a->types[c] != b->types[c] && !(is_str_code(a->types[c]) && is_str_code(b->types[c])))
      return set_error(DQ_E_INVALID, "%s: column %zu has type %d in table a, %d in table b", me, c, a->types[c],
                       b->types[c]);
  if (a->hashed != b->hashed) return set_error(DQ_E_INVALID, "%s: a hashed and an unhashed table", me);
  if (a->device != b->device)
    return set_error(DQ_E_INVALID, "%s: table a is on device %d, table b on device %d", me, a->device, b->device);
  if (a->n_values == 0 || b->n_values == 0) return DQ_OK;  // defined = 0: an empty side has no distribution
  DQ_HIP(hipSetDevice(a->device));
  const hipStream_t S = reinterpret_cast<hipStream_t>(hip_stream);
  GroupCols sa, sb;
  std::memset(&sa, 0, sizeof(sa));
  std::memset(&sb, 0, sizeof(sb));
  if (a->hashed) sa = store_cols(a), sb = store_cols(b);
  Frame fr(group_arena(), a->device);
  const int grid = dist_grid(a->n_groups + b->n_groups);
  DistPart *d_part = nullptr, *d_out = nullptr;
  if (dq_status s = take(fr, d_part, grid)) return s;
  if (dq_status s = take(fr, d_out, 1)) return s;
  const double NA = (double)a->n_values, NB = (double)b->n_values;
  if (a->hashed)
    hipLaunchKernelGGL(freq_distance_part<true>, dim3(grid), dim3(kDistThreads), 0, S, a->d_keys.get(),
                       a->d_counts.get(), a->n_groups, NA, b->d_keys.get(), b->d_counts.get(), b->n_groups, NB, sa, sb,
                       d_part);
  else
    hipLaunchKernelGGL(freq_distance_part<false>, dim3(grid), dim3(kDistThreads), 0, S, a->d_keys.get(),
                       a->d_counts.get(), a->n_groups, NA, b->d_keys.get(), b->d_counts.get(), b->n_groups, NB, sa, sb,
                       d_part);
  DQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(freq_distance_final, dim3(1), dim3(64), 0, S, d_part, grid, d_out);
  DQ_HIP(hipGetLastError());
  DistPart h;
  if (dq_status s = read_back(&h, d_out, S)) return s;
  out->defined = 1;
  out->linf = h.linf;
  out->tv = 0.5 * h.tv;
  out->js = std::min(std::max(0.5 * h.js, 0.0), 0.6931471805599453);  // [0, ln 2]: the roundings' last bits clipped
  out->linf_key = h.key;
  out->linf_side = h.side;
  out->n_common = h.n_common, out->n_only_a = h.n_only_a, out->n_only_b = h.n_only_b;
  out->count_only_a = h.count_only_a, out->count_only_b = h.count_only_b;
  return DQ_OK;
}

dq_status dq_freq_ks(const dq_freq_table* a, const dq_freq_table* b, void* hip_stream, double* ks, int32_t* defined) {
  const char* me = "dq_freq_ks";
  if (!ks || !defined) return set_error(DQ_E_INVALID, "%s: ks / defined is NULL", me);
  if (!a || !b) return set_error(DQ_E_INVALID, "%s: table is NULL", me);
  *ks = 0.0;
  *defined = 0;
  int kind[2] = {0, 0};
  int at = 0;
  for (const dq_freq_table* t : {a, b}) {
    if (t->hashed || t->types.size() != 1)
      return set_error(DQ_E_UNSUPPORTED, "%s: table %s is hashed (strings, decimals, several columns): the statistic "
                                         "needs one ordered fixed-width column", me, t == a ? "a" : "b");
    switch (t->types[0]) {
      case DQ_TYPE_F64: kind[at] = kKsF64; break;
      case DQ_TYPE_F32: kind[at] = kKsF32; break;
      case DQ_TYPE_I64: case DQ_TYPE_I32: case DQ_TYPE_I16: case DQ_TYPE_I8: case DQ_TYPE_DATE32:
      case DQ_TYPE_TIMESTAMP: kind[at] = kKsInt; break;
      default:
        return set_error(DQ_E_UNSUPPORTED, "%s: table %s has column type %d, which has no order here", me,
                         t == a ? "a" : "b", t->types[0]);
    }
    ++at;
  }
  if (a->types[0] != b->types[0])
    return set_error(DQ_E_INVALID, "%s: column 0 has type %d in table a, %d in table b", me, a->types[0], b->types[0]);
  if (a->device != b->device)
    return set_error(DQ_E_INVALID, "%s: table a is on device %d, table b on device %d", me, a->device, b->device);
  const int64_t GA = a->n_groups, GB = b->n_groups;
  if (GA >= (1ll << 31) - 1 || GB >= (1ll << 31) - 1)  // dq_prim's scan takes fewer than 2^31 items
    return set_error(DQ_E_UNSUPPORTED, "%s: a table of %lld groups (at most 2^31 - 2)", me, (long long)std::max(GA, GB));
  if (a->n_values == 0 || b->n_values == 0) return DQ_OK;  // defined = 0
  DQ_HIP(hipSetDevice(a->device));
  const hipStream_t S = reinterpret_cast<hipStream_t>(hip_stream);
  Frame fr(group_arena(), a->device);
  uint64_t *wa = nullptr, *wb = nullptr;
  int64_t *ca = nullptr, *cb = nullptr;
  unsigned long long* d_bits = nullptr;
  void* scan_tmp = nullptr;
  if (dq_status s = take(fr, wa, GA)) return s;
  if (dq_status s = take(fr, ca, GA + 1)) return s;
  if (dq_status s = take(fr, wb, GB)) return s;
  if (dq_status s = take(fr, cb, GB + 1)) return s;
  if (dq_status s = take(fr, scan_tmp, prim::scan_temp_bytes(std::max(GA, GB) + 1))) return s;
  if (dq_status s = take(fr, d_bits, 1)) return s;
  DQ_HIP(hipMemsetAsync(d_bits, 0, sizeof(*d_bits), S));
  hipLaunchKernelGGL(ks_order, dim3(dist_grid(GA + 1)), dim3(256), 0, S, a->d_keys.get(), a->d_counts.get(), GA,
                     kind[0], wa, ca);
  DQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(ks_order, dim3(dist_grid(GB + 1)), dim3(256), 0, S, b->d_keys.get(), b->d_counts.get(), GB,
                     kind[1], wb, cb);
  DQ_HIP(hipGetLastError());
  DQ_HIP(prim::exclusive_sum_i64(ca, ca, GA + 1, scan_tmp, S));
  DQ_HIP(prim::exclusive_sum_i64(cb, cb, GB + 1, scan_tmp, S));
  hipLaunchKernelGGL(ks_points, dim3(dist_grid(GA + GB)), dim3(256), 0, S, wa, ca, GA, (double)a->n_values, wb, cb, GB,
                     (double)b->n_values, d_bits);
  DQ_HIP(hipGetLastError());
  unsigned long long bits = 0;
  if (dq_status s = read_back(&bits, d_bits, S)) return s;
  std::memcpy(ks, &bits, sizeof(bits));
  *defined = 1;
  return DQ_OK;
}

}  // extern "C"
