// dq_dict.hip -- dictionary-encoded string columns (DQ_TYPE_DICT_UTF8) on gfx950.
//
//   dq_dict_entries   one pass over a dictionary's D entries: XXH64 (seed 42) of the entry's bytes -> HLL register
//                     index and rank, the entry's StatefulDataType class, its non-null bit -> one uint32 entry word.
//   dq_dict_scan      the row pass of a plan: per row the int32 index, its validity bit and the `where` bit; the
//                     entry word is gathered (bounds-checked) and accumulated into the same ColPartial fields and
//                     privatised LDS HLL registers the utf8_* column variants fill.  No string byte is read.
//   dq_dict_decode    (index, validity, entry non-null) -> gather index + output validity, then dq_take_rows'
//                     string gather (dq::take_strings, dq_schema.hip): the plain UTF8 column.
//   dq_dict_count     counts[e] += rows that carry index e (valid row, index inside the table, entry non-NULL): the
//                     grouping of the column, from which dq_freq_build_weighted makes the frequency table.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "dq_device.h"
#include "dq_hash.h"
#include "dq_hip_host.h"
#include "dq_lane.h"

namespace dq {

// ------------------------------------------------------------------------------------------
// Entry pass
// ------------------------------------------------------------------------------------------
// 32 bytes from byte `pos` of an entry of n bytes as little-endian dwords; bytes past the entry read 0 (byte
// loads: an entry may start at any byte and end at the buffer's last one)
__device__ __forceinline__ void dict_load32(const uint8_t* p, int64_t pos, int64_t n, uint32_t (&w)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (pos + 4 * k + b < n) v |= (uint32_t)p[pos + 4 * k + b] << (8 * b);
    w[k] = v;
  }
}

// XXH64.hashUnsafeBytes (seed 42) of p[0, n) in dq_hash.h's formulation: the 32-byte stripe loop and the merge
// for n >= 32, then the remainder's rounds (what dq_kernels.hip xxh64_window_head runs for the string pass)
__device__ uint64_t dict_hash(const uint8_t* p, int64_t n) {
  uint64_t h = kSeed + XP5;
  int64_t pos = 0;
  uint32_t w[8];
  if (n >= 32) {
    uint64_t v[4] = {kXxhV0, kXxhV1, kXxhV2, kXxhV3};
    const int64_t end = n & ~int64_t(31);
    do {
      dict_load32(p, pos, n, w);
      xxh64_stripe32(v, w);
      pos += 32;
    } while (pos < end);
    h = xxh64_merge4(v);
  }
  dict_load32(p, pos, n, w);
  return fmix_tail(xxh64_rem_head(h + (uint64_t)n, w, (uint32_t)(n & 31), MulP5{}));
}

// StatefulDataType's class of a string value (dq_kernels.hip dt_class_bytes, the string pass's any-length path;
// DtClass numbering): FRACTIONAL 1, INTEGRAL 2, BOOLEAN 3, STRING 4
__device__ uint32_t dict_class(const uint8_t* p, int64_t len) {
  int64_t i = 0;
  if (len > 0 && (p[0] == '+' || p[0] == '-')) i = 1;
  if (i < len && p[i] == ' ') ++i;
  bool numeric = true;
  uint32_t dots = 0;
  for (; i < len && numeric; ++i) {
    const uint8_t c = p[i];
    if (c == '.') ++dots;
    else if (c < '0' || c > '9') numeric = false;
  }
  const bool boolean = (len == 4 && p[0] == 't' && p[1] == 'r' && p[2] == 'u' && p[3] == 'e') ||
                       (len == 5 && p[0] == 'f' && p[1] == 'a' && p[2] == 'l' && p[3] == 's' && p[4] == 'e');
  return numeric && dots <= 1 ? (dots ? 1u : 2u) : (boolean ? 3u : 4u);
}

template <typename OffT>
__global__ __launch_bounds__(kBlock) void dq_dict_entries_kernel(const uint8_t* __restrict__ data,
                                                                 const OffT* __restrict__ offsets,
                                                                 const uint32_t* __restrict__ validity, int64_t n,
                                                                 uint32_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  uint32_t word = 0;  // a NULL entry: every field 0
  if (!validity || ((validity[e >> 5] >> ((uint32_t)e & 31u)) & 1u)) {
    const int64_t o0 = (int64_t)offsets[e];
    int64_t len = (int64_t)offsets[e + 1] - o0;
    if (len < 0) len = 0;
    const uint64_t x = dict_hash(data + o0, len);
    const uint32_t idx = (uint32_t)(x >> 55);
    const uint32_t pw = (uint32_t)__clzll((long long)((x << 9) | 256ull)) + 1u;  // StatefulHyperloglogPlus.scala:96-113
    word = idx | pw << kDictPwShift | dict_class(data + o0, len) << kDictClassShift | kDictNonNull;
  }
  out[e] = word;
}

// ------------------------------------------------------------------------------------------
// Row pass
// ------------------------------------------------------------------------------------------
// Workgroup b: task b % ntasks, row range b / ntasks (as dq_column_scan).  Lane l of wave w takes rows
// base + 64 j + l of the wave's 512-row block, so a 64-row group's selection (validity & where, clipped to the
// range) is one scalar word and the selected / non-null counts are popcounts of ballots.  An index is used only
// after (uint32_t)idx < D; a row that fails it is NULL, without the load.
__global__ __launch_bounds__(kBlock) void dq_dict_scan(const ColTask* __restrict__ tasks, int32_t ntasks,
                                                       int32_t part_base, ScanCols cols, DictSizes sizes, ScanBitmaps bm,
                                                       int64_t n_rows, int64_t rows_per_range,
                                                       ColPartial* __restrict__ partials,
                                                       uint32_t* __restrict__ hll_acc) {
  __shared__ int32_t regs[512];               // q = pw - 1, -1 = empty
  __shared__ uint32_t tab[kDictLdsEntries];   // the entry table, when it fits
  __shared__ uint32_t red[kWaves][4];
  const int32_t ti = blockIdx.x % ntasks;
  const int32_t range = blockIdx.x / ntasks;
  const ColTask t = tasks[ti];
  const int64_t row0 = (int64_t)range * rows_per_range;
  int64_t row1 = row0 + rows_per_range;
  if (row1 > n_rows) row1 = n_rows;
  const int32_t* __restrict__ indices = reinterpret_cast<const int32_t*>(cols.values[t.col]);
  const uint32_t* validity = cols.validity[t.col];
  const uint32_t* __restrict__ gtab = reinterpret_cast<const uint32_t*>(cols.offsets[t.col]);
  const uint32_t D = (uint32_t)sizes.n[t.col];
  const uint32_t* mask = t.where >= 0 ? reinterpret_cast<const uint32_t*>(bm.where_bits[t.where]) : nullptr;
  const bool hll = (t.arg & kDictArgHll) != 0, dtype = (t.arg & kDictArgDtype) != 0;
  const bool staged = D <= (uint32_t)kDictLdsEntries;  // (block-uniform)
  for (int i = threadIdx.x; i < 512; i += kBlock) regs[i] = -1;
  if (staged)
    for (uint32_t i = threadIdx.x; i < D; i += kBlock) tab[i] = gtab[i];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t cnt = 0, frac = 0, integ = 0, boolean = 0;  // cnt: wave-uniform; the class counts per lane
  const int32_t nr = (int32_t)(row1 - row0);
  for (int32_t rb = wave * 512; rb < nr; rb += kRowsPerIter) {
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
      const int32_t left = nr - rb - 64 * j;  // rows of this group below row1
      if (left <= 0) break;
      const int64_t gbase = row0 + rb + 64 * j;
      const uint64_t m = sel_word(validity, mask, gbase >> 5, left);
      if (m == 0) continue;
      const bool sel = lane_bit(m);
      uint32_t word = 0;
      if (sel) {
        const uint32_t idx = (uint32_t)indices[gbase + lane];
        if (idx < D) word = staged ? tab[idx] : gtab[idx];
      }
      const bool nn = (word & kDictNonNull) != 0;
      cnt += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(nn));
      if (hll && nn)
        atomicMax(&regs[word & ((1u << kDictIdxBits) - 1u)],
                  (int32_t)((word >> kDictPwShift) & ((1u << kDictPwBits) - 1u)) - 1);
      if (dtype) {
        const uint32_t cls = (word >> kDictClassShift) & ((1u << kDictClassBits) - 1u);
        frac += cls == 1u;
        integ += cls == 2u;
        boolean += cls == 3u;
      }
    }
  }
  frac = wave_sum_u32(frac);
  integ = wave_sum_u32(integ);
  boolean = wave_sum_u32(boolean);
  if (lane == 0) {
    red[wave][0] = cnt; red[wave][1] = frac; red[wave][2] = integ; red[wave][3] = boolean;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t c = 0, f = 0, g = 0, b = 0;
    for (int w = 0; w < kWaves; ++w) { c += red[w][0]; f += red[w][1]; g += red[w][2]; b += red[w][3]; }
    // the string tasks' use of ColPartial (dq_kernels.hip DtCounts::flush): count = selected non-null rows,
    // isum = FRACTIONAL, nan_count = INTEGRAL, sum = BOOLEAN; every other field neutral (stats_init)
    ColPartial p;
    p.n = 0.0; p.mean = 0.0; p.m2 = 0.0;
    p.sum = (double)b;
    p.isum = f;
    p.count = c;
    p.nan_count = g;
    p.fmin = __longlong_as_double(0x7FF0000000000000ll);
    p.fmax = __longlong_as_double((long long)0xFFF0000000000000ull);
    p.pinf_count = 0; p.ninf_count = 0; p.isum_hi = 0;
    partials[(size_t)(part_base + ti) * kMaxWG + range] = p;
  }
  if (hll && t.hll_slot >= 0) {
    // (the barrier above ordered every wave's register updates before these reads; merge as dq_column_scan does)
    uint32_t* dst = hll_acc + ((size_t)t.hll_slot * kHllCopies + (blockIdx.x % kHllCopies)) * 512;
    for (int i = threadIdx.x; i < 512; i += kBlock) {
      const uint32_t v = (uint32_t)(regs[i] + 1);
      if (v > __builtin_nontemporal_load(dst + i)) atomicMax(dst + i, v);
    }
  }
}

hipError_t launch_dict_scan(const ColTask* tasks, int32_t ntasks, int32_t part_base, const ScanCols& cols,
                            const DictSizes& sizes, const ScanBitmaps& bm, int64_t n_rows, int64_t rows_per_range,
                            int32_t nranges, ColPartial* partials, uint32_t* hll_acc, hipStream_t stream) {
  hipLaunchKernelGGL(dq_dict_scan, dim3((unsigned)(ntasks * nranges)), dim3(kBlock), 0, stream, tasks, ntasks, part_base,
                     cols, sizes, bm, n_rows, rows_per_range, partials, hll_acc);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Decode
// ------------------------------------------------------------------------------------------
// gather[r] = the entry row r decodes to, or -1 for a NULL row (index validity 0, entry NULL, index outside the
// table); out_validity word g = those bits of rows 64 g .. 64 g + 63 (bits past n_rows 0)
__global__ __launch_bounds__(kBlock) void dq_dict_gather_index(const int32_t* __restrict__ indices,
                                                               const uint32_t* __restrict__ validity,
                                                               const uint32_t* __restrict__ entry_validity, int64_t n_rows,
                                                               int64_t n_entries, int64_t* __restrict__ gather,
                                                               uint64_t* __restrict__ out_validity) {
  const int lane = threadIdx.x & 63;
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;  // wave-uniform
  const int64_t r = g * 64 + lane;
  bool ok = false;
  if (r < n_rows) {
    ok = !validity || ((validity[r >> 5] >> ((uint32_t)r & 31u)) & 1u);
    int64_t e = -1;
    if (ok) {
      const uint32_t idx = (uint32_t)indices[r];
      ok = (int64_t)idx < n_entries && (!entry_validity || ((entry_validity[idx >> 5] >> (idx & 31u)) & 1u));
      if (ok) e = (int64_t)idx;
    }
    gather[r] = e;
  }
  const uint64_t m = __builtin_amdgcn_ballot_w64(ok);
  if (lane == 0 && g * 64 < n_rows && out_validity) out_validity[g] = m;
}

// ------------------------------------------------------------------------------------------
// Index count
// ------------------------------------------------------------------------------------------
// A table of at most this many entries is counted in a workgroup-private LDS table of uint32 counters (16 KB: eight
// workgroups, the CU's 32 waves, hold 128 KB of its 160 KB; twice as many entries would leave room for five)
constexpr int32_t kDictCountLdsEntries = 4096;
constexpr int32_t kDictCountMaxWG = 2048;  // row ranges per launch: eight workgroups per CU

// Workgroup b counts rows [b rows_per_range, (b + 1) rows_per_range), lane l of a wave taking row base + 64 j + l as
// dq_dict_scan does (rows_per_range is a multiple of kRowsPerIter: a 64-row group's validity is one scalar word).  A
// row counts when its validity bit is set, (uint32_t)idx < D and its entry word has the non-NULL bit -- dq_dict_scan's
// rule for a non-NULL row; an index that fails the compare touches neither table.
// STAGED: the counters live in LDS (a range is below 2^31 rows: they cannot wrap) and are added to counts[] once per
// workgroup, entry e by lane e % 256 (consecutive 8-byte adds), where the entry's non-NULL bit is looked at -- once
// per entry and workgroup, not per row.  Not STAGED: one global add per counted row.  (Combining the equal indices
// of a 64-row group before the LDS add -- one pass per distinct index -- was measured and lost)
// SEL: the group's word is validity & mask, mask being the selection bitmap (dq_lane.h's sel_word: one more scalar
// load per 64 rows).
template <bool STAGED, bool SEL>
__global__ __launch_bounds__(kBlock) void dq_dict_count_kernel(const int32_t* __restrict__ indices,
                                                               const uint32_t* validity, const uint32_t* mask,
                                                               const uint32_t* __restrict__ gtab, uint32_t D,
                                                               int64_t n_rows, int64_t rows_per_range,
                                                               unsigned long long* __restrict__ counts) {
  __shared__ uint32_t cnt[STAGED ? kDictCountLdsEntries : 1];
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_range;
  int64_t row1 = row0 + rows_per_range;
  if (row1 > n_rows) row1 = n_rows;
  if constexpr (STAGED) {
    for (uint32_t i = threadIdx.x; i < D; i += kBlock) cnt[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t nr = (int32_t)(row1 - row0);
  for (int32_t rb = wave * 512; rb < nr; rb += kRowsPerIter) {
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
      const int32_t left = nr - rb - 64 * j;  // rows of this group below row1
      if (left <= 0) break;
      const int64_t gbase = row0 + rb + 64 * j;
      const uint64_t m = SEL ? sel_word(validity, mask, gbase >> 5, left) : sel_word(validity, gbase >> 5, left);
      if (m == 0) continue;
      uint32_t idx = D;
      if (lane_bit(m)) idx = (uint32_t)indices[gbase + lane];
      const bool in = idx < D;
      if constexpr (STAGED) {
        if (in) atomicAdd(&cnt[idx], 1u);
      } else {
        if (in && (gtab[idx] & kDictNonNull)) atomicAdd(&counts[idx], 1ull);
      }
    }
  }
  if constexpr (STAGED) {
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < D; e += kBlock) {
      const uint32_t c = cnt[e];
      if (c && (gtab[e] & kDictNonNull)) atomicAdd(&counts[e], (unsigned long long)c);
    }
  }
}

}  // namespace dq

extern "C" {

dq_status dq_dict_entries(int32_t dict_type, const dq_column_view* dict, int64_t n_entries, uint32_t* entries_out,
                          int32_t device, void* hip_stream) {
  using namespace dq;
  const char* me = "dq_dict_entries";
  if (dict_type != DQ_TYPE_UTF8 && dict_type != DQ_TYPE_LARGE_UTF8)
    return set_error(DQ_E_UNSUPPORTED, "%s: dictionary values of type %d (UTF8 / LARGE_UTF8 only)", me, dict_type);
  if (!dict || dict->reserved != 0 || n_entries < 0 || n_entries > INT32_MAX)
    return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (n_entries == 0) return DQ_OK;
  if (!entries_out || !dict->offsets || ((uintptr_t)entries_out & 3) || ((uintptr_t)dict->offsets & 3) ||
      ((uintptr_t)dict->validity & 3))
    return set_error(DQ_E_INVALID, "%s: NULL or misaligned buffer", me);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  const unsigned grid = (unsigned)((n_entries + kBlock - 1) / kBlock);
  const uint8_t* data = static_cast<const uint8_t*>(dict->values);
  const uint32_t* val = reinterpret_cast<const uint32_t*>(dict->validity);
  if (dict_type == DQ_TYPE_LARGE_UTF8)
    hipLaunchKernelGGL(dq_dict_entries_kernel<int64_t>, dim3(grid), dim3(kBlock), 0, st, data,
                       static_cast<const int64_t*>(dict->offsets), val, n_entries, entries_out);
  else
    hipLaunchKernelGGL(dq_dict_entries_kernel<int32_t>, dim3(grid), dim3(kBlock), 0, st, data,
                       static_cast<const int32_t*>(dict->offsets), val, n_entries, entries_out);
  DQ_HIP(hipGetLastError());
  return DQ_OK;
}

dq_status dq_dict_decode(int32_t dict_type, const dq_column_view* dict, int64_t n_entries,
                         const dq_column_view* indices, int64_t n_rows, void* out_values, int64_t values_capacity,
                         uint8_t* out_validity, void* out_offsets, int64_t* data_bytes, int32_t device,
                         void* hip_stream) {
  using namespace dq;
  const char* me = "dq_dict_decode";
  if (dict_type != DQ_TYPE_UTF8 && dict_type != DQ_TYPE_LARGE_UTF8)
    return set_error(DQ_E_UNSUPPORTED, "%s: dictionary values of type %d (UTF8 / LARGE_UTF8 only)", me, dict_type);
  if (!dict || !indices || dict->reserved != 0 || indices->reserved != 0 || n_entries < 0 || n_entries > INT32_MAX ||
      n_rows < 0 || values_capacity < 0)
    return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (data_bytes) *data_bytes = 0;
  if (n_rows == 0) return DQ_OK;
  if (!indices->values || !out_offsets || (n_entries > 0 && !dict->offsets))
    return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
  if (((uintptr_t)indices->values & 3) || ((uintptr_t)indices->validity & 3) || ((uintptr_t)dict->validity & 3) ||
      ((uintptr_t)dict->values & 3) || ((uintptr_t)dict->offsets & 3) || ((uintptr_t)out_validity & 7) ||
      ((uintptr_t)out_offsets & 7) || ((uintptr_t)out_values & 15))
    return set_error(DQ_E_INVALID, "%s: misaligned buffer", me);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  DevPtr<int64_t> gather;
  DQ_HIP(gather.alloc((size_t)n_rows));
  const unsigned grid = (unsigned)((((n_rows + 63) >> 6) * 64 + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(dq_dict_gather_index, dim3(grid), dim3(kBlock), 0, st, static_cast<const int32_t*>(indices->values),
                     reinterpret_cast<const uint32_t*>(indices->validity), reinterpret_cast<const uint32_t*>(dict->validity),
                     n_rows, n_entries, gather.get(), reinterpret_cast<uint64_t*>(out_validity));
  DQ_HIP(hipGetLastError());
  // (take_strings synchronises the stream before it returns: the gather index is freed after its last use)
  return take_strings(dict_type == DQ_TYPE_LARGE_UTF8, dict, n_entries, gather.get(), n_rows, out_values,
                      values_capacity, out_offsets, data_bytes, st, me);
}

static dq_status dict_count_impl(const char* me, const dq_column_view* indices, int64_t n_rows,
                                 const uint64_t* selection, int64_t* counts, int32_t device, void* hip_stream) {
  using namespace dq;
  if ((uintptr_t)selection & 7) return set_error(DQ_E_INVALID, "%s: the selection is not 8-byte aligned", me);
  if (!indices || indices->reserved < 0 || indices->reserved > INT32_MAX || n_rows < 0)
    return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (n_rows > INT32_MAX) return set_error(DQ_E_UNSUPPORTED, "%s: at most 2^31 - 1 rows per call", me);
  const uint32_t D = (uint32_t)indices->reserved;
  if (n_rows == 0 || D == 0) return DQ_OK;  // (no entry: every row is NULL)
  if (!indices->values || !indices->offsets || !counts) return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
  if (((uintptr_t)indices->values & 3) || ((uintptr_t)indices->validity & 3) || ((uintptr_t)indices->offsets & 3) ||
      ((uintptr_t)counts & 7))
    return set_error(DQ_E_INVALID, "%s: misaligned buffer", me);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  // row ranges: whole kRowsPerIter blocks, at most kDictCountMaxWG of them
  const int64_t blocks = (n_rows + kRowsPerIter - 1) / kRowsPerIter;
  const int64_t rows_per_range = (blocks + kDictCountMaxWG - 1) / kDictCountMaxWG * kRowsPerIter;
  const unsigned grid = (unsigned)((n_rows + rows_per_range - 1) / rows_per_range);
  // DQ_DICT_COUNT_AB=global (dqscan.h; A/B runs of tools/dict_bench.py): a small table is counted with global adds
  // too; exactly that value, read per call
  const char* knob = std::getenv("DQ_DICT_COUNT_AB");
  const bool staged = D <= (uint32_t)kDictCountLdsEntries && !(knob && std::strcmp(knob, "global") == 0);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, static_cast<const int32_t*>(indices->values),
                       reinterpret_cast<const uint32_t*>(indices->validity), reinterpret_cast<const uint32_t*>(selection),
                       static_cast<const uint32_t*>(indices->offsets), D, n_rows, rows_per_range,
                       reinterpret_cast<unsigned long long*>(counts));
  };
  if (selection) {
    if (staged) launch(dq_dict_count_kernel<true, true>);
    else launch(dq_dict_count_kernel<false, true>);
  } else {
    if (staged) launch(dq_dict_count_kernel<true, false>);
    else launch(dq_dict_count_kernel<false, false>);
  }
  DQ_HIP(hipGetLastError());
  return DQ_OK;
}

dq_status dq_dict_count(const dq_column_view* indices, int64_t n_rows, int64_t* counts, int32_t device,
                        void* hip_stream) {
  return dict_count_impl("dq_dict_count", indices, n_rows, nullptr, counts, device, hip_stream);
}

dq_status dq_dict_count_where(const dq_column_view* indices, int64_t n_rows, const uint64_t* selection, int64_t* counts,
                              int32_t device, void* hip_stream) {
  return dict_count_impl("dq_dict_count_where", indices, n_rows, selection, counts, device, hip_stream);
}

}  // extern "C"
