// dq_cathist.hip -- the ColumnProfiler's third pass on the GPU: the counts of every value of K low-cardinality
// string / boolean columns in one read of each column.
//
// Reference: ColumnProfiler.computeHistograms (profiles/ColumnProfiler.scala:518-565): every row mapped to
// ((column, value), 1) for all target columns at once and counted by key; NULL counts under
// Histogram.NullFieldReplacement.  Pass 1 has bounded the targets' cardinality (lowCardinalityHistogramThreshold,
// default 120), so no sort, compaction or sample is needed: a workgroup counts a contiguous row range of one column
// into an open-addressed table in LDS -- (key, count, representative row) per slot, the key the grouping pass's
// 64-bit tuple hash (dq_strkey.h) -- and adds its occupied slots to the column's table in global memory at the end.
//
// Exactness.  A row is counted under a slot only after its bytes were compared with a row published in that slot
// before it: the slot's representative is the smallest row id seen (kept inverted, so that 0 is "none" and one
// memset clears a table), published with an atomic max whose return value is the representative it replaced.  A
// row that publishes itself is compared with the one it replaced, every other row with the one it read; the first
// has nothing to compare with.  By induction every row of a slot equals its first, in LDS and -- workgroup
// representatives against the global one, across chunks -- in global memory.  Different bytes under one key are a
// hash collision: the call fails (DQ_E_UNSUPPORTED), never a silent merge.  No lane waits for another: a key is
// claimed by compare-and-swap, and everything read afterwards is either absent or final enough to compare with
// (keys never change once set, representatives only move to other rows of the same chain).
//
// Capacity: kCatCap distinct non-null values per column in kCatSlots slots (load factor <= 0.5).  The claim that
// makes a table's kCatCap + 1st entry raises the column's `over` flag; its counts are then discarded (the caller
// falls back to dq_freq_build for that column) and other columns are untouched.  Probes are bounded by the slot
// count, so a full table ends a probe instead of spinning.
// Counts are integers: the order of the atomics cannot change a result, and the representative is the smallest
// row id, so two runs export identical arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "dq_hash.h"
#include "dq_hip_host.h"
#include "dq_strkey.h"

namespace dq {
namespace {

constexpr int kCatCap = 512;     // distinct non-null values per column (>= 4 x the default threshold of 120)
constexpr int kCatSlots = 1024;  // load factor <= 0.5; LDS: 8 + 8 + 4 bytes per slot = 20 KiB -> 8 workgroups per CU
constexpr int kCatBlock = 256;
constexpr int kCatPer = 2;                             // rows per thread and step
constexpr int kCatStep = kCatBlock * kCatPer;          // 512-row steps, as the other passes
constexpr int64_t kCatMinRows = 16 * kCatStep;         // rows per workgroup before the grid grows
constexpr int64_t kCatMaxRange = (int64_t)1 << 30;     // rows per workgroup at most: the LDS counts are 32-bit
constexpr int kCatWorkgroups = 2048;                   // 256 CUs x 8 resident workgroups
constexpr int kMaxCatCols = 1024;
constexpr int kMaxCatChunks = 4096;
constexpr int kCatRowBits = 40;                        // row id = chunk << 40 | row
constexpr uint64_t kZeroKey = 0x9E3779B97F4A7C15ull;   // stands in for the key 0 (0 marks an empty slot)

struct CatView {  // one column of one chunk
  const void* values;
  const uint32_t* validity;
  const void* offsets;
};

struct CatState {  // one column's table in global memory (all zero = empty)
  unsigned long long keys[kCatSlots];
  unsigned long long counts[kCatSlots];
  unsigned long long ireps[kCatSlots];  // ~(smallest row id), 0 = none
  unsigned long long n_null, n_true, n_false;
  uint32_t n_used, over;
};

__device__ __forceinline__ int cat_slot(uint64_t key) { return (int)((key * XP1) >> 54); }  // top 10 bits
static_assert(kCatSlots == 1 << 10, "cat_slot takes the product's top 10 bits");

// the 64 validity bits of rows [r0, r0 + 64) below n (r0 a multiple of 64; bitmaps are readable in 32-bit words)
__device__ __forceinline__ uint64_t valid64(const uint32_t* validity, int64_t r0, int64_t n) {
  const int64_t left = n - r0;
  const uint64_t range = left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
  if (!validity) return range;
  uint64_t w = left > 0 ? validity[r0 >> 5] : 0u;
  if (left > 32) w |= (uint64_t)validity[(r0 >> 5) + 1] << 32;
  return w & range;
}

__device__ __forceinline__ bool rows_equal(const CatView& va, bool large, int64_t a, const CatView& vb, int64_t b) {
  const uint8_t *pa, *pb;
  int64_t la, lb;
  str_of(va.values, va.offsets, large, a, pa, la);
  str_of(vb.values, vb.offsets, large, b, pb, lb);
  return la == lb && bytes_equal(pa, pb, la);
}

// String columns: blockIdx.y = the index into str_cols, blockIdx.x = the row range [x * range, (x + 1) * range) of
// the chunk (range a multiple of kCatStep).  A wave takes 64 consecutive rows per step and row of the thread: their
// validity is one scalar mask.
__global__ __launch_bounds__(kCatBlock) void cat_hist_str(const CatView* __restrict__ views, const int32_t* __restrict__ types,
                                                          const int32_t* __restrict__ str_cols, int32_t n_cols,
                                                          int32_t chunk, int64_t n, int64_t range, uint64_t key_mask,
                                                          CatState* __restrict__ states, int32_t* __restrict__ collision) {
  __shared__ unsigned long long s_key[kCatSlots];
  __shared__ unsigned long long s_irep[kCatSlots];
  __shared__ uint32_t s_cnt[kCatSlots];
  __shared__ uint32_t s_used, s_over;
  const int col = str_cols[blockIdx.y];
  CatState& st = states[col];
  const CatView view = views[(int64_t)chunk * n_cols + col];
  const bool large = types[col] == DQ_TYPE_LARGE_UTF8;
  for (int s = threadIdx.x; s < kCatSlots; s += kCatBlock) {
    s_key[s] = 0;
    s_irep[s] = 0;
    s_cnt[s] = 0;
  }
  if (threadIdx.x == 0) {
    s_used = 0;
    // over capacity already (an earlier chunk, another workgroup): one thread reads it, so that all leave or none
    s_over = __hip_atomic_load(&st.over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (s_over) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t begin = (int64_t)blockIdx.x * range, end = begin + range < n ? begin + range : n;
  const uint64_t chunk_bits = (uint64_t)chunk << kCatRowBits;
  unsigned long long nulls = 0;  // (the wave's, kept by every lane)
  bool collided = false;

  int64_t o0[kCatPer], o1[kCatPer], no0[kCatPer], no1[kCatPer];
  auto fetch = [&](int64_t base) __attribute__((always_inline)) {  // the offsets of the step at base
#pragma unroll
    for (int u = 0; u < kCatPer; ++u) {
      const int64_t r = base + u * kCatBlock + threadIdx.x;
      no0[u] = no1[u] = 0;
      if (r < end) {
        if (large) {
          no0[u] = reinterpret_cast<const int64_t*>(view.offsets)[r];
          no1[u] = reinterpret_cast<const int64_t*>(view.offsets)[r + 1];
        } else {
          no0[u] = reinterpret_cast<const int32_t*>(view.offsets)[r];
          no1[u] = reinterpret_cast<const int32_t*>(view.offsets)[r + 1];
        }
      }
    }
  };
  fetch(begin);
  for (int64_t base = begin; base < end; base += kCatStep) {
#pragma unroll
    for (int u = 0; u < kCatPer; ++u) {
      o0[u] = no0[u];
      o1[u] = no1[u];
    }
    if (base + kCatStep < end) fetch(base + kCatStep);  // a step ahead, in flight behind this step's strings
    if (__hip_atomic_load(&s_over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
#pragma unroll
    for (int u = 0; u < kCatPer; ++u) {
      const int64_t r = base + u * kCatBlock + threadIdx.x;
      const int64_t w0 = base + u * kCatBlock + wave * 64;  // the wave's first row: a multiple of 64
      const uint64_t vmask = valid64(view.validity, w0, end);
      const int64_t left = end - w0;
      const uint64_t in = left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
      nulls += (unsigned long long)__builtin_popcountll(in & ~vmask);
      const bool sel = (vmask >> lane) & 1ull;
      int slot = -1;
      if (sel) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(view.values) + o0[u];
        const int64_t len = o1[u] - o0[u];
        uint64_t key = str_tuple_hash(p, len) & key_mask;
        if (key == 0) key = kZeroKey;
        int s = cat_slot(key);
        for (int probe = 0; probe < kCatSlots; ++probe) {
          unsigned long long k = __hip_atomic_load(&s_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (k == 0) {
            if (__hip_atomic_load(&s_over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
            k = atomicCAS(&s_key[s], 0ull, (unsigned long long)key);
            if (k == 0) {  // claimed: the table's kCatCap + 1st entry puts the column over capacity
              k = key;
              if (atomicAdd(&s_used, 1u) >= (uint32_t)kCatCap)
                __hip_atomic_store(&s_over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
          if (k == key) {
            slot = s;
            break;
          }
          s = (s + 1) & (kCatSlots - 1);
        }
        if (slot < 0) {  // a full table, or over capacity already
          __hip_atomic_store(&s_over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          const unsigned long long mine = ~(chunk_bits | (uint64_t)r);
          unsigned long long cur = __hip_atomic_load(&s_irep[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (cur < mine) cur = atomicMax(&s_irep[slot], mine);  // none yet, or a later row: publish, get the replaced
          if (cur != 0 && cur != mine) {
            const int64_t rr = (int64_t)(~cur & ((1ull << kCatRowBits) - 1ull));  // (a row of this chunk)
            const uint8_t* q;
            int64_t qlen;
            str_of(view.values, view.offsets, large, rr, q, qlen);
            if (qlen != len || !bytes_equal(p, q, len)) collided = true;
          }
        }
      }
      // counts: lanes sharing the slot of the first pending lane add once, twice over (columns of two or three
      // values would otherwise serialise 64 atomics on one address); what is left adds by itself
#pragma unroll
      for (int round = 0; round < 2; ++round) {
        const uint64_t pending = __builtin_amdgcn_ballot_w64(slot >= 0);
        if (pending == 0) break;
        const int leader = __builtin_ctzll(pending);
        const int ls = __builtin_amdgcn_readlane(slot, leader);
        const uint64_t same = __builtin_amdgcn_ballot_w64(slot == ls);
        if (lane == leader) atomicAdd(&s_cnt[ls], (uint32_t)__builtin_popcountll(same));
        if (slot == ls) slot = -1;
      }
      if (slot >= 0) atomicAdd(&s_cnt[slot], 1u);
    }
  }
  if (collided) atomicOr(collision, 1);
  __syncthreads();
  if (s_over) {
    if (threadIdx.x == 0) __hip_atomic_store(&st.over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (lane == 0 && nulls) atomicAdd(&st.n_null, nulls);
  // the occupied slots into the column's global table: find or claim the key, add the count, publish the
  // representative and compare with the one it replaced (or the one already there)
  for (int ls = threadIdx.x; ls < kCatSlots; ls += kCatBlock) {
    const unsigned long long key = s_key[ls];
    if (key == 0) continue;
    int s = cat_slot(key), slot = -1;
    for (int probe = 0; probe < kCatSlots; ++probe) {
      unsigned long long k = __hip_atomic_load(&st.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k == 0) {
        if (__hip_atomic_load(&st.over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        k = atomicCAS(&st.keys[s], 0ull, key);
        if (k == 0) {
          k = key;
          if (atomicAdd(&st.n_used, 1u) >= (uint32_t)kCatCap)
            __hip_atomic_store(&st.over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (k == key) {
        slot = s;
        break;
      }
      s = (s + 1) & (kCatSlots - 1);
    }
    if (slot < 0) {
      __hip_atomic_store(&st.over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    atomicAdd(&st.counts[slot], (unsigned long long)s_cnt[ls]);
    const unsigned long long mine = s_irep[ls];
    unsigned long long cur = __hip_atomic_load(&st.ireps[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur < mine) cur = atomicMax(&st.ireps[slot], mine);
    if (cur != 0 && cur != mine) {
      const uint64_t ra = ~mine, rb = ~cur;  // rb: a row of this or an earlier chunk
      const CatView other = views[(int64_t)(rb >> kCatRowBits) * n_cols + col];
      if (!rows_equal(view, large, (int64_t)(ra & ((1ull << kCatRowBits) - 1ull)), other,
                      (int64_t)(rb & ((1ull << kCatRowBits) - 1ull))))
        atomicOr(collision, 1);
    }
  }
}

// Boolean columns: TRUE / FALSE / NULL counts from popcounts of the value and validity words (bit 0 = row 0 of the
// chunk, as the column pass reads them), the last word masked at the chunk's end.  blockIdx.y = index into bool_cols.
__global__ __launch_bounds__(kCatBlock) void cat_hist_bool(const CatView* __restrict__ views, const int32_t* __restrict__ bool_cols,
                                                           int32_t n_cols, int32_t chunk, int64_t n,
                                                           CatState* __restrict__ states) {
  const int col = bool_cols[blockIdx.y];
  const CatView view = views[(int64_t)chunk * n_cols + col];
  const uint32_t* values = reinterpret_cast<const uint32_t*>(view.values);
  const int64_t words = (n + 31) >> 5;
  unsigned long long t = 0, f = 0, z = 0;
  for (int64_t w = (int64_t)blockIdx.x * kCatBlock + threadIdx.x; w < words; w += (int64_t)gridDim.x * kCatBlock) {
    const int64_t left = n - (w << 5);
    const uint32_t in = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
    const uint32_t sel = (view.validity ? view.validity[w] : 0xFFFFFFFFu) & in;
    const uint32_t v = values[w];
    t += __popc(sel & v);
    f += __popc(sel & ~v);
    z += __popc(in & ~sel);
  }
  for (int d = 32; d >= 1; d >>= 1) {
    t += __shfl_xor(t, d);
    f += __shfl_xor(f, d);
    z += __shfl_xor(z, d);
  }
  if ((threadIdx.x & 63) == 0) {
    CatState& st = states[col];
    if (t) atomicAdd(&st.n_true, t);
    if (f) atomicAdd(&st.n_false, f);
    if (z) atomicAdd(&st.n_null, z);
  }
}

}  // namespace
}  // namespace dq

using namespace dq;

struct dq_cat_hist {
  struct Column {
    int32_t status = 0;  // 0 ok, 1 over capacity
    int64_t n_null = 0;
    std::vector<int64_t> counts;    // in the order of rep_rows
    std::vector<uint64_t> rep_rows;  // strings: ascending row ids (first occurrences); booleans: the value, 0 / 1
  };
  std::vector<Column> cols;
};

extern "C" {

int32_t dq_cat_hist_capacity(void) { return kCatCap; }

dq_status dq_cat_hist_build(const int32_t* types, int32_t n_cols, const dq_column_view* cols, const int64_t* chunk_rows,
                            int32_t n_chunks, int32_t device, void* hip_stream, dq_cat_hist** out) {
  if (!out) return set_error(DQ_E_INVALID, "dq_cat_hist_build: out is NULL");
  *out = nullptr;
  if (n_cols < 0 || n_cols > kMaxCatCols || (n_cols > 0 && !types))
    return set_error(DQ_E_INVALID, "dq_cat_hist_build: 0..%d columns", kMaxCatCols);
  if (n_chunks < 0 || n_chunks > kMaxCatChunks || (n_chunks > 0 && n_cols > 0 && (!cols || !chunk_rows)))
    return set_error(DQ_E_INVALID, "dq_cat_hist_build: bad chunks (at most %d)", kMaxCatChunks);
  std::vector<int32_t> str_cols, bool_cols;
  for (int c = 0; c < n_cols; ++c) {
    if (types[c] == DQ_TYPE_UTF8 || types[c] == DQ_TYPE_LARGE_UTF8) str_cols.push_back(c);
    else if (types[c] == DQ_TYPE_BOOL) bool_cols.push_back(c);
    else return set_error(DQ_E_UNSUPPORTED, "dq_cat_hist_build: column %d of type %d (UTF8, LARGE_UTF8 and BOOL only)", c, types[c]);
  }
  int64_t total = 0;
  for (int k = 0; k < n_chunks && n_cols > 0; ++k) {
    if (chunk_rows[k] < 0 || chunk_rows[k] >= (1ll << kCatRowBits))
      return set_error(DQ_E_INVALID, "dq_cat_hist_build: chunk %d has %lld rows", k, (long long)chunk_rows[k]);
    total += chunk_rows[k];
    for (int c = 0; c < n_cols && chunk_rows[k] > 0; ++c) {
      const dq_column_view& v = cols[(size_t)k * n_cols + c];
      if (v.reserved != 0 || !v.values || (types[c] != DQ_TYPE_BOOL && !v.offsets))
        return set_error(DQ_E_INVALID, "dq_cat_hist_build: bad view of column %d in chunk %d", c, k);
      if (((uintptr_t)v.values & (types[c] == DQ_TYPE_BOOL ? 3 : 0)) || ((uintptr_t)v.validity & 3) ||
          ((uintptr_t)v.offsets & (types[c] == DQ_TYPE_LARGE_UTF8 ? 7 : 3)))
        return set_error(DQ_E_INVALID, "dq_cat_hist_build: misaligned buffer of column %d in chunk %d", c, k);
      if (types[c] == DQ_TYPE_UTF8 && chunk_rows[k] >= INT32_MAX)
        return set_error(DQ_E_INVALID, "dq_cat_hist_build: UTF8 chunk of %lld rows", (long long)chunk_rows[k]);
    }
  }
  auto h = std::make_unique<dq_cat_hist>();
  h->cols.resize((size_t)n_cols);
  if (n_cols == 0 || total == 0) {  // nothing to read: every column empty
    *out = h.release();
    return DQ_OK;
  }
  const uint64_t key_mask = test_hash_mask();
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));

  std::vector<CatView> hviews((size_t)n_chunks * n_cols);
  for (size_t i = 0; i < hviews.size(); ++i)
    hviews[i] = CatView{cols[i].values, reinterpret_cast<const uint32_t*>(cols[i].validity), cols[i].offsets};
  std::vector<int32_t> hidx;  // types, then the string columns, then the boolean columns
  hidx.insert(hidx.end(), types, types + n_cols);
  hidx.insert(hidx.end(), str_cols.begin(), str_cols.end());
  hidx.insert(hidx.end(), bool_cols.begin(), bool_cols.end());
  StreamBuf d_views, d_idx, d_states, d_coll;
  DQ_HIP(d_views.alloc(hviews.size() * sizeof(CatView), st));
  DQ_HIP(d_idx.alloc(hidx.size() * sizeof(int32_t), st));
  DQ_HIP(d_states.alloc((size_t)n_cols * sizeof(CatState), st));
  DQ_HIP(d_coll.alloc(sizeof(int32_t), st));
  DQ_HIP(hipMemcpyAsync(d_views.get(), hviews.data(), hviews.size() * sizeof(CatView), hipMemcpyHostToDevice, st));
  DQ_HIP(hipMemcpyAsync(d_idx.get(), hidx.data(), hidx.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  DQ_HIP(hipMemsetAsync(d_states.get(), 0, (size_t)n_cols * sizeof(CatState), st));
  DQ_HIP(hipMemsetAsync(d_coll.get(), 0, sizeof(int32_t), st));
  const int32_t* d_types = static_cast<const int32_t*>(d_idx.get());
  const int32_t* d_str = d_types + n_cols;
  const int32_t* d_bool = d_str + str_cols.size();
  auto* states = static_cast<CatState*>(d_states.get());

  for (int k = 0; k < n_chunks; ++k) {
    const int64_t n = chunk_rows[k];
    if (n == 0) continue;
    if (!str_cols.empty()) {
      // a workgroup's contiguous range: whole 512-row steps, at least kCatMinRows where the chunk has them, the
      // grid about kCatWorkgroups over all columns, and never more than kCatMaxRange rows (32-bit LDS counts)
      const int64_t per_col = std::max<int64_t>(1, kCatWorkgroups / (int64_t)str_cols.size());
      int64_t gx = std::max<int64_t>(1, std::min<int64_t>(per_col, (n + kCatMinRows - 1) / kCatMinRows));
      int64_t range = ((n + gx - 1) / gx + kCatStep - 1) / kCatStep * kCatStep;
      range = std::min(range, kCatMaxRange);
      gx = (n + range - 1) / range;
      hipLaunchKernelGGL(cat_hist_str, dim3((unsigned)gx, (unsigned)str_cols.size()), dim3(kCatBlock), 0, st,
                         static_cast<const CatView*>(d_views.get()), d_types, d_str, n_cols, (int32_t)k, n, range, key_mask,
                         states, static_cast<int32_t*>(d_coll.get()));
      DQ_HIP(hipGetLastError());
    }
    if (!bool_cols.empty()) {
      const int64_t words = (n + 31) / 32;
      const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(1024, (words + kCatBlock * 4 - 1) / (kCatBlock * 4)));
      hipLaunchKernelGGL(cat_hist_bool, dim3((unsigned)gx, (unsigned)bool_cols.size()), dim3(kCatBlock), 0, st,
                         static_cast<const CatView*>(d_views.get()), d_bool, n_cols, (int32_t)k, n, states);
      DQ_HIP(hipGetLastError());
    }
  }
  std::vector<CatState> hstates((size_t)n_cols);
  int32_t collided = 0;
  DQ_HIP(hipMemcpyAsync(hstates.data(), d_states.get(), (size_t)n_cols * sizeof(CatState), hipMemcpyDeviceToHost, st));
  DQ_HIP(hipMemcpyAsync(&collided, d_coll.get(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (collided) return set_error(DQ_E_UNSUPPORTED, "dq_freq_build: 64-bit tuple-hash collision between distinct values");

  for (int c = 0; c < n_cols; ++c) {
    const CatState& s = hstates[(size_t)c];
    dq_cat_hist::Column& o = h->cols[(size_t)c];
    if (types[c] == DQ_TYPE_BOOL) {
      o.n_null = (int64_t)s.n_null;
      if (s.n_false) { o.counts.push_back((int64_t)s.n_false); o.rep_rows.push_back(0); }
      if (s.n_true) { o.counts.push_back((int64_t)s.n_true); o.rep_rows.push_back(1); }
      continue;
    }
    if (s.over || s.n_used > (uint32_t)kCatCap) {
      o.status = 1;
      continue;
    }
    o.n_null = (int64_t)s.n_null;
    std::vector<std::pair<uint64_t, int64_t>> groups;  // (row id, count), by first occurrence
    for (int i = 0; i < kCatSlots; ++i)
      if (s.keys[i]) groups.emplace_back(~(uint64_t)s.ireps[i], (int64_t)s.counts[i]);
    std::sort(groups.begin(), groups.end());
    for (const auto& g : groups) {
      o.rep_rows.push_back(g.first);
      o.counts.push_back(g.second);
    }
  }
  *out = h.release();
  return DQ_OK;
}

dq_status dq_cat_hist_column(const dq_cat_hist* h, int32_t col, int32_t* status, int64_t* n_null, int32_t* n_values) {
  if (!h || col < 0 || (size_t)col >= h->cols.size() || !status || !n_null || !n_values)
    return set_error(DQ_E_INVALID, "dq_cat_hist_column: bad arguments");
  const dq_cat_hist::Column& c = h->cols[(size_t)col];
  *status = c.status;
  *n_null = c.n_null;
  *n_values = (int32_t)c.counts.size();
  return DQ_OK;
}

dq_status dq_cat_hist_export(const dq_cat_hist* h, int32_t col, int64_t* counts, uint64_t* rep_rows, int32_t cap) {
  if (!h || col < 0 || (size_t)col >= h->cols.size()) return set_error(DQ_E_INVALID, "dq_cat_hist_export: bad arguments");
  const dq_cat_hist::Column& c = h->cols[(size_t)col];
  if (c.status != 0) return set_error(DQ_E_STATE, "dq_cat_hist_export: column %d is over capacity", col);
  const size_t n = c.counts.size();
  if ((size_t)std::max(cap, 0) < n || (n > 0 && (!counts || !rep_rows)))
    return set_error(DQ_E_INVALID, "dq_cat_hist_export: %zu values, room for %d", n, cap);
  if (n > 0) {
    std::memcpy(counts, c.counts.data(), n * sizeof(int64_t));
    std::memcpy(rep_rows, c.rep_rows.data(), n * sizeof(uint64_t));
  }
  return DQ_OK;
}

void dq_cat_hist_destroy(dq_cat_hist* h) { delete h; }

}  // extern "C"
