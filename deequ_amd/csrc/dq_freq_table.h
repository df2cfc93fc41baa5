// dq_freq_table.h -- the frequency table (dq_freq_table) and the pieces that read it, shared by the four translation
// units that work on such tables: the grouping analyzers' build, MutualInformation, summary and top-N (dq_group.hip),
// the table as a persisted state -- merge, value store, image (dq_freq_store.hip), the probes of other data's rows
// against a table (dq_probe.hip) and the comparison of two tables (dq_dist.hip).  One copy of the chunk descriptor, of
// the value-bits rule (NaN canonical, -0.0 and 0.0 distinct), of the row's validity, hash and key -- a probe hashes a
// row exactly as the build hashed it, because both call these -- of the by-value tuple comparison, and of the scratch
// arena's and the launches' host helpers.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "dq_arena.h"
#include "dq_hash.h"
#include "dq_hip_host.h"
#include "dq_strkey.h"

namespace dq {

constexpr int kMaxGroupCols = 8;
constexpr int kMaxGroupChunks = 4096;
constexpr int kRowBits = 40;  // row id = chunk << 40 | row

constexpr uint64_t kSeed2 = 0x9E3779B97F4A7C15ull;  // seed of the second (verification) tuple hash

struct GroupCols {
  const void* values[kMaxGroupCols];
  const uint32_t* validity[kMaxGroupCols];
  const void* offsets[kMaxGroupCols];
  int32_t type[kMaxGroupCols];
  int32_t n_cols;
  uint64_t key_mask;  // applied to the primary tuple hash: ~0, or fewer bits from DQ_TEST_GROUP_HASH_MASK (tests)
  const int64_t* weight;  // dq_freq_build_weighted: row r stands for weight[r] rows (<= 0: for none); else NULL
};

__device__ __forceinline__ uint64_t canon_f64(uint64_t bits) {
  const uint64_t mag = bits & 0x7FFFFFFFFFFFFFFFull;
  return mag > 0x7FF0000000000000ull ? 0x7FF8000000000000ull : bits;  // any NaN -> Double.NaN
}

// the grouping key of a fixed-width value: its exact bits (UnsafeRow's binary equality: NaN canonical, -0.0 and
// 0.0 distinct), integers sign-extended, a boolean 0 / 1
__device__ __forceinline__ uint64_t fixed_bits(int32_t type, const void* values, int64_t r) {
  switch (type) {
    case DQ_TYPE_F64: return canon_f64(reinterpret_cast<const uint64_t*>(values)[r]);
    case DQ_TYPE_I64: case DQ_TYPE_TIMESTAMP: return reinterpret_cast<const uint64_t*>(values)[r];
    case DQ_TYPE_F32: {
      const uint32_t b = reinterpret_cast<const uint32_t*>(values)[r];
      return (b & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000ull : (uint64_t)b;  // any NaN -> Float.NaN
    }
    case DQ_TYPE_I16: return (uint64_t)(int64_t)reinterpret_cast<const int16_t*>(values)[r];
    case DQ_TYPE_I8: return (uint64_t)(int64_t)reinterpret_cast<const int8_t*>(values)[r];
    case DQ_TYPE_BOOL: return (reinterpret_cast<const uint32_t*>(values)[r >> 5] >> (r & 31)) & 1u;
    default: return (uint64_t)(int64_t)reinterpret_cast<const int32_t*>(values)[r];  // IntegerType, DateType
  }
}
__device__ __forceinline__ uint64_t value_bits(const GroupCols& g, int c, int64_t r) {
  return fixed_bits(g.type[c], g.values[c], r);
}

// a DecimalType column: grouped (like strings) by a hash of its 16-byte unscaled value, checked word by word
__device__ __forceinline__ bool is_dec(int32_t t) { return DQ_TYPE_BASE(t) == DQ_TYPE_DECIMAL128; }
__device__ __forceinline__ const uint64_t* dec_at(const GroupCols& g, int c, int64_t r) {
  return reinterpret_cast<const uint64_t*>(g.values[c]) + 2 * r;
}

__device__ __forceinline__ void str_of(const GroupCols& g, int c, int64_t r, const uint8_t*& p, int64_t& len) {
  dq::str_of(g.values[c], g.offsets[c], g.type[c] == DQ_TYPE_LARGE_UTF8, r, p, len);
}

// row a of ga and row b of gb hold the same tuple: strings by length and bytes, a decimal's 16 bytes, value bits otherwise
__device__ __forceinline__ bool tuple_equal_rows(const GroupCols& ga, const GroupCols& gb, int64_t a, int64_t b) {
  for (int c = 0; c < ga.n_cols; ++c) {
    if (ga.type[c] == DQ_TYPE_UTF8 || ga.type[c] == DQ_TYPE_LARGE_UTF8) {
      const uint8_t *pa, *pb;
      int64_t la, lb;
      str_of(ga, c, a, pa, la);
      str_of(gb, c, b, pb, lb);
      if (la != lb) return false;
      if (!bytes_equal(pa, pb, la)) return false;
    } else if (is_dec(ga.type[c])) {
      const uint64_t *va = dec_at(ga, c, a), *vb = dec_at(gb, c, b);
      if (va[0] != vb[0] || va[1] != vb[1]) return false;
    } else if (value_bits(ga, c, a) != value_bits(gb, c, b)) {
      return false;
    }
  }
  return true;
}

__device__ __forceinline__ bool row_valid(const GroupCols& g, int64_t r) {
  if (g.weight && g.weight[r] <= 0) return false;
  for (int c = 0; c < g.n_cols; ++c)
    if (g.validity[c] && !((g.validity[c][r >> 5] >> (r & 31)) & 1u)) return false;
  return true;
}

// 64-bit hash of the row's tuple (columns in order; strings by bytes and length)
inline __device__ uint64_t tuple_hash(const GroupCols& g, int64_t r, uint64_t seed = kSeed) {
  uint64_t h = seed + XP5;
  for (int c = 0; c < g.n_cols; ++c) {
    if (g.type[c] == DQ_TYPE_UTF8 || g.type[c] == DQ_TYPE_LARGE_UTF8) {
      const uint8_t* p;
      int64_t len;
      str_of(g, c, r, p, len);
      h = mix_str(h, p, len);
    } else if (is_dec(g.type[c])) {
      const uint64_t* v = dec_at(g, c, r);
      h = mix8(mix8(h, v[0]), v[1]);
    } else {
      h = mix8(h, value_bits(g, c, r));
    }
  }
  return fmix64(h);
}
inline __device__ uint64_t tuple_key(const GroupCols& g, int64_t r) { return tuple_hash(g, r) & g.key_mask; }

inline __device__ bool tuple_equal(const GroupCols* chunks, uint64_t ra, uint64_t rb) {
  return tuple_equal_rows(chunks[ra >> kRowBits], chunks[rb >> kRowBits], (int64_t)(ra & ((1ull << kRowBits) - 1)),
                          (int64_t)(rb & ((1ull << kRowBits) - 1)));
}

// the scratch of every grouping call (dq_arena.h): one arena for all translation units, defined in dq_group.hip
using Frame = Arena<DeviceMem>::Frame;
Arena<DeviceMem>& group_arena();

// out[i] = i for i < n, enqueued on s (the kernel is dq_group.hip's: one copy for the units that number groups)
dq_status fill_iota_u64(uint64_t* out, int64_t n, hipStream_t s);

// out = the frame's next buffer, of `count` elements
template <typename T> dq_status take(Frame& f, T*& out, size_t count) {
  size_t want = 0;
  out = static_cast<T*>(f.take_bytes(count * sizeof(std::conditional_t<std::is_void_v<T>, char, T>), &want));
  return out ? DQ_OK : set_error(DQ_E_OOM, "hipMalloc(%zu) failed", want);
}
template <typename... T> dq_status take_each(Frame& f, size_t count, T*&... out) {  // one buffer of `count` elements each
  dq_status s = DQ_OK;
  ((s = s ? s : take(f, out, count)), ...);
  return s;
}

// *out = *src after everything enqueued on s so far (one copy, one synchronisation)
template <typename T> dq_status read_back(T* out, const void* src, hipStream_t s) {
  static_assert(std::is_trivially_copyable_v<T>, "read_back copies bytes");
  DQ_HIP(hipMemcpyAsync(out, src, sizeof(T), hipMemcpyDeviceToHost, s));
  DQ_HIP(hipStreamSynchronize(s));
  return DQ_OK;
}

// *raised = the flag a kernel may have set: the flag's 8 bytes zeroed, `launch` enqueued, the flag read back
template <typename Launch> dq_status read_flag(void* d_flag, hipStream_t s, int32_t* raised, Launch&& launch) {
  DQ_HIP(hipMemsetAsync(d_flag, 0, 8, s));
  launch();
  DQ_HIP(hipGetLastError());
  return read_back(raised, d_flag, s);
}
// f(std::true_type / std::false_type): a run-time bool as a template argument
template <typename F> void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

inline int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(8192, (n + 255) / 256)); }

// one column of a table's value store (owned: freed with it)
struct StoreCol {
  DevPtr<void> values;      // the values (fixed width) or the strings' bytes
  DevPtr<int64_t> offsets;  // strings: n + 1 offsets into values
  int64_t bytes = 0;        // length of values
};

}  // namespace dq

struct dq_freq_table {
  int32_t device = 0;
  hipStream_t stream = nullptr;
  int32_t hashed = 0;
  std::vector<int32_t> types;
  int64_t n_groups = 0;
  int64_t n_values = 0;  // rows with all grouping columns non-null
  dq::DevPtr<uint64_t> d_keys;
  dq::DevPtr<int64_t> d_counts;
  dq::DevPtr<uint64_t> d_rep;    // hashed tables built from data: one row id (chunk << 40 | row) per group
  dq::DevPtr<uint64_t> d_keys2;  // hashed tables: second tuple hash per group (merge collision check)
  // The value store of a self-contained hashed table (dq_freq_materialize, dq_freq_merge of two such tables,
  // dq_freq_from_bytes): per grouping column the n_groups representative values in group order, laid out as one more
  // input chunk without validity -- a dense array of dq_freq_elem_size(type) bytes per value (a BOOL one byte), or
  // int64 offsets[n_groups + 1] and the bytes for strings -- so that store_cols() reads group g's tuple as row g.
  bool has_store = false;
  dq::StoreCol store[dq::kMaxGroupCols];
};

namespace dq {

// the chunk descriptor of one chunk's row of views (n_cols of them); a gather of non-null rows carries no validity
inline GroupCols view_cols(const int32_t* types, int n_cols, const dq_column_view* row, uint64_t key_mask,
                           bool with_validity) {
  GroupCols g;
  std::memset(&g, 0, sizeof(g));
  g.n_cols = n_cols;
  g.key_mask = key_mask;
  for (int c = 0; c < n_cols; ++c) {
    g.values[c] = row[c].values;
    if (with_validity) g.validity[c] = reinterpret_cast<const uint32_t*>(row[c].validity);
    g.offsets[c] = row[c].offsets;
    g.type[c] = types[c];
  }
  return g;
}

// the chunk descriptor of a table's value store: group g's tuple is row g (strings have int64 offsets, a BOOL is a byte)
inline GroupCols store_cols(const dq_freq_table* t) {
  GroupCols g;
  std::memset(&g, 0, sizeof(g));
  g.n_cols = (int32_t)t->types.size();
  g.key_mask = test_hash_mask();
  for (int c = 0; c < g.n_cols; ++c) {
    const int32_t ty = t->types[c];
    g.values[c] = t->store[c].values.get();
    g.offsets[c] = t->store[c].offsets.get();
    g.type[c] = ty == DQ_TYPE_UTF8 ? DQ_TYPE_LARGE_UTF8 : ty == DQ_TYPE_BOOL ? DQ_TYPE_I8 : ty;
  }
  return g;
}

}  // namespace dq
