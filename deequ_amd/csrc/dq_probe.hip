// dq_probe.hip -- rows of other data against a frequency table (dq_freq_table.h; dq_group.hip builds it): which rows'
// groups have one member (dq_freq_unique_rows), which rows' keys the table holds and where (dq_freq_contains_rows,
// dq_freq_lookup_rows), and -- with the looked-up indices, no table -- whether a row's other columns equal those of the
// row it was matched with (dq_rows_match).  A probe finds a row's group only because it computes the row's key exactly
// as the build did: row_valid, tuple_key and value_bits are dq_freq_table.h's, the one copy both call.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "dq_freq_table.h"

namespace dq {
namespace {

// dq_freq_unique_rows: a wave takes the 64 rows of one output word at a time.  A row whose grouping columns are all
// non-null computes its key as group_compact does (HASHED: tuple_key, else the single column's value_bits), finds it
// in the table's ascending keys and reads its group's count; the ballots of "count == 1" and "non-null" are the two
// words, written by lane 0 (rows past n vote 0, so the last word's tail is 0).  The build has checked that equal keys
// are equal tuples, so a found key is the row's group; a key the table lacks raises *missing.  tot[0] / tot[1]: the
// set bits of the two bitmaps.
// SEL: a row outside the selection bitmap `sel` (one word per wave and step: word w) is in neither bitmap.
template <bool HASHED, bool SEL>
__global__ __launch_bounds__(256) void unique_rows(GroupCols g, int64_t n, const uint64_t* __restrict__ keys,
                                                   const int64_t* __restrict__ counts, int64_t G,
                                                   uint64_t* __restrict__ unique, uint64_t* __restrict__ grouped,
                                                   unsigned long long* __restrict__ tot, int32_t* __restrict__ missing,
                                                   const uint64_t* __restrict__ sel) {
  const int lane = threadIdx.x & 63;
  const int64_t words = (n + 63) >> 6;
  unsigned long long nu = 0, ng = 0;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < words; w += (int64_t)gridDim.x * 4) {
    const int64_t r = w * 64 + lane;
    bool v = r < n;
    if constexpr (SEL) v = v && ((sel[w] >> lane) & 1ull);
    v = v && row_valid(g, r);
    bool one = false;
    if (v) {
      const uint64_t k = HASHED ? tuple_key(g, r) : value_bits(g, 0, r);
      int64_t lo = 0, hi = G - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
      }
      if (G == 0 || keys[lo] != k) atomicOr(missing, 1);
      else one = counts[lo] == 1;
    }
    const uint64_t bu = __builtin_amdgcn_ballot_w64(one), bg = __builtin_amdgcn_ballot_w64(v);
    if (lane == 0) {
      unique[w] = bu;
      if (grouped) grouped[w] = bg;
      nu += (unsigned long long)__builtin_popcountll(bu);
      ng += (unsigned long long)__builtin_popcountll(bg);
    }
  }
  if (lane == 0 && (nu | ng)) {
    atomicAdd(&tot[0], nu);
    atomicAdd(&tot[1], ng);
  }
}

// dq_freq_contains_rows: the probe of foreign data, where a key the table lacks is the answer.  The search of the
// table's ascending keys starts in LDS: contains_splitters takes n_split = min(kSplitters, G) evenly spaced keys once
// per call (splitter b = keys[b * G / n_split], the first key of bucket b), every workgroup of contains_rows copies
// them into LDS, a row finds its bucket there (the last splitter <= its key) and finishes in the bucket's
// ceil(G / n_split) keys in global memory -- log2(G) - 11 dependent global loads instead of log2(G); none when the
// key is a splitter (every key of a table of at most kSplitters groups is).
constexpr int kSplitters = 2048;       // 16 KiB of LDS per 256-thread workgroup: 8 workgroups per CU fit in 160 KiB
constexpr int kContainsMaxGrid = 2048; // workgroups (each reads the splitters once: 32 MiB from L2 at most)
__global__ void contains_splitters(const uint64_t* __restrict__ keys, int64_t G, int n_split,
                                   uint64_t* __restrict__ split) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n_split) split[b] = keys[((int64_t)b * G) / n_split];
}
// A wave takes the 64 rows of one output word at a time, as unique_rows.  A row applies when the filter (NULL: every
// row) has its bit; a row that applies and whose key columns are all non-null computes its key as group_compact does
// and looks it up.  HASHED: nothing has verified that a found hash is this row's tuple, so the row's tuple is compared
// by value with the group's stored tuple (row `pos` of the table's store `st`); a different tuple is not contained.
// GROUP (dq_freq_lookup_rows): every row also stores WHICH group it hit -- group[r] = its index in the table's sorted
// keys, -1 for a row that is not contained -- beside the ballot; no bitmap is written, tot[0] counts the found rows.
template <bool HASHED, bool GROUP>
__global__ __launch_bounds__(256) void contains_rows(GroupCols g, GroupCols st, int64_t n,
                                                     const uint64_t* __restrict__ filter,
                                                     const uint64_t* __restrict__ keys, int64_t G,
                                                     const uint64_t* __restrict__ split, int n_split,
                                                     uint64_t* __restrict__ contained, uint64_t* __restrict__ applies,
                                                     int32_t* __restrict__ group, unsigned long long* __restrict__ tot) {
  __shared__ uint64_t sp[kSplitters];
  for (int i = threadIdx.x; i < n_split; i += blockDim.x) sp[i] = split[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t words = (n + 63) >> 6;
  unsigned long long nc = 0, na = 0;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < words; w += (int64_t)gridDim.x * 4) {
    const int64_t r = w * 64 + lane;
    const bool a = r < n && (!filter || ((filter[w] >> lane) & 1ull));
    bool found = false;
    [[maybe_unused]] int32_t hit = -1;
    if (a && row_valid(g, r)) {
      const uint64_t k = HASHED ? tuple_key(g, r) : value_bits(g, 0, r);
      int b = 0;  // the number of splitters <= k
      for (int len = n_split; len > 0;) {
        const int half = len >> 1;
        if (sp[b + half] <= k) {
          b += half + 1;
          len -= half + 1;
        } else {
          len = half;
        }
      }
      if (b > 0) {  // (k below the first key, or an empty table: no bucket)
        --b;
        int64_t lo = ((int64_t)b * G) / n_split;
        if (sp[b] != k) {  // the bucket's other keys: lo + 1 .. the next bucket's first key
          int64_t hi = ((int64_t)(b + 1) * G) / n_split - 1;
          ++lo;
          if (lo > hi) {
            lo = -1;
          } else {
            while (lo < hi) {
              const int64_t mid = (lo + hi) >> 1;
              if (keys[mid] < k) lo = mid + 1;
              else hi = mid;
            }
            if (keys[lo] != k) lo = -1;
          }
        }
        found = lo >= 0 && (!HASHED || tuple_equal_rows(g, st, r, lo));
        if constexpr (GROUP) hit = found ? (int32_t)lo : -1;
      }
    }
    const uint64_t bc = __builtin_amdgcn_ballot_w64(found), ba = __builtin_amdgcn_ballot_w64(a);
    if constexpr (GROUP) {
      if (r < n) group[r] = hit;
    }
    if (lane == 0) {
      if constexpr (!GROUP) {
        contained[w] = bc;
        if (applies) applies[w] = ba;
      }
      nc += (unsigned long long)__builtin_popcountll(bc);
      na += (unsigned long long)__builtin_popcountll(ba);
    }
  }
  if (lane == 0 && (nc | na)) {
    atomicAdd(&tot[0], nc);
    atomicAdd(&tot[1], na);
  }
}

// dq_rows_match: a probe row's compare columns against payload row group[r] (the reference's row with the same key).
// One wave per 64-row output word, lane per row, as contains_rows; a workgroup keeps its totals in LDS and adds them
// to the launch's with at most 3 + n_cols global atomics, and the grid is capped, so the atomics do not grow with the
// chunk.  The columns are walked uniformly by the wave (the descriptors are scalar loads); a lane whose row is not
// found, or -- when the per-column counts are not wanted -- has already differed, loads nothing more, and the wave
// leaves the walk when no lane is left.
constexpr int kMaxMatchCols = 16;
constexpr int kMatchMaxGrid = 2048;  // workgroups of 4 waves
struct MatchCols {
  const void* values[kMaxMatchCols];
  const uint32_t* validity[kMaxMatchCols];
  const void* offsets[kMaxMatchCols];
  int32_t type[kMaxMatchCols];
};
__host__ __device__ inline bool is_str(int32_t t) { return t == DQ_TYPE_UTF8 || t == DQ_TYPE_LARGE_UTF8; }
// null-safe equality of column c: row r of a, row q of p.  NULL = NULL, NULL != any value, and the bytes under a NULL
// slot are never loaded; values by tuple_equal_rows' rule (the two sides of a string column may differ in offset width)
__device__ __forceinline__ bool match_equal(const MatchCols& a, const MatchCols& p, int c, int64_t r, int64_t q) {
  const bool va = !a.validity[c] || ((a.validity[c][r >> 5] >> (r & 31)) & 1u);
  const bool vp = !p.validity[c] || ((p.validity[c][q >> 5] >> (q & 31)) & 1u);
  if (!va || !vp) return va == vp;
  const int32_t ta = a.type[c], tp = p.type[c];
  if (is_str(ta)) {
    const uint8_t *pa, *pb;
    int64_t la, lb;
    dq::str_of(a.values[c], a.offsets[c], ta == DQ_TYPE_LARGE_UTF8, r, pa, la);
    dq::str_of(p.values[c], p.offsets[c], tp == DQ_TYPE_LARGE_UTF8, q, pb, lb);
    return la == lb && bytes_equal(pa, pb, la);
  }
  if (is_dec(ta)) {
    const uint64_t* xa = reinterpret_cast<const uint64_t*>(a.values[c]) + 2 * r;
    const uint64_t* xp = reinterpret_cast<const uint64_t*>(p.values[c]) + 2 * q;
    return xa[0] == xp[0] && xa[1] == xp[1];
  }
  return fixed_bits(ta, a.values[c], r) == fixed_bits(tp, p.values[c], q);
}
// tot: [0] matched, [1] found, [2] applies, [3 + c] the found rows whose column c differs (PER_COL)
template <bool PER_COL>
__global__ __launch_bounds__(256) void rows_match(MatchCols a, MatchCols p, int n_cols, int64_t n, int64_t n_payload,
                                                  const int32_t* __restrict__ group,
                                                  const uint64_t* __restrict__ filter, uint64_t* __restrict__ matched,
                                                  uint64_t* __restrict__ found, uint64_t* __restrict__ applies,
                                                  unsigned long long* __restrict__ tot) {
  __shared__ unsigned int cnt[3 + kMaxMatchCols];  // (a workgroup sees fewer than 2^31 rows)
  if (threadIdx.x < 3 + kMaxMatchCols) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t words = (n + 63) >> 6;
  unsigned int nm = 0, nf = 0, na = 0;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < words; w += (int64_t)gridDim.x * 4) {
    const int64_t r = w * 64 + lane;
    const bool ap = r < n && (!filter || ((filter[w] >> lane) & 1ull));
    int64_t q = -1;
    if (ap) q = group[r];
    const bool f = q >= 0 && q < n_payload;  // (an index past the payload addresses nothing: not found)
    bool eq = f;
    for (int c = 0; c < n_cols; ++c) {
      if constexpr (PER_COL) {
        const bool differs = f && !match_equal(a, p, c, r, q);
        eq = eq && !differs;
        const uint64_t bd = __builtin_amdgcn_ballot_w64(differs);
        if (lane == 0 && bd) atomicAdd(&cnt[3 + c], (unsigned int)__builtin_popcountll(bd));
      } else {
        if (!__builtin_amdgcn_ballot_w64(eq)) break;
        if (eq) eq = match_equal(a, p, c, r, q);
      }
    }
    const uint64_t bm = __builtin_amdgcn_ballot_w64(eq), bf = __builtin_amdgcn_ballot_w64(f),
                   ba = __builtin_amdgcn_ballot_w64(ap);
    if (lane == 0) {
      matched[w] = bm;
      if (found) found[w] = bf;
      if (applies) applies[w] = ba;
      nm += (unsigned int)__builtin_popcountll(bm);
      nf += (unsigned int)__builtin_popcountll(bf);
      na += (unsigned int)__builtin_popcountll(ba);
    }
  }
  if (lane == 0) {
    if (nm) atomicAdd(&cnt[0], nm);
    if (nf) atomicAdd(&cnt[1], nf);
    if (na) atomicAdd(&cnt[2], na);
  }
  __syncthreads();
  if (threadIdx.x < 3 + n_cols && cnt[threadIdx.x]) atomicAdd(&tot[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// Column c of a probe (type ty, view v) is the column it is probed against (`theirs`: the "table" or the "payload",
// whose column has type *ref): the same type (a decimal's precision and scale are part of its code), or a string
// column of the other offset width -- the probe hashes and compares what the build hashed, nothing is widened -- and
// a type code this library knows (every table's are).  Then the view: values present and 4-byte aligned, validity
// 4-byte aligned, offsets present for strings.  ref NULL: the types are checked already; v NULL: the type only.
dq_status check_probe_col(const char* me, const char* theirs, int c, int32_t ty, const int32_t* ref,
                          const dq_column_view* v) {
  auto known = [](int32_t t) {
    const int32_t b = DQ_TYPE_BASE(t);
    return b >= DQ_TYPE_F64 && b <= DQ_TYPE_DECIMAL128 && (b == DQ_TYPE_DECIMAL128 || t == b);
  };
  if (ref && (!known(ty) || !known(*ref) || (ty != *ref && !(is_str(ty) && is_str(*ref)))))
    return set_error(DQ_E_INVALID, "%s: column %d has type %d, the %s's has %d", me, c, ty, theirs, *ref);
  if (v && (!v->values || ((uintptr_t)v->values & 3) || ((uintptr_t)v->validity & 3) || (is_str(ty) && !v->offsets)))
    return set_error(DQ_E_INVALID, "%s: column %d: missing or misaligned buffer", me, c);
  return DQ_OK;
}

dq_status unique_rows_impl(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols,
                           int64_t n_rows, const uint64_t* selection, uint64_t* unique, uint64_t* grouped,
                           void* hip_stream, int64_t* num_unique, int64_t* num_grouped) {
  if (!t) return set_error(DQ_E_INVALID, "dq_freq_unique_rows: table is NULL");
  if (n_rows < 0 || n_rows >= (1ll << 31)) return set_error(DQ_E_INVALID, "dq_freq_unique_rows: 0 <= n_rows < 2^31");
  if (n_rows == 0) {
    if (num_unique) *num_unique = 0;
    if (num_grouped) *num_grouped = 0;
    return DQ_OK;
  }
  const int n_cols = (int)t->types.size();
  if (!cols) return set_error(DQ_E_INVALID, "dq_freq_unique_rows: cols is NULL");
  if (!unique || ((uintptr_t)unique & 7) || ((uintptr_t)grouped & 7) || ((uintptr_t)selection & 7))
    return set_error(DQ_E_INVALID, "dq_freq_unique_rows: the bitmaps must be 8-byte aligned device buffers");
  std::vector<int32_t> ty(t->types);
  for (int c = 0; c < n_cols; ++c) {
    if (types) ty[c] = types[c];
    if (dq_status s = check_probe_col("dq_freq_unique_rows", "table", c, ty[c], &t->types[c], &cols[c])) return s;
  }
  DQ_HIP(hipSetDevice(t->device));
  const hipStream_t S = reinterpret_cast<hipStream_t>(hip_stream);
  const GroupCols g = view_cols(ty.data(), n_cols, cols, test_hash_mask(), true);
  Frame fr(group_arena(), t->device);
  unsigned long long* d_out = nullptr;  // tot[2], then the missing flag
  if (dq_status s = take(fr, d_out, 4)) return s;
  DQ_HIP(hipMemsetAsync(d_out, 0, 4 * sizeof(unsigned long long), S));
  const int64_t words = (n_rows + 63) / 64;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(8192, (words + 3) / 4));
  with_bool(t->hashed != 0, [&](auto hashed) {
    with_bool(selection != nullptr, [&](auto filtered) {
      hipLaunchKernelGGL((unique_rows<decltype(hashed)::value, decltype(filtered)::value>), dim3(grid), dim3(256), 0, S, g,
                         n_rows, t->d_keys.get(), t->d_counts.get(), t->n_groups, unique, grouped, d_out,
                         reinterpret_cast<int32_t*>(d_out + 2), selection);
    });
  });
  DQ_HIP(hipGetLastError());
  unsigned long long h[4];
  if (dq_status s = read_back(&h, d_out, S)) return s;
  if (h[2]) return set_error(DQ_E_INVALID, "dq_freq_unique_rows: a row whose key is no group of the table (built from other data)");
  if (num_unique) *num_unique = (int64_t)h[0];
  if (num_grouped) *num_grouped = (int64_t)h[1];
  return DQ_OK;
}

// dq_freq_contains_rows (group NULL: the bitmaps) and dq_freq_lookup_rows (group: the index of every row's group, no
// bitmap) are one search: the same checks in the same order, the same splitters, the same kernel
dq_status contains_impl(const char* me, const dq_freq_table* t, const int32_t* types, const dq_column_view* cols,
                        int64_t n_rows, const uint64_t* filter, uint64_t* contained, uint64_t* applies,
                        int32_t* group, bool lookup, void* hip_stream, int64_t* num_contained,
                        int64_t* num_applies) {
  // the arguments that need no table first, then the table, then what the table says about the columns: all of it
  // before anything touches the device
  if (n_rows < 0 || n_rows >= (1ll << 31)) return set_error(DQ_E_INVALID, "%s: 0 <= n_rows < 2^31", me);
  if (((uintptr_t)contained & 7) || ((uintptr_t)applies & 7) || ((uintptr_t)filter & 7))
    return set_error(DQ_E_INVALID, "%s: the bitmaps must be 8-byte aligned device buffers", me);
  if ((uintptr_t)group & 3) return set_error(DQ_E_INVALID, "%s: group must be a 4-byte aligned device buffer", me);
  if (n_rows > 0 && !lookup && !contained) return set_error(DQ_E_INVALID, "%s: contained is NULL", me);
  if (n_rows > 0 && lookup && !group) return set_error(DQ_E_INVALID, "%s: group is NULL", me);
  if (n_rows > 0 && !cols) return set_error(DQ_E_INVALID, "%s: cols is NULL", me);
  if (!t) return set_error(DQ_E_INVALID, "%s: table is NULL", me);
  if (lookup && t->n_groups > INT32_MAX)
    return set_error(DQ_E_UNSUPPORTED, "%s: the table has %lld groups, a group index is 32 bits (2^31 - 1 at most)", me,
                     (long long)t->n_groups);
  if (n_rows == 0) {
    if (num_contained) *num_contained = 0;
    if (num_applies) *num_applies = 0;
    return DQ_OK;
  }
  if (t->hashed && !t->has_store)
    return set_error(DQ_E_STATE, "%s: the table does not own its values (dq_freq_materialize it "
                                 "first): a found hash is compared with the group's stored tuple", me);
  const int n_cols = (int)t->types.size();
  std::vector<int32_t> ty(t->types);
  for (int c = 0; c < n_cols; ++c) {
    if (types) ty[c] = types[c];
    if (dq_status s = check_probe_col(me, "table", c, ty[c], &t->types[c], &cols[c])) return s;
  }
  DQ_HIP(hipSetDevice(t->device));
  const hipStream_t S = reinterpret_cast<hipStream_t>(hip_stream);
  const GroupCols g = view_cols(ty.data(), n_cols, cols, test_hash_mask(), true);
  GroupCols st;
  std::memset(&st, 0, sizeof(st));
  if (t->hashed) st = store_cols(t);
  Frame fr(group_arena(), t->device);
  unsigned long long* d_tot = nullptr;
  uint64_t* d_split = nullptr;
  if (dq_status s = take(fr, d_tot, 2)) return s;
  if (dq_status s = take(fr, d_split, kSplitters)) return s;
  DQ_HIP(hipMemsetAsync(d_tot, 0, 2 * sizeof(unsigned long long), S));
  const int64_t G = t->n_groups;
  const int n_split = (int)std::min<int64_t>(kSplitters, G);
  if (n_split > 0) {
    hipLaunchKernelGGL(contains_splitters, dim3((n_split + 255) / 256), dim3(256), 0, S, t->d_keys.get(), G, n_split,
                       d_split);
    DQ_HIP(hipGetLastError());
  }
  const int64_t words = (n_rows + 63) / 64;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(kContainsMaxGrid, (words + 3) / 4));
  with_bool(t->hashed != 0, [&](auto hashed) {
    with_bool(lookup, [&](auto with_group) {
      hipLaunchKernelGGL((contains_rows<decltype(hashed)::value, decltype(with_group)::value>), dim3(grid), dim3(256), 0,
                         S, g, st, n_rows, filter, t->d_keys.get(), G, d_split, n_split, contained, applies, group,
                         d_tot);
    });
  });
  DQ_HIP(hipGetLastError());
  unsigned long long h[2];
  if (dq_status s = read_back(&h, d_tot, S)) return s;
  if (num_contained) *num_contained = (int64_t)h[0];
  if (num_applies) *num_applies = (int64_t)h[1];
  return DQ_OK;
}

}  // namespace
}  // namespace dq

using namespace dq;

extern "C" {

dq_status dq_freq_unique_rows(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols, int64_t n_rows,
                              uint64_t* unique, uint64_t* grouped, void* hip_stream, int64_t* num_unique,
                              int64_t* num_grouped) {
  return unique_rows_impl(t, types, cols, n_rows, nullptr, unique, grouped, hip_stream, num_unique, num_grouped);
}

dq_status dq_freq_unique_rows_where(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols,
                                    int64_t n_rows, const uint64_t* selection, uint64_t* unique, uint64_t* grouped,
                                    void* hip_stream, int64_t* num_unique, int64_t* num_grouped) {
  return unique_rows_impl(t, types, cols, n_rows, selection, unique, grouped, hip_stream, num_unique, num_grouped);
}

dq_status dq_freq_contains_rows(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols,
                                int64_t n_rows, const uint64_t* filter, uint64_t* contained, uint64_t* applies,
                                void* hip_stream, int64_t* num_contained, int64_t* num_applies) {
  return contains_impl("dq_freq_contains_rows", t, types, cols, n_rows, filter, contained, applies, nullptr, false,
                       hip_stream, num_contained, num_applies);
}

dq_status dq_freq_lookup_rows(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols, int64_t n_rows,
                              const uint64_t* filter, int32_t* group, void* hip_stream, int64_t* num_found) {
  return contains_impl("dq_freq_lookup_rows", t, types, cols, n_rows, filter, nullptr, nullptr, group, true, hip_stream,
                       num_found, nullptr);
}

dq_status dq_rows_match(const int32_t* types, const dq_column_view* cols, const int32_t* payload_types,
                        const dq_column_view* payload, int32_t n_cols, int64_t n_rows, int64_t n_payload_rows,
                        const int32_t* group, const uint64_t* filter, uint64_t* matched, uint64_t* found,
                        uint64_t* applies, int32_t device, void* hip_stream, int64_t* num_matched, int64_t* num_found,
                        int64_t* num_applies, int64_t* num_mismatch) {
  const char* me = "dq_rows_match";
  if (n_cols < 1 || n_cols > kMaxMatchCols)
    return set_error(DQ_E_INVALID, "%s: 1 <= n_cols <= %d, got %d", me, kMaxMatchCols, n_cols);
  if (n_rows < 0 || n_rows >= (1ll << 31)) return set_error(DQ_E_INVALID, "%s: 0 <= n_rows < 2^31", me);
  if (n_payload_rows < 0) return set_error(DQ_E_INVALID, "%s: n_payload_rows < 0", me);
  if (((uintptr_t)matched & 7) || ((uintptr_t)found & 7) || ((uintptr_t)applies & 7) || ((uintptr_t)filter & 7))
    return set_error(DQ_E_INVALID, "%s: the bitmaps must be 8-byte aligned device buffers", me);
  if ((uintptr_t)group & 3) return set_error(DQ_E_INVALID, "%s: group must be a 4-byte aligned device buffer", me);
  if (!types || !payload_types) return set_error(DQ_E_INVALID, "%s: types is NULL", me);
  if (n_rows > 0 && !matched) return set_error(DQ_E_INVALID, "%s: matched is NULL", me);
  if (n_rows > 0 && !group) return set_error(DQ_E_INVALID, "%s: group is NULL", me);
  if (n_rows > 0 && (!cols || !payload)) return set_error(DQ_E_INVALID, "%s: cols is NULL", me);
  for (int c = 0; c < n_cols; ++c)
    if (dq_status s = check_probe_col(me, "payload", c, types[c], &payload_types[c], nullptr)) return s;
  MatchCols a, p;
  std::memset(&a, 0, sizeof(a));
  std::memset(&p, 0, sizeof(p));
  for (int c = 0; n_rows > 0 && c < n_cols; ++c) {
    const dq_column_view &v = cols[c], &u = payload[c];
    if (dq_status s = check_probe_col(me, "payload", c, types[c], nullptr, &v)) return s;
    if (((uintptr_t)u.values & 3) || ((uintptr_t)u.validity & 3) ||
        (n_payload_rows > 0 && (!u.values || (is_str(payload_types[c]) && !u.offsets))))
      return set_error(DQ_E_INVALID, "%s: payload column %d: missing or misaligned buffer", me, c);
    a.values[c] = v.values, a.validity[c] = reinterpret_cast<const uint32_t*>(v.validity), a.offsets[c] = v.offsets;
    p.values[c] = u.values, p.validity[c] = reinterpret_cast<const uint32_t*>(u.validity), p.offsets[c] = u.offsets;
    a.type[c] = types[c], p.type[c] = payload_types[c];
  }
  if (n_rows == 0) {
    if (num_matched) *num_matched = 0;
    if (num_found) *num_found = 0;
    if (num_applies) *num_applies = 0;
    for (int c = 0; num_mismatch && c < n_cols; ++c) num_mismatch[c] = 0;
    return DQ_OK;
  }
  DQ_HIP(hipSetDevice(device));
  const hipStream_t S = reinterpret_cast<hipStream_t>(hip_stream);
  Frame fr(group_arena(), device);
  unsigned long long* d_tot = nullptr;
  constexpr int kTot = 3 + kMaxMatchCols;
  if (dq_status s = take(fr, d_tot, kTot)) return s;
  DQ_HIP(hipMemsetAsync(d_tot, 0, kTot * sizeof(unsigned long long), S));
  const int64_t words = (n_rows + 63) / 64;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(kMatchMaxGrid, (words + 3) / 4));
  with_bool(num_mismatch != nullptr, [&](auto per_col) {
    hipLaunchKernelGGL(rows_match<decltype(per_col)::value>, dim3(grid), dim3(256), 0, S, a, p, (int)n_cols, n_rows,
                       n_payload_rows, group, filter, matched, found, applies, d_tot);
  });
  DQ_HIP(hipGetLastError());
  unsigned long long h[kTot];
  if (dq_status s = read_back(&h, d_tot, S)) return s;
  if (num_matched) *num_matched = (int64_t)h[0];
  if (num_found) *num_found = (int64_t)h[1];
  if (num_applies) *num_applies = (int64_t)h[2];
  for (int c = 0; num_mismatch && c < n_cols; ++c) num_mismatch[c] = (int64_t)h[3 + c];
  return DQ_OK;
}

}  // extern "C"
