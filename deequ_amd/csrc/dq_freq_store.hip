// dq_freq_store.hip -- a frequency table (dq_freq_table.h; dq_group.hip builds it) as a persisted state: the merge of
// two tables, the value store that makes a hashed table self-contained, and the table's byte image.
//
// dq_freq_merge is FrequenciesAndNumRows.sum (GroupingAnalyzers.scala:118-138), an outer join adding counts.  It no
// longer has the rows, so two distinct tuples whose first hashes collide are told apart by their stored tuples when
// both tables own their values, else by the second hash every hashed table keeps per group (equal first hash,
// different second hash: DQ_E_UNSUPPORTED) -- never by adding their counts.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "dq_freq_image.h"
#include "dq_freq_table.h"
#include "dq_prim.h"

namespace dq {
namespace {

// merge of hashed tables: (second hash, count) in first-hash order; equal first hashes with different
// second hashes are distinct tuples
__global__ void merge_gather_check(const uint64_t* __restrict__ k1s, const uint64_t* __restrict__ pos,
                                   const uint64_t* __restrict__ k2, const int64_t* __restrict__ c, int64_t n,
                                   uint64_t* __restrict__ k2s, int64_t* __restrict__ cs, int32_t* __restrict__ collision) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t p = pos[i];
    k2s[i] = k2[p];
    cs[i] = c[p];
    if (i > 0 && k1s[i] == k1s[i - 1] && k2[p] != k2[pos[i - 1]]) atomicOr(collision, 1);
  }
}

// ---- the value store: gathers of representative tuples (dq_freq_materialize, dq_freq_merge, dq_freq_take_values) ----
// A gather reads row ids (chunk << 40 | row) against an array of chunk descriptors: the caller's input chunks, or the
// stores of one or two tables (a store is one more chunk; row = group).

// every row id names a chunk below n_chunks and a row below its chunk's row count
__global__ void rep_check(const uint64_t* __restrict__ rep, int64_t G, const int64_t* __restrict__ chunk_rows,
                          int32_t n_chunks, int32_t* __restrict__ bad) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t r = rep[g], k = r >> kRowBits;
    if (k >= (uint64_t)n_chunks || (int64_t)(r & ((1ull << kRowBits) - 1)) >= chunk_rows[k]) atomicOr(bad, 1);
  }
}

// out[g] = column c's value at row id rep[g]; es = bytes per stored value (a bit-packed BOOL becomes one byte)
__global__ void gather_fixed(const uint64_t* __restrict__ rep, int64_t G, const GroupCols* __restrict__ chunks, int c, int es,
                             void* __restrict__ out) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t r = rep[g];
    const GroupCols& gc = chunks[r >> kRowBits];
    const int64_t lr = (int64_t)(r & ((1ull << kRowBits) - 1));
    const void* v = gc.values[c];
    if (gc.type[c] == DQ_TYPE_BOOL) {
      reinterpret_cast<uint8_t*>(out)[g] = (uint8_t)((reinterpret_cast<const uint32_t*>(v)[lr >> 5] >> (lr & 31)) & 1u);
    } else if (es == 16) {
      reinterpret_cast<uint64_t*>(out)[2 * g] = reinterpret_cast<const uint64_t*>(v)[2 * lr];
      reinterpret_cast<uint64_t*>(out)[2 * g + 1] = reinterpret_cast<const uint64_t*>(v)[2 * lr + 1];
    } else if (es == 8) {
      reinterpret_cast<uint64_t*>(out)[g] = reinterpret_cast<const uint64_t*>(v)[lr];
    } else if (es == 4) {
      reinterpret_cast<uint32_t*>(out)[g] = reinterpret_cast<const uint32_t*>(v)[lr];
    } else if (es == 2) {
      reinterpret_cast<uint16_t*>(out)[g] = reinterpret_cast<const uint16_t*>(v)[lr];
    } else {
      reinterpret_cast<uint8_t*>(out)[g] = reinterpret_cast<const uint8_t*>(v)[lr];
    }
  }
}

// lens[g] = byte length of string column c at row id rep[g] (random reads of the offsets); lens[G] = 0, so that the
// exclusive sum over G + 1 entries leaves the offsets array, its last entry the byte total
__global__ void gather_str_lens(const uint64_t* __restrict__ rep, int64_t G, const GroupCols* __restrict__ chunks, int c,
                                int64_t* __restrict__ lens) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= G; g += (int64_t)gridDim.x * blockDim.x) {
    int64_t len = 0;
    if (g < G) {
      const uint64_t r = rep[g];
      const uint8_t* p;
      str_of(chunks[r >> kRowBits], c, (int64_t)(r & ((1ull << kRowBits) - 1)), p, len);
    }
    lens[g] = len;
  }
}

// one lane copies one short string: 8 bytes, then 4, then single bytes per step by unaligned loads and stores (as
// mix_str reads them); nothing is read or written outside [p, p + len) / [d, d + len)
__device__ __forceinline__ void copy_lane(uint8_t* __restrict__ d, const uint8_t* __restrict__ p, int64_t len) {
  int64_t i = 0;
  for (; i + 8 <= len; i += 8) *reinterpret_cast<strkey_u64u*>(d + i) = *reinterpret_cast<const strkey_u64u*>(p + i);
  if (i + 4 <= len) {
    *reinterpret_cast<strkey_u32u*>(d + i) = *reinterpret_cast<const strkey_u32u*>(p + i);
    i += 4;
  }
  for (; i < len; ++i) d[i] = p[i];
}
// the wave copies one long string (d, p, len wave-uniform): single bytes up to the destination's next 8-byte
// boundary, then 64 x 8 bytes per step (aligned stores, unaligned loads), then the last < 8 bytes
__device__ __forceinline__ void copy_wave(uint8_t* __restrict__ d, const uint8_t* __restrict__ p, int64_t len, int lane) {
  int64_t head = (int64_t)((8 - (reinterpret_cast<uintptr_t>(d) & 7)) & 7);
  if (head > len) head = len;
  if (lane < head) d[lane] = p[lane];
  d += head;
  p += head;
  len -= head;
  const int64_t body = len & ~(int64_t)7;
  for (int64_t i = (int64_t)lane * 8; i < body; i += 512)
    *reinterpret_cast<uint64_t*>(d + i) = *reinterpret_cast<const strkey_u64u*>(p + i);
  if (body + lane < len) d[body + lane] = p[body + lane];
}
constexpr int kWaveCopyLen = 40;  // strings of at least this many bytes take the wave path (the sweep)
// out[offs[g] ..) = the bytes of string column c at row id rep[g].  A wave takes 64 consecutive groups: each lane
// copies its own string when it is shorter than wave_len; the longer ones are then copied one after the other by
// the whole wave (their descriptors broadcast from the owning lane).
__global__ __launch_bounds__(256) void gather_str_bytes(const uint64_t* __restrict__ rep, int64_t G,
                                                        const GroupCols* __restrict__ chunks, int c,
                                                        const int64_t* __restrict__ offs, uint8_t* __restrict__ out,
                                                        int64_t wave_len) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;  // a multiple of 64: i0 is wave-uniform
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < G; i0 += stride) {
    const int64_t g = i0 + lane;
    const uint8_t* p = nullptr;
    uint8_t* d = out;
    int64_t len = 0;
    if (g < G) {
      const uint64_t r = rep[g];
      str_of(chunks[r >> kRowBits], c, (int64_t)(r & ((1ull << kRowBits) - 1)), p, len);
      d = out + offs[g];
    }
    const bool coop = len >= wave_len;
    if (!coop) copy_lane(d, p, len);
    uint64_t m = __builtin_amdgcn_ballot_w64(coop);
    while (m) {
      const int src = __builtin_ctzll(m);
      m &= m - 1;
      const uint64_t sp = __shfl((unsigned long long)reinterpret_cast<uintptr_t>(p), src);
      const uint64_t sd = __shfl((unsigned long long)reinterpret_cast<uintptr_t>(d), src);
      const int64_t sl = (int64_t)__shfl((unsigned long long)len, src);
      copy_wave(reinterpret_cast<uint8_t*>(sd), reinterpret_cast<const uint8_t*>(sp), sl, lane);
    }
  }
}

// merge of two self-contained hashed tables: as merge_gather_check, but members of a run of equal first hashes are
// compared value by value through the two stores (chunks[0] = a's, chunks[1] = b's; position p of the concatenated
// groups is row p of a, or row p - na of b)
__device__ __forceinline__ uint64_t merge_row_id(uint64_t p, int64_t na) {
  return p < (uint64_t)na ? p : ((1ull << kRowBits) | (p - (uint64_t)na));
}
__global__ void merge_gather_check_values(const uint64_t* __restrict__ k1s, const uint64_t* __restrict__ pos,
                                          const uint64_t* __restrict__ k2, const int64_t* __restrict__ c, int64_t n,
                                          int64_t na, const GroupCols* __restrict__ chunks, uint64_t* __restrict__ k2s,
                                          int64_t* __restrict__ cs, int32_t* __restrict__ collision) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t p = pos[i];
    k2s[i] = k2[p];
    cs[i] = c[p];
    if (i > 0 && k1s[i] == k1s[i - 1] && !tuple_equal(chunks, merge_row_id(p, na), merge_row_id(pos[i - 1], na)))
      atomicOr(collision, 1);
  }
}
__global__ void merge_row_ids(uint64_t* __restrict__ pos, int64_t n, int64_t na) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    pos[i] = merge_row_id(pos[i], na);
}

// idx[i] = the group whose key is want[i] (binary search of the table's ascending keys); a key the table lacks
// raises *missing
__global__ void find_groups(const uint64_t* __restrict__ want, int32_t n, const uint64_t* __restrict__ keys, int64_t G,
                            uint64_t* __restrict__ idx, int32_t* __restrict__ missing) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = want[i];
  int64_t lo = 0, hi = G - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  idx[i] = (uint64_t)lo;
  if (G == 0 || keys[lo] != k) atomicOr(missing, 1);
}

int64_t wave_copy_len() {  // DQ_FREQ_WAVE_COPY: the lane / wave switch length of the string gather (sweeps)
  const char* e = std::getenv("DQ_FREQ_WAVE_COPY");  // (read per call: tools/freq_state_bench.py sweeps it)
  const long long v = e ? std::atoll(e) : 0;
  return v > 0 ? v : kWaveCopyLen;
}

// Column c (type code `type`) of the tuples at row ids d_rep[0 .. G) of the chunks d_chunks, gathered into *out
// (allocated here, owned by the caller's StoreCol).  The caller has checked the row ids; scan_tmp is its frame's
// buffer of prim::scan_temp_bytes(G + 1) bytes (one for all the columns it gathers).
dq_status gather_column(hipStream_t S, const GroupCols* d_chunks, const uint64_t* d_rep, int64_t G, int c,
                        int32_t type, void* scan_tmp, StoreCol* out) {
  const int es = dq_freq_elem_size(type);
  if (es < 0) return set_error(DQ_E_TYPE, "frequency table: unknown type code %d", type);
  if (es > 0) {
    out->bytes = G * es;
    DQ_HIP(out->values.alloc(std::max<int64_t>(8, out->bytes)));
    if (G > 0) {
      hipLaunchKernelGGL(gather_fixed, dim3(grid_for(G)), dim3(256), 0, S, d_rep, G, d_chunks, c, es, out->values.get());
      DQ_HIP(hipGetLastError());
    }
    return DQ_OK;
  }
  DQ_HIP(out->offsets.alloc(G + 1));
  int64_t* const offs = out->offsets.get();
  hipLaunchKernelGGL(gather_str_lens, dim3(grid_for(G + 1)), dim3(256), 0, S, d_rep, G, d_chunks, c, offs);
  DQ_HIP(hipGetLastError());
  DQ_HIP(prim::exclusive_sum_i64(offs, offs, G + 1, scan_tmp, S));
  if (dq_status s = read_back(&out->bytes, offs + G, S)) return s;
  DQ_HIP(out->values.alloc(std::max<int64_t>(8, out->bytes)));
  if (G > 0 && out->bytes > 0) {
    hipLaunchKernelGGL(gather_str_bytes, dim3(grid_for(G)), dim3(256), 0, S, d_rep, G, d_chunks, c, offs,
                       out->values.as<uint8_t>(), wave_copy_len());
    DQ_HIP(hipGetLastError());
  }
  return DQ_OK;
}

// the sections of t's image (offsets as FreqImageView), its total length returned
int64_t image_layout(const dq_freq_table* t, FreqImageView* v) {
  const int n_cols = (int)t->types.size();
  const int64_t G = t->n_groups;
  v->n_cols = n_cols;
  v->hashed = t->hashed;
  v->n_groups = G;
  v->n_values = t->n_values;
  int64_t at = freq_image_header_bytes(n_cols);
  v->keys = at;
  v->counts = at + 8 * G;
  v->keys2 = t->hashed ? at + 16 * G : 0;
  at += (t->hashed ? 24 : 16) * G;
  for (int c = 0; c < n_cols && t->hashed; ++c) {
    v->types[c] = t->types[c];
    if (t->store[c].offsets) {
      v->col_offsets[c] = at + 8;
      at += 8 + 8 * (G + 1);
    }
    v->col_values[c] = at;
    v->col_bytes[c] = t->store[c].bytes;
    at += freq_image_pad8(t->store[c].bytes);
  }
  return at;
}

}  // namespace
}  // namespace dq

using namespace dq;

extern "C" {

dq_status dq_freq_merge(const dq_freq_table* a, const dq_freq_table* b, dq_freq_table** out) {
  if (!a || !b || !out) return set_error(DQ_E_INVALID, "dq_freq_merge: NULL argument");
  *out = nullptr;
  if (a->types != b->types || a->hashed != b->hashed)
    return set_error(DQ_E_STATE, "dq_freq_merge: frequency tables over different column types");
  const int64_t n = a->n_groups + b->n_groups;
  if (n >= (int64_t(1) << 31))  // dq_prim's sort positions are 32-bit
    return set_error(DQ_E_UNSUPPORTED, "dq_freq_merge: %lld groups in the two tables (at most 2^31 - 1)", (long long)n);
  if (a->hashed && ((a->n_groups > 0 && !a->d_keys2) || (b->n_groups > 0 && !b->d_keys2)))
    return set_error(DQ_E_STATE, "dq_freq_merge: hashed table without its verification hashes");
  DQ_HIP(hipSetDevice(a->device));
  auto* t = new dq_freq_table();
  std::unique_ptr<dq_freq_table> guard(t);
  t->device = a->device;
  t->stream = a->stream;
  t->types = a->types;
  t->hashed = a->hashed;
  t->n_values = a->n_values + b->n_values;
  Frame fr(group_arena(), a->device);
  const hipStream_t S = t->stream;
  const int64_t na = a->n_groups, nb = b->n_groups;
  uint64_t *k_in = nullptr, *k_s = nullptr, *rep_out = nullptr;
  int64_t *c_in = nullptr, *c_s = nullptr, *nruns = nullptr;
  GroupCols* d_stores = nullptr;
  void *tmp = nullptr, *scan_tmp = nullptr;
  // both inputs self-contained: the output is, and equal first hashes are settled by the values; else the second hash
  // decides as before and the output carries no values
  const bool stores = t->hashed && a->has_store && b->has_store;
  if (dq_status s = take_each(fr, std::max<int64_t>(1, n), k_in, c_in, k_s, c_s)) return s;
  if (dq_status s = take(fr, nruns, 1)) return s;
  DQ_HIP(hipMemcpyAsync(k_in, a->d_keys.get(), na * 8, hipMemcpyDeviceToDevice, S));
  DQ_HIP(hipMemcpyAsync(k_in + na, b->d_keys.get(), nb * 8, hipMemcpyDeviceToDevice, S));
  DQ_HIP(hipMemcpyAsync(c_in, a->d_counts.get(), na * 8, hipMemcpyDeviceToDevice, S));
  DQ_HIP(hipMemcpyAsync(c_in + na, b->d_counts.get(), nb * 8, hipMemcpyDeviceToDevice, S));
  DQ_HIP(t->d_keys.alloc(std::max<int64_t>(1, n)));
  DQ_HIP(t->d_counts.alloc(std::max<int64_t>(1, n)));
  if (t->hashed) DQ_HIP(t->d_keys2.alloc(std::max<int64_t>(1, n)));
  const size_t tb = std::max({prim::sort_temp_bytes(n, 8), prim::runs_temp_bytes(n), prim::run_sums_temp_bytes(n)});
  if (n > 0 && !t->hashed) {
    // both tables' keys are sorted: every key lies between the smaller first and the larger last key, and so
    // shares their common high bits -- the sort covers only the bits below (same order as all 64)
    uint64_t ends[4] = {~0ull, 0ull, ~0ull, 0ull};
    if (na > 0) {
      DQ_HIP(hipMemcpyAsync(&ends[0], a->d_keys.get(), 8, hipMemcpyDeviceToHost, S));
      DQ_HIP(hipMemcpyAsync(&ends[1], a->d_keys.get() + (na - 1), 8, hipMemcpyDeviceToHost, S));
    }
    if (nb > 0) {
      DQ_HIP(hipMemcpyAsync(&ends[2], b->d_keys.get(), 8, hipMemcpyDeviceToHost, S));
      DQ_HIP(hipMemcpyAsync(&ends[3], b->d_keys.get() + (nb - 1), 8, hipMemcpyDeviceToHost, S));
    }
    DQ_HIP(hipStreamSynchronize(S));
    const uint64_t lo = std::min(ends[0], ends[2]), hi = std::max(ends[1], ends[3]);
    const int end_bit = (lo ^ hi) ? 64 - __builtin_clzll(lo ^ hi) : 1;
    int64_t* starts = nullptr;  // the runs' starts
    if (dq_status s = take(fr, tmp, tb)) return s;
    if (dq_status s = take(fr, starts, n)) return s;
    DQ_HIP(prim::sort_pairs(k_in, k_s, c_in, c_s, 8, n, 0, end_bit, false, tmp, tb, S));
    // equal keys of the two tables are now neighbours: one group each, counts added
    DQ_HIP(prim::runs(k_s, n, t->d_keys.get(), starts, nullptr, nruns, tmp, S));
    DQ_HIP(prim::run_sums_i64(c_s, n, starts, nruns, t->d_counts.get(), tmp, S));
    DQ_HIP(hipMemcpyAsync(&t->n_groups, nruns, 8, hipMemcpyDeviceToHost, S));  // (synchronised below)
  } else if (n > 0) {
    // hashed keys: sort by the first hash carrying positions, gather (second hash, count), refuse equal first
    // hashes with different second hashes, then reduce counts and keep each group's second hash
    uint64_t *k2_in = nullptr, *pos = nullptr, *pos_s = nullptr, *k2_s = nullptr;
    int64_t* kdrop = nullptr;
    int32_t* coll = nullptr;
    if (dq_status s = take_each(fr, n, k2_in, pos, pos_s, k2_s, kdrop)) return s;
    if (dq_status s = take(fr, coll, 2)) return s;
    DQ_HIP(hipMemcpyAsync(k2_in, a->d_keys2.get(), na * 8, hipMemcpyDeviceToDevice, S));
    DQ_HIP(hipMemcpyAsync(k2_in + na, b->d_keys2.get(), nb * 8, hipMemcpyDeviceToDevice, S));
    if (dq_status s = fill_iota_u64(pos, n, S)) return s;
    if (dq_status s = take(fr, tmp, tb)) return s;
    DQ_HIP(prim::sort_pairs(k_in, k_s, pos, pos_s, 8, n, 0, 64, false, tmp, tb, S));
    DQ_HIP(hipMemsetAsync(coll, 0, 8, S));
    if (stores) {  // members of a run compared exactly, value by value, through the two stores
      const GroupCols two[2] = {store_cols(a), store_cols(b)};
      if (dq_status s = take(fr, d_stores, 2)) return s;
      DQ_HIP(hipMemcpyAsync(d_stores, two, sizeof(two), hipMemcpyHostToDevice, S));
      DQ_HIP(hipStreamSynchronize(S));  // (two is on this frame)
      hipLaunchKernelGGL(merge_gather_check_values, dim3(grid_for(n)), dim3(256), 0, S, k_s, pos_s, k2_in, c_in, n, na,
                         d_stores, k2_s, c_s, coll);
    } else {
      hipLaunchKernelGGL(merge_gather_check, dim3(grid_for(n)), dim3(256), 0, S, k_s, pos_s, k2_in, c_in, n, k2_s, c_s,
                         coll);
    }
    DQ_HIP(hipGetLastError());
    // runs of equal first hashes (kdrop: their starts): counts added, the first second hash kept
    DQ_HIP(prim::runs(k_s, n, t->d_keys.get(), kdrop, nullptr, nruns, tmp, S));
    DQ_HIP(prim::run_sums_i64(c_s, n, kdrop, nruns, t->d_counts.get(), tmp, S));
    DQ_HIP(prim::run_firsts_u64(k2_s, n, kdrop, nruns, t->d_keys2.get(), S));
    int32_t collided = 0;
    DQ_HIP(hipMemcpyAsync(&collided, coll, 4, hipMemcpyDeviceToHost, S));
    if (dq_status s = read_back(&t->n_groups, nruns, S)) return s;
    if (collided)
      return set_error(DQ_E_UNSUPPORTED, "dq_freq_merge: 64-bit tuple-hash collision between distinct values of the two tables");
    if (stores) {
      // every output group's tuple from the first member of its run, gathered from the two stores
      if (dq_status s = take(fr, rep_out, std::max<int64_t>(1, t->n_groups))) return s;
      DQ_HIP(prim::run_firsts_u64(pos_s, n, kdrop, nruns, rep_out, S));
      hipLaunchKernelGGL(merge_row_ids, dim3(grid_for(t->n_groups)), dim3(256), 0, S, rep_out, t->n_groups, na);
      DQ_HIP(hipGetLastError());
    }
  }
  if (stores) {
    if (dq_status s = take(fr, scan_tmp, prim::scan_temp_bytes(t->n_groups + 1))) return s;
    for (int c = 0; c < (int)t->types.size(); ++c)
      if (dq_status s = gather_column(S, d_stores, rep_out, t->n_groups, c, t->types[c], scan_tmp, &t->store[c])) return s;
    t->has_store = true;
  }
  DQ_HIP(hipStreamSynchronize(S));
  *out = guard.release();
  return DQ_OK;
}

int32_t dq_freq_self_contained(const dq_freq_table* t) { return t && (!t->hashed || t->has_store) ? 1 : 0; }

dq_status dq_freq_materialize(dq_freq_table* t, const dq_column_view* cols, const int64_t* chunk_rows, int32_t n_chunks) {
  if (!t) return set_error(DQ_E_INVALID, "dq_freq_materialize: NULL table");
  if (!t->hashed || t->has_store) return DQ_OK;  // its keys are its values / already done
  if (t->n_groups > 0 && !t->d_rep)
    return set_error(DQ_E_STATE, "dq_freq_materialize: a hashed table without representative rows (merged without values)");
  const int n_cols = (int)t->types.size();
  if (n_chunks < 0 || n_chunks > kMaxGroupChunks || (n_chunks > 0 && (!cols || !chunk_rows)) ||
      (t->n_groups > 0 && n_chunks == 0))
    return set_error(DQ_E_INVALID, "dq_freq_materialize: bad chunks (%d for %lld groups)", n_chunks, (long long)t->n_groups);
  std::vector<GroupCols> gcs(std::max(1, n_chunks));
  for (int k = 0; k < n_chunks; ++k) {
    if (chunk_rows[k] < 0 || chunk_rows[k] >= (1ll << kRowBits)) return set_error(DQ_E_INVALID, "chunk rows");
    gcs[k] = view_cols(t->types.data(), n_cols, cols + (size_t)k * n_cols, ~0ull, false);
  }
  DQ_HIP(hipSetDevice(t->device));
  Frame fr(group_arena(), t->device);
  const hipStream_t S = t->stream;
  GroupCols* d_chunks = nullptr;
  int64_t* d_rows = nullptr;
  int32_t* bad = nullptr;
  void* scan_tmp = nullptr;
  if (dq_status s = take(fr, d_chunks, gcs.size())) return s;
  if (dq_status s = take(fr, d_rows, std::max(1, n_chunks))) return s;
  if (dq_status s = take(fr, bad, 2)) return s;
  if (dq_status s = take(fr, scan_tmp, prim::scan_temp_bytes(t->n_groups + 1))) return s;
  DQ_HIP(hipMemcpyAsync(d_chunks, gcs.data(), gcs.size() * sizeof(GroupCols), hipMemcpyHostToDevice, S));
  if (t->n_groups > 0) {
    // the views must cover every stored row id before anything is read through them
    DQ_HIP(hipMemcpyAsync(d_rows, chunk_rows, (size_t)n_chunks * 8, hipMemcpyHostToDevice, S));
    int32_t out_of_range = 0;
    if (dq_status s = read_flag(bad, S, &out_of_range, [&] {
          hipLaunchKernelGGL(rep_check, dim3(grid_for(t->n_groups)), dim3(256), 0, S, t->d_rep.get(), t->n_groups, d_rows,
                             n_chunks, bad);
        }))
      return s;
    if (out_of_range)
      return set_error(DQ_E_INVALID, "dq_freq_materialize: the chunks do not cover the table's representative rows "
                                     "(not the views it was built from)");
  }
  StoreCol cols_out[kMaxGroupCols];
  for (int c = 0; c < n_cols; ++c)
    if (dq_status s = gather_column(S, d_chunks, t->d_rep.get(), t->n_groups, c, t->types[c], scan_tmp, &cols_out[c]))
      return s;
  DQ_HIP(hipStreamSynchronize(S));
  for (int c = 0; c < n_cols; ++c) t->store[c] = std::move(cols_out[c]);  // all columns or none
  t->has_store = true;
  return DQ_OK;
}

int64_t dq_freq_to_bytes(const dq_freq_table* t, uint8_t* out, int64_t cap) {
  if (!t) return set_error(DQ_E_INVALID, "dq_freq_to_bytes: NULL table");
  if (t->hashed && !t->has_store)
    return set_error(DQ_E_STATE, "dq_freq_to_bytes: the table does not own its values (dq_freq_materialize it first)");
  FreqImageView v;
  const int64_t size = image_layout(t, &v);
  if (!out || cap < size) return size;
  DQ_HIP(hipSetDevice(t->device));
  std::memset(out, 0, (size_t)size);
  std::memcpy(out, "DQFT", 4);
  const uint32_t head[3] = {kFreqImageVersion, kFreqImageOrder, (uint32_t)v.n_cols};
  std::memcpy(out + 4, head, 12);
  std::memcpy(out + 16, t->types.data(), 4 * (size_t)v.n_cols);
  int64_t at = 16 + 4 * (int64_t)((v.n_cols + 1) & ~1);
  const int32_t hashed = t->hashed;
  std::memcpy(out + at, &hashed, 4);
  std::memcpy(out + at + 8, &v.n_groups, 8);
  std::memcpy(out + at + 16, &v.n_values, 8);
  const int64_t G = v.n_groups;
  const hipStream_t S = t->stream;
  if (G > 0) {
    DQ_HIP(hipMemcpyAsync(out + v.keys, t->d_keys.get(), G * 8, hipMemcpyDeviceToHost, S));
    DQ_HIP(hipMemcpyAsync(out + v.counts, t->d_counts.get(), G * 8, hipMemcpyDeviceToHost, S));
    if (t->hashed) DQ_HIP(hipMemcpyAsync(out + v.keys2, t->d_keys2.get(), G * 8, hipMemcpyDeviceToHost, S));
  }
  for (int c = 0; c < v.n_cols && t->hashed; ++c) {
    if (v.col_offsets[c]) {
      std::memcpy(out + v.col_offsets[c] - 8, &v.col_bytes[c], 8);
      DQ_HIP(hipMemcpyAsync(out + v.col_offsets[c], t->store[c].offsets.get(), (G + 1) * 8, hipMemcpyDeviceToHost, S));
    }
    if (v.col_bytes[c] > 0)
      DQ_HIP(hipMemcpyAsync(out + v.col_values[c], t->store[c].values.get(), v.col_bytes[c], hipMemcpyDeviceToHost, S));
  }
  DQ_HIP(hipStreamSynchronize(S));
  return size;
}

dq_status dq_freq_from_bytes(const uint8_t* bytes, int64_t n, int32_t device, void* hip_stream, dq_freq_table** out) {
  if (!out) return set_error(DQ_E_INVALID, "dq_freq_from_bytes: out is NULL");
  *out = nullptr;
  FreqImageView v;
  char err[256];
  if (dq_status s = freq_image_parse(bytes, n, &v, err, sizeof(err))) return set_error(s, "%s", err);
  DQ_HIP(hipSetDevice(device));
  auto* t = new dq_freq_table();
  std::unique_ptr<dq_freq_table> guard(t);
  t->device = device;
  t->stream = reinterpret_cast<hipStream_t>(hip_stream);
  t->hashed = v.hashed;
  t->types.assign(v.types, v.types + v.n_cols);
  t->n_groups = v.n_groups;
  t->n_values = v.n_values;
  const int64_t G = v.n_groups;
  const hipStream_t S = t->stream;
  DQ_HIP(t->d_keys.alloc(std::max<int64_t>(1, G)));
  DQ_HIP(t->d_counts.alloc(std::max<int64_t>(1, G)));
  if (t->hashed) DQ_HIP(t->d_keys2.alloc(std::max<int64_t>(1, G)));
  if (G > 0) {
    DQ_HIP(hipMemcpyAsync(t->d_keys.get(), bytes + v.keys, G * 8, hipMemcpyHostToDevice, S));
    DQ_HIP(hipMemcpyAsync(t->d_counts.get(), bytes + v.counts, G * 8, hipMemcpyHostToDevice, S));
    if (t->hashed) DQ_HIP(hipMemcpyAsync(t->d_keys2.get(), bytes + v.keys2, G * 8, hipMemcpyHostToDevice, S));
  }
  for (int c = 0; c < v.n_cols && t->hashed; ++c) {
    StoreCol& sc = t->store[c];
    sc.bytes = v.col_bytes[c];
    DQ_HIP(sc.values.alloc(std::max<int64_t>(8, sc.bytes)));
    if (sc.bytes > 0) DQ_HIP(hipMemcpyAsync(sc.values.get(), bytes + v.col_values[c], sc.bytes, hipMemcpyHostToDevice, S));
    if (v.col_offsets[c]) {
      DQ_HIP(sc.offsets.alloc(G + 1));
      DQ_HIP(hipMemcpyAsync(sc.offsets.get(), bytes + v.col_offsets[c], (G + 1) * 8, hipMemcpyHostToDevice, S));
    }
  }
  t->has_store = t->hashed != 0;
  DQ_HIP(hipStreamSynchronize(S));
  *out = guard.release();
  return DQ_OK;
}

dq_status dq_freq_take_values(const dq_freq_table* t, const uint64_t* keys, int32_t n, int32_t col, void* values,
                              int64_t values_cap, int64_t* offsets, int64_t* values_bytes) {
  if (!t || n < 0 || !values_bytes || (n > 0 && !keys) || col < 0 || col >= (int)t->types.size())
    return set_error(DQ_E_INVALID, "dq_freq_take_values: bad arguments");
  if (!t->has_store) return set_error(DQ_E_STATE, "dq_freq_take_values: the table does not own its values");
  const int es = dq_freq_elem_size(t->types[col]);
  if (es == 0 && !offsets) return set_error(DQ_E_INVALID, "dq_freq_take_values: a string column needs offsets[n + 1]");
  DQ_HIP(hipSetDevice(t->device));
  Frame fr(group_arena(), t->device);
  const hipStream_t S = t->stream;
  uint64_t *want = nullptr, *idx = nullptr;
  int32_t* missing = nullptr;
  GroupCols* d_store = nullptr;
  void* scan_tmp = nullptr;
  if (dq_status s = take_each(fr, std::max(1, n), want, idx)) return s;
  if (dq_status s = take(fr, missing, 2)) return s;
  if (dq_status s = take(fr, d_store, 1)) return s;
  if (dq_status s = take(fr, scan_tmp, prim::scan_temp_bytes((int64_t)n + 1))) return s;
  const GroupCols st = store_cols(t);
  DQ_HIP(hipMemcpyAsync(d_store, &st, sizeof(st), hipMemcpyHostToDevice, S));
  if (n > 0) {
    DQ_HIP(hipMemcpyAsync(want, keys, (size_t)n * 8, hipMemcpyHostToDevice, S));
    int32_t miss = 0;
    if (dq_status s = read_flag(missing, S, &miss, [&] {
          hipLaunchKernelGGL(find_groups, dim3((n + 255) / 256), dim3(256), 0, S, want, n, t->d_keys.get(), t->n_groups, idx,
                             missing);
        }))
      return s;
    if (miss) return set_error(DQ_E_INVALID, "dq_freq_take_values: a key that is not a group of the table");
  }
  DQ_HIP(hipStreamSynchronize(S));
  StoreCol got;
  if (dq_status s = gather_column(S, d_store, idx, n, col, t->types[col], scan_tmp, &got)) return s;
  *values_bytes = got.bytes;
  if (got.offsets) DQ_HIP(hipMemcpyAsync(offsets, got.offsets.get(), ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, S));
  if (values && values_cap >= got.bytes && got.bytes > 0)
    DQ_HIP(hipMemcpyAsync(values, got.values.get(), got.bytes, hipMemcpyDeviceToHost, S));
  DQ_HIP(hipStreamSynchronize(S));
  return DQ_OK;
}

}  // extern "C"
