// dq_schema.hip -- RowLevelSchemaValidator.validate (schema/RowLevelSchemaValidator.scala:183-281) on the device:
// the fused per-row verdict of a whole schema, and the stable row compaction that builds validRows / invalidRows.
// The per-value rules are dq_schema.h's.
//
// Verdict kernel (dq_schema_verdict_kernel): dq_cast.hip's shape -- one row per lane, wave w of a block takes
// kGroupsPerWave consecutive 64-row groups, a lane walks its string through the aligned dwords that hold its bytes.
// One launch evaluates every definition of the schema in order (toCNF's foldLeft, :226): a lane stops evaluating at
// its first FALSE clause (FALSE AND x = FALSE) and otherwise goes on, so it meets every NULL clause (:246) that
// separates TRUE from UNKNOWN.  The definitions, compiled masks and DFAs are read through wave-uniform pointers (the
// DFAs from LDS when they fit).  Per group the wave's ballots of "m is TRUE" and "m is FALSE" are the two bitmap
// words, stored by lane 0 (bits past n_rows are 0); per cast column every lane stores its value and lane 0 the
// ballot of "cast not NULL".  Plain stores only; the only atomics are the two counters, one add per wave each.
//
// Take (dq_take_index + dq_take_rows): per-word popcounts of the selection bitmap, prim::exclusive_sum_i64 over
// them, and each selected row's rank = its word's base + the popcount of the lower bits; the ranks give the index of
// selected rows in source order, which every column of the table then gathers through: fixed-width values (1, 2, 4,
// 8, 16 bytes) by one load and one store per row, bitmaps (validity, bool values) by a ballot per 64 output rows,
// strings by scanning the selected lengths into the new offsets and copying the bytes, one string per lane.
// Copy granularity: the strings of an ingested table are short (a dozen bytes), so a lane copies its own string --
// bytes up to the destination's 4-byte boundary, then whole destination dwords assembled from two aligned source
// dwords, then the tail bytes; a wave per string would leave most lanes idle at these lengths, and whole dwords
// written by their single owner need no atomics where neighbouring strings share a dword.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "dq_hip_host.h"
#include "dq_prim.h"
#include "dq_regex.h"
#include "dq_schema.h"

#define DQ_DEC_TABLE static __constant__ const
#include "dq_dec_tables.inc"
#undef DQ_DEC_TABLE

namespace dq {
namespace {

constexpr int kSchemaBlock = 256;
constexpr int kGroupsPerWave = 4;                                  // 64-row groups per wave
constexpr int kRowsPerBlock = kSchemaBlock * kGroupsPerWave;       // 1024
constexpr int kDfaLdsWords = 24 * 1024;                            // DFAs up to 48 KiB are staged in LDS
// (tests/regex_cases.py SCHEMA_PATTERNS are sized around this constant -- one DFA under it, two over -- and
// tests/test_regex_cases_host.py restates it: change them together, or the global-memory walk loses its test)

// the bytes of one string through the aligned dwords that hold them (dq_cast.hip's reader, 64-bit positions)
struct SchemaDevBytes {
  using idx = int64_t;
  const uint32_t* words;
  int64_t base;
  int64_t cur;
  uint32_t w;
  __device__ __forceinline__ uint32_t at(int64_t i) {
    const int64_t p = base + i;
    const int64_t k = p >> 2;
    if (k != cur) {
      w = words[k];
      cur = k;
    }
    return (w >> (((uint32_t)p & 3u) * 8u)) & 0xFFu;
  }
};

// one definition's buffers of one chunk
struct SchemaColDev {
  const uint32_t* data;
  const void* offsets;
  const uint32_t* validity;  // null: no NULL rows
  void* out_values;          // null: the cast is not materialised
  uint64_t* out_validity;
  int32_t large;             // int64 offsets
  int32_t pad;
};

// counters[0]: rows whose m is TRUE, counters[1]: rows whose m is FALSE
__global__ __launch_bounds__(kSchemaBlock) void dq_schema_verdict_kernel(
    const SchemaDef* __restrict__ defs, const SchemaColDev* __restrict__ cols, int n_defs,
    const SchemaMaskEl* __restrict__ masks, const uint16_t* __restrict__ regex, int regex_lds_words, int64_t n_rows,
    uint64_t* __restrict__ bm_true, uint64_t* __restrict__ bm_false, unsigned long long* counters) {
  extern __shared__ __attribute__((aligned(16))) uint16_t dfa_lds[];
  const uint16_t* dfa = regex;
  if (regex_lds_words > 0) {
    for (int k = threadIdx.x; k < regex_lds_words; k += kSchemaBlock) dfa_lds[k] = regex[k];
    __syncthreads();
    dfa = dfa_lds;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_groups = (n_rows + 63) >> 6;
  const int64_t g0 = ((int64_t)blockIdx.x * (kSchemaBlock / 64) + wave) * kGroupsPerWave;
  const DecTab tab{kDecP10Lo, kDecP10Hi, kDecRcpHi, kDecRcpLo};
  uint32_t n_true = 0, n_false = 0;  // wave-uniform
  for (int j = 0; j < kGroupsPerWave; ++j) {
    const int64_t g = g0 + j;
    if (g >= n_groups) break;
    const int64_t row = g * 64 + lane;
    const bool in = row < n_rows;
    int outcome = 0;  // SchemaOutcome bits over the definitions so far
    for (int d = 0; d < n_defs; ++d) {
      const SchemaDef def = defs[d];
      const SchemaColDev col = cols[d];
      SchemaCast cast{0, 0, false};
      if (in && !(outcome & SCHEMA_CLAUSE_FALSE)) {
        bool valid = true;
        if (col.validity != nullptr) valid = (col.validity[row >> 5] >> ((uint32_t)row & 31u)) & 1u;
        int64_t o0 = 0, o1 = 0;
        if (valid) {
          if (col.large) {
            o0 = static_cast<const int64_t*>(col.offsets)[row];
            o1 = static_cast<const int64_t*>(col.offsets)[row + 1];
          } else {
            o0 = static_cast<const int32_t*>(col.offsets)[row];
            o1 = static_cast<const int32_t*>(col.offsets)[row + 1];
          }
          if (o0 < 0 || o1 < o0) o1 = o0 = 0;  // (malformed offsets read nothing: an empty value)
        }
        SchemaDevBytes rd{col.data, o0, (int64_t)-1, 0u};
        outcome |= schema_eval(def, masks, dfa, tab, rd, o1 - o0, !valid, cast);
      }
      if (col.out_values != nullptr) {  // wave-uniform
        const uint64_t okm = __builtin_amdgcn_ballot_w64(cast.ok);
        if (lane == 0) col.out_validity[g] = okm;
        if (in) {
          if (def.kind == SCHEMA_INT) static_cast<int32_t*>(col.out_values)[row] = (int32_t)cast.lo;
          else if (def.kind == SCHEMA_DECIMAL) static_cast<ulonglong2*>(col.out_values)[row] = make_ulonglong2(cast.lo, cast.hi);
          else static_cast<uint64_t*>(col.out_values)[row] = cast.lo;
        }
      }
    }
    const uint64_t tm = __builtin_amdgcn_ballot_w64(in && outcome == 0);
    const uint64_t fm = __builtin_amdgcn_ballot_w64(in && (outcome & SCHEMA_CLAUSE_FALSE));
    if (lane == 0) {
      bm_true[g] = tm;
      bm_false[g] = fm;
    }
    n_true += (uint32_t)__builtin_popcountll(tm);
    n_false += (uint32_t)__builtin_popcountll(fm);
  }
  if (lane == 0 && n_true != 0) atomicAdd(&counters[0], (unsigned long long)n_true);
  if (lane == 0 && n_false != 0) atomicAdd(&counters[1], (unsigned long long)n_false);
}

// ---------------------------------------------------------------------------------------------------- take
constexpr int kTakeBlock = 256;

// counts[w] = selected rows of word w (bits past n_rows do not count)
__global__ void dq_take_popcount(const uint64_t* __restrict__ sel, int64_t n_rows, int64_t n_words,
                                 int64_t* __restrict__ counts) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  uint64_t m = sel[w];
  const int64_t left = n_rows - w * 64;
  if (left < 64) m &= (1ull << left) - 1;
  counts[w] = __builtin_popcountll(m);
}

// index[rank] = row for every selected row; rank = the word's base + the popcount of the lower bits
__global__ void dq_take_scatter_index(const uint64_t* __restrict__ sel, const int64_t* __restrict__ base,
                                      int64_t n_rows, int64_t n_selected, int64_t* __restrict__ index) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  const uint64_t m = sel[row >> 6];
  const uint32_t b = (uint32_t)row & 63u;
  if (!((m >> b) & 1ull)) return;
  const int64_t rank = base[row >> 6] + __builtin_popcountll(m & ((1ull << b) - 1));
  if (rank < n_selected) index[rank] = row;
}

template <typename T>
__global__ void dq_take_fixed(const T* __restrict__ src, const int64_t* __restrict__ index, int64_t n_selected,
                              int64_t n_rows, T* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_selected) return;
  const int64_t s = index[r];
  if ((uint64_t)s < (uint64_t)n_rows) out[r] = src[s];
}

// out word g = the source bits (LSB-first, 32-bit words; null: all set) of output rows 64 g .. 64 g + 63
__global__ void dq_take_bits(const uint32_t* __restrict__ bits, const int64_t* __restrict__ index, int64_t n_selected,
                             int64_t n_rows, uint64_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
  const int64_t r = g * 64 + lane;
  bool bit = false;
  if (r < n_selected) {
    const int64_t s = index[r];
    if ((uint64_t)s < (uint64_t)n_rows) bit = bits == nullptr || ((bits[s >> 5] >> ((uint32_t)s & 31u)) & 1u);
  }
  const uint64_t m = __builtin_amdgcn_ballot_w64(bit);
  if (lane == 0 && g * 64 < n_selected) out[g] = m;
}

// lens[r] = bytes of selected row r; lens[n_selected] = 0 (its exclusive sum is the total)
template <typename OffT>
__global__ void dq_take_lengths(const OffT* __restrict__ offsets, const int64_t* __restrict__ index,
                                int64_t n_selected, int64_t n_rows, int64_t* __restrict__ lens) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_selected) return;
  int64_t len = 0;
  if (r < n_selected) {
    const int64_t s = index[r];
    if ((uint64_t)s < (uint64_t)n_rows) {
      len = (int64_t)offsets[s + 1] - (int64_t)offsets[s];
      if (len < 0) len = 0;
    }
  }
  lens[r] = len;
}

// the new offsets, and one string per lane copied to its place (see the header comment for the granularity)
template <typename OffT>
__global__ void dq_take_strings(const uint32_t* __restrict__ src_words, const OffT* __restrict__ offsets,
                                const int64_t* __restrict__ index, const int64_t* __restrict__ starts,
                                int64_t n_selected, int64_t n_rows, OffT* __restrict__ out_offsets,
                                uint8_t* __restrict__ out_bytes) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_selected) return;
  const int64_t d = starts[r];
  out_offsets[r] = (OffT)d;
  if (r == n_selected || out_bytes == nullptr) return;
  const int64_t n = starts[r + 1] - d;
  const int64_t row = index[r];
  if (n <= 0 || (uint64_t)row >= (uint64_t)n_rows) return;
  const int64_t s = (int64_t)offsets[row];
  const uint8_t* src = reinterpret_cast<const uint8_t*>(src_words);
  int64_t i = 0;
  for (; i < n && ((d + i) & 3); ++i) out_bytes[d + i] = src[s + i];
  uint32_t* out_words = reinterpret_cast<uint32_t*>(out_bytes);
  for (; n - i >= 4; i += 4) {
    // the aligned source dwords k and (when the position is unaligned) k + 1 both hold bytes of this string
    const int64_t p = s + i, k = p >> 2;
    const uint32_t sh = ((uint32_t)p & 3u) * 8u;
    uint32_t v = src_words[k];
    if (sh != 0) v = (v >> sh) | (src_words[k + 1] << (32u - sh));
    out_words[(d + i) >> 2] = v;
  }
  for (; i < n; ++i) out_bytes[d + i] = src[s + i];
}

inline unsigned grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

int fixed_width(int32_t type) {
  switch (DQ_TYPE_BASE(type)) {
    case DQ_TYPE_F64: case DQ_TYPE_I64: case DQ_TYPE_TIMESTAMP: return 8;
    case DQ_TYPE_I32: case DQ_TYPE_F32: case DQ_TYPE_DATE32: return 4;
    case DQ_TYPE_I16: return 2;
    case DQ_TYPE_I8: return 1;
    case DQ_TYPE_DECIMAL128: return 16;
    default: return 0;
  }
}

const DecTab& schema_host_tab() { return dec_host_tab(); }

}  // namespace
}  // namespace dq

struct dq_schema_plan {
  std::vector<dq::SchemaDef> defs;
  std::vector<int32_t> column;             // per definition: index into the caller's views
  std::vector<dq::SchemaMaskEl> masks;
  std::vector<uint16_t> regex;             // regex_serialize blobs, back to back
  std::vector<dq::SchemaColDev> cols;      // staging of one call's pointers
  int32_t device = -1;                     // where the device copies live (-1: nowhere yet)
  dq::DevPtr<dq::SchemaDef> d_defs;
  dq::DevPtr<dq::SchemaMaskEl> d_masks;
  dq::DevPtr<uint16_t> d_regex;
  dq::DevPtr<dq::SchemaColDev> d_cols;
  dq::DevPtr<unsigned long long> d_counters;
  void release() {
    d_defs.reset(), d_masks.reset(), d_regex.reset(), d_cols.reset(), d_counters.reset();
    device = -1;
  }
};

namespace dq {
// The string gather of dq_take_rows, also dq_dict_decode's (dq_dict.hip): string r of the output is string index[r] of
// src's n_rows (an index outside them: the empty string); the same row may be taken any number of times.
dq_status take_strings(bool large, const dq_column_view* src, int64_t n_rows, const int64_t* index, int64_t n_selected,
                       void* out_values, int64_t values_capacity, void* out_offsets, int64_t* data_bytes,
                       hipStream_t st, const char* me) {
  const unsigned grid1 = grid_for(n_selected + 1, kTakeBlock);
  if (!large && n_selected >= INT32_MAX) return set_error(DQ_E_INVALID, "%s: UTF8 chunk of %lld rows", me, (long long)n_selected);
  DevPtr<int64_t> lens;
  DevPtr<void> temp;
  DQ_HIP(lens.alloc((size_t)(n_selected + 1)));
  DQ_HIP(temp.alloc(prim::scan_temp_bytes(n_selected + 1) + 16));
  int64_t* const dl = lens.get();
  if (large) hipLaunchKernelGGL(dq_take_lengths<int64_t>, dim3(grid1), dim3(kTakeBlock), 0, st, static_cast<const int64_t*>(src->offsets), index, n_selected, n_rows, dl);
  else hipLaunchKernelGGL(dq_take_lengths<int32_t>, dim3(grid1), dim3(kTakeBlock), 0, st, static_cast<const int32_t*>(src->offsets), index, n_selected, n_rows, dl);
  DQ_HIP(hipGetLastError());
  DQ_HIP(prim::exclusive_sum_i64(dl, dl, n_selected + 1, temp.get(), st));
  int64_t total = 0;
  DQ_HIP(hipMemcpyAsync(&total, dl + n_selected, 8, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (data_bytes) *data_bytes = total;
  if (!large && total > INT32_MAX) return set_error(DQ_E_INVALID, "%s: %lld bytes do not fit UTF8 offsets", me, (long long)total);
  if (out_values && values_capacity < total)
    return set_error(DQ_E_INVALID, "%s: %lld value bytes for %lld", me, (long long)values_capacity, (long long)total);
  // (out_values NULL: the sizing call -- offsets and *data_bytes only)
  if (large) hipLaunchKernelGGL(dq_take_strings<int64_t>, dim3(grid1), dim3(kTakeBlock), 0, st, static_cast<const uint32_t*>(src->values), static_cast<const int64_t*>(src->offsets), index, dl, n_selected, n_rows, static_cast<int64_t*>(out_offsets), static_cast<uint8_t*>(out_values));
  else hipLaunchKernelGGL(dq_take_strings<int32_t>, dim3(grid1), dim3(kTakeBlock), 0, st, static_cast<const uint32_t*>(src->values), static_cast<const int32_t*>(src->offsets), index, dl, n_selected, n_rows, static_cast<int32_t*>(out_offsets), static_cast<uint8_t*>(out_values));
  DQ_HIP(hipGetLastError());
  DQ_HIP(hipStreamSynchronize(st));
  return DQ_OK;
}
}  // namespace dq

extern "C" {

dq_status dq_schema_plan_create(const dq_schema_column* defs, int32_t n_defs, dq_schema_plan** out) {
  using namespace dq;
  if (!out || n_defs < 0 || (n_defs > 0 && !defs)) return set_error(DQ_E_INVALID, "dq_schema_plan_create: bad argument");
  *out = nullptr;
  auto plan = new dq_schema_plan();
  const auto fail = [&](dq_status s) {
    delete plan;
    return s;
  };
  for (int32_t i = 0; i < n_defs; ++i) {
    const dq_schema_column& c = defs[i];
    SchemaDef d{};
    d.kind = c.kind;
    if (c.column < 0) return fail(set_error(DQ_E_INVALID, "dq_schema_plan_create: definition %d: column %d", i, c.column));
    if (!c.nullable) d.flags |= SCHEMA_NOT_NULLABLE;
    switch (c.kind) {
      case DQ_SCHEMA_STRING:
      case DQ_SCHEMA_INT:
        if (c.has_min) d.flags |= SCHEMA_HAS_MIN, d.minv = c.min_value;
        if (c.has_max) d.flags |= SCHEMA_HAS_MAX, d.maxv = c.max_value;
        if (c.kind == DQ_SCHEMA_STRING && c.text) {
          RegexDfa dfa;
          if (dq_status s = regex_compile(c.text, DQ_REGEX_EXTRACT_NONEMPTY, dfa)) return fail(s);
          d.flags |= SCHEMA_HAS_REGEX;
          d.aux = (int32_t)plan->regex.size();
          regex_serialize(dfa, plan->regex);
        }
        break;
      case DQ_SCHEMA_DECIMAL:
        // DataTypes.createDecimalType(p, s) (:255); precisions the device holds: DecimalType.MAX_PRECISION = 38
        if (!(c.scale >= 0 && c.scale <= c.precision && c.precision >= 1 && c.precision <= kDecMaxPrecision))
          return fail(set_error(DQ_E_INVALID, "dq_schema_plan_create: definition %d: DecimalType(%d,%d)", i, c.precision, c.scale));
        d.p = c.precision;
        d.s = c.scale;
        break;
      case DQ_SCHEMA_TIMESTAMP: {
        if (!c.text) return fail(set_error(DQ_E_INVALID, "dq_schema_plan_create: definition %d: no mask", i));
        SchemaMaskEl els[kSchemaMaxMask];
        const char* why = nullptr;
        const int n = schema_compile_mask(c.text, els, &why);
        if (n < 0) return fail(set_error(DQ_E_UNSUPPORTED, "timestamp mask \"%s\": %s", c.text, why));
        d.aux = (int32_t)plan->masks.size();
        d.aux_n = n;
        plan->masks.insert(plan->masks.end(), els, els + n);
        break;
      }
      default:
        return fail(set_error(DQ_E_INVALID, "dq_schema_plan_create: definition %d: kind %d", i, c.kind));
    }
    plan->defs.push_back(d);
    plan->column.push_back(c.column);
  }
  plan->cols.resize(plan->defs.size());
  *out = plan;
  return DQ_OK;
}

void dq_schema_plan_destroy(dq_schema_plan* plan) {
  if (!plan) return;
  plan->release();
  delete plan;
}

dq_status dq_schema_validate(dq_schema_plan* plan, const int32_t* types, const dq_column_view* cols, int32_t n_cols,
                             int64_t n_rows, uint64_t* valid_bitmap, uint64_t* invalid_bitmap, void* const* cast_values,
                             uint8_t* const* cast_validity, int32_t device, void* hip_stream, int64_t* num_valid,
                             int64_t* num_invalid) {
  using namespace dq;
  const char* me = "dq_schema_validate";
  if (!plan || n_rows < 0 || n_cols < 0) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (num_valid) *num_valid = 0;
  if (num_invalid) *num_invalid = 0;
  const int n_defs = (int)plan->defs.size();
  for (int d = 0; d < n_defs; ++d) {
    const int32_t c = plan->column[d];
    if (c >= n_cols || !types || !cols) return set_error(DQ_E_INVALID, "%s: definition %d reads column %d of %d", me, d, c, n_cols);
    if (types[c] != DQ_TYPE_UTF8 && types[c] != DQ_TYPE_LARGE_UTF8)
      return set_error(DQ_E_TYPE, "%s: column %d has type %d, not UTF8 / LARGE_UTF8", me, c, types[c]);
    if (cols[c].reserved != 0) return set_error(DQ_E_INVALID, "%s: bad view", me);
    if (types[c] == DQ_TYPE_UTF8 && n_rows >= INT32_MAX) return set_error(DQ_E_INVALID, "%s: UTF8 chunk of %lld rows", me, (long long)n_rows);
  }
  if (n_rows == 0) return DQ_OK;
  if (!valid_bitmap || !invalid_bitmap || ((uintptr_t)valid_bitmap & 7) || ((uintptr_t)invalid_bitmap & 7))
    return set_error(DQ_E_INVALID, "%s: NULL or misaligned bitmap", me);
  for (int d = 0; d < n_defs; ++d) {
    const dq_column_view& v = cols[plan->column[d]];
    SchemaColDev& o = plan->cols[d];
    if (!v.values || !v.offsets) return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
    if (((uintptr_t)v.values & 3) || ((uintptr_t)v.validity & 3) || ((uintptr_t)v.offsets & 3))
      return set_error(DQ_E_INVALID, "%s: misaligned buffer", me);
    o.data = static_cast<const uint32_t*>(v.values);
    o.offsets = v.offsets;
    o.validity = reinterpret_cast<const uint32_t*>(v.validity);
    o.large = types[plan->column[d]] == DQ_TYPE_LARGE_UTF8;
    o.pad = 0;
    o.out_values = nullptr;
    o.out_validity = nullptr;
    if (plan->defs[d].kind != SCHEMA_STRING && cast_values && cast_values[d]) {
      if (!cast_validity || !cast_validity[d] || ((uintptr_t)cast_values[d] & 15) || ((uintptr_t)cast_validity[d] & 7))
        return set_error(DQ_E_INVALID, "%s: definition %d: NULL or misaligned cast buffer", me, d);
      o.out_values = cast_values[d];
      o.out_validity = reinterpret_cast<uint64_t*>(cast_validity[d]);
    }
  }
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  if (plan->device != device) {  // the plan's constants move to the device it is first used on
    plan->release();
    const size_t nd = plan->defs.size() ? plan->defs.size() : 1;
    DQ_HIP(plan->d_defs.alloc(nd));
    DQ_HIP(plan->d_cols.alloc(nd));
    DQ_HIP(plan->d_masks.alloc(plan->masks.size() + 1));
    DQ_HIP(plan->d_regex.alloc(plan->regex.size() + 2));
    DQ_HIP(plan->d_counters.alloc(2));
    plan->device = device;
    if (!plan->defs.empty()) DQ_HIP(hipMemcpy(plan->d_defs.get(), plan->defs.data(), plan->defs.size() * sizeof(SchemaDef), hipMemcpyHostToDevice));
    if (!plan->masks.empty()) DQ_HIP(hipMemcpy(plan->d_masks.get(), plan->masks.data(), plan->masks.size() * sizeof(SchemaMaskEl), hipMemcpyHostToDevice));
    if (!plan->regex.empty()) DQ_HIP(hipMemcpy(plan->d_regex.get(), plan->regex.data(), plan->regex.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  if (n_defs > 0) DQ_HIP(hipMemcpyAsync(plan->d_cols.get(), plan->cols.data(), (size_t)n_defs * sizeof(SchemaColDev), hipMemcpyHostToDevice, st));
  DQ_HIP(hipMemsetAsync(plan->d_counters.get(), 0, 16, st));
  const int regex_words = (int)plan->regex.size();
  const int lds_words = regex_words <= kDfaLdsWords ? regex_words : 0;
  hipLaunchKernelGGL(dq_schema_verdict_kernel, dim3(grid_for(n_rows, kRowsPerBlock)), dim3(kSchemaBlock),
                     (size_t)lds_words * sizeof(uint16_t), st, plan->d_defs.get(), plan->d_cols.get(), n_defs,
                     plan->d_masks.get(), plan->d_regex.get(), lds_words, n_rows, valid_bitmap, invalid_bitmap,
                     plan->d_counters.get());
  DQ_HIP(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  DQ_HIP(hipMemcpyAsync(h, plan->d_counters.get(), 16, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (num_valid) *num_valid = (int64_t)h[0];
  if (num_invalid) *num_invalid = (int64_t)h[1];
  return DQ_OK;
}

dq_status dq_schema_check_host(const dq_schema_plan* plan, const uint8_t* const* data, const int64_t* const* offsets,
                               const uint8_t* const* valid, int32_t n_cols, int64_t n_rows, uint8_t* verdict,
                               void* const* cast_values, uint8_t* const* cast_ok) {
  using namespace dq;
  if (!plan || n_rows < 0 || (n_rows > 0 && (!data || !offsets || !verdict)))
    return set_error(DQ_E_INVALID, "dq_schema_check_host: bad argument");
  const int n_defs = (int)plan->defs.size();
  for (int d = 0; d < n_defs; ++d)
    if (plan->column[d] >= n_cols || (n_rows > 0 && (!data[plan->column[d]] || !offsets[plan->column[d]])))
      return set_error(DQ_E_INVALID, "dq_schema_check_host: definition %d: no column %d", d, plan->column[d]);
  const DecTab& tab = schema_host_tab();
  for (int64_t r = 0; r < n_rows; ++r) {
    int outcome = 0;
    for (int d = 0; d < n_defs; ++d) {  // (no early stop here: every definition's cast is reported)
      const int c = plan->column[d];
      const bool is_null = valid && valid[c] && !valid[c][r];
      const int64_t o0 = offsets[c][r], o1 = offsets[c][r + 1];
      CastHostBytes rd{data[c] + o0};
      SchemaCast cast{0, 0, false};
      outcome |= schema_eval(plan->defs[d], plan->masks.data(), plan->regex.data(), tab, rd, is_null ? 0 : o1 - o0, is_null, cast);
      if (cast_ok && cast_ok[d]) cast_ok[d][r] = cast.ok ? 1 : 0;
      if (cast_values && cast_values[d]) {
        if (plan->defs[d].kind == SCHEMA_INT) static_cast<int32_t*>(cast_values[d])[r] = (int32_t)cast.lo;
        else if (plan->defs[d].kind == SCHEMA_DECIMAL) std::memcpy(static_cast<uint8_t*>(cast_values[d]) + 16 * r, &cast.lo, 8), std::memcpy(static_cast<uint8_t*>(cast_values[d]) + 16 * r + 8, &cast.hi, 8);
        else if (plan->defs[d].kind == SCHEMA_TIMESTAMP) static_cast<int64_t*>(cast_values[d])[r] = (int64_t)cast.lo;
      }
    }
    verdict[r] = (outcome & SCHEMA_CLAUSE_FALSE) ? 0 : (outcome ? 2 : 1);
  }
  return DQ_OK;
}

dq_status dq_take_index(const uint64_t* selection, int64_t n_rows, int64_t n_selected, int64_t* index, int32_t device,
                        void* hip_stream) {
  using namespace dq;
  const char* me = "dq_take_index";
  if (n_rows < 0 || n_selected < 0 || n_selected > n_rows) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (n_rows == 0) return DQ_OK;
  if (!selection || ((uintptr_t)selection & 7) || (n_selected > 0 && (!index || ((uintptr_t)index & 7))))
    return set_error(DQ_E_INVALID, "%s: NULL or misaligned buffer", me);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  const int64_t nw = (n_rows + 63) >> 6;
  DevPtr<int64_t> counts;
  DevPtr<void> temp;
  DQ_HIP(counts.alloc((size_t)(nw + 1)));
  DQ_HIP(temp.alloc(prim::scan_temp_bytes(nw + 1) + 16));
  int64_t* const dc = counts.get();
  DQ_HIP(hipMemsetAsync(dc + nw, 0, 8, st));
  hipLaunchKernelGGL(dq_take_popcount, dim3(grid_for(nw, kTakeBlock)), dim3(kTakeBlock), 0, st, selection, n_rows, nw, dc);
  DQ_HIP(hipGetLastError());
  DQ_HIP(prim::exclusive_sum_i64(dc, dc, nw + 1, temp.get(), st));  // dc[nw] = the number of selected rows
  int64_t total = -1;
  DQ_HIP(hipMemcpyAsync(&total, dc + nw, 8, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (total != n_selected)
    return set_error(DQ_E_INVALID, "%s: the bitmap selects %lld rows, not %lld", me, (long long)total, (long long)n_selected);
  if (n_selected == 0) return DQ_OK;
  hipLaunchKernelGGL(dq_take_scatter_index, dim3(grid_for(n_rows, kTakeBlock)), dim3(kTakeBlock), 0, st, selection, dc,
                     n_rows, n_selected, index);
  DQ_HIP(hipGetLastError());
  DQ_HIP(hipStreamSynchronize(st));  // (the scratch is freed on return)
  return DQ_OK;
}

dq_status dq_take_rows(int32_t type, const dq_column_view* src, int64_t n_rows, const int64_t* index, int64_t n_selected,
                       void* out_values, int64_t values_capacity, uint8_t* out_validity, void* out_offsets,
                       int64_t* data_bytes, int32_t device, void* hip_stream) {
  using namespace dq;
  const char* me = "dq_take_rows";
  if (!type_valid(type)) return set_error(DQ_E_TYPE, "%s: type %d", me, type);
  if (!src || src->reserved != 0 || n_rows < 0 || n_selected < 0 || n_selected > n_rows || values_capacity < 0)
    return set_error(DQ_E_INVALID, "%s: bad argument", me);
  if (data_bytes) *data_bytes = 0;
  const bool str = type == DQ_TYPE_UTF8 || type == DQ_TYPE_LARGE_UTF8, large = type == DQ_TYPE_LARGE_UTF8;
  if (n_selected == 0) return DQ_OK;  // (nothing selected: the caller's cleared buffers are the result)
  if (!index || !src->values || (str && (!src->offsets || !out_offsets)) || (!str && !out_values))
    return set_error(DQ_E_INVALID, "%s: NULL buffer", me);
  if (((uintptr_t)out_values & 15) || ((uintptr_t)out_validity & 7) || ((uintptr_t)src->values & 15) ||
      ((uintptr_t)src->validity & 3) || ((uintptr_t)out_offsets & 7) || ((uintptr_t)src->offsets & 3) || ((uintptr_t)index & 7))
    return set_error(DQ_E_INVALID, "%s: misaligned buffer", me);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  DQ_HIP(hipSetDevice(device));
  const unsigned grid = grid_for(n_selected, kTakeBlock);
  const unsigned grid_bits = grid_for(((n_selected + 63) >> 6) * 64, kTakeBlock);
  if (out_validity) {
    hipLaunchKernelGGL(dq_take_bits, dim3(grid_bits), dim3(kTakeBlock), 0, st, reinterpret_cast<const uint32_t*>(src->validity),
                       index, n_selected, n_rows, reinterpret_cast<uint64_t*>(out_validity));
    DQ_HIP(hipGetLastError());
  }
  if (!str) {
    const int w = fixed_width(type);
    const int64_t need = DQ_TYPE_BASE(type) == DQ_TYPE_BOOL ? ((n_selected + 63) >> 6) * 8 : n_selected * w;
    if (values_capacity < need) return set_error(DQ_E_INVALID, "%s: %lld value bytes for %lld", me, (long long)values_capacity, (long long)need);
#define DQ_TAKE_FIXED(T)                                                                                              \
  hipLaunchKernelGGL(dq_take_fixed<T>, dim3(grid), dim3(kTakeBlock), 0, st, static_cast<const T*>(src->values), index, \
                     n_selected, n_rows, static_cast<T*>(out_values))
    switch (w) {
      case 1: DQ_TAKE_FIXED(uint8_t); break;
      case 2: DQ_TAKE_FIXED(uint16_t); break;
      case 4: DQ_TAKE_FIXED(uint32_t); break;
      case 8: DQ_TAKE_FIXED(uint64_t); break;
      case 16: DQ_TAKE_FIXED(ulonglong2); break;
      default:  // BOOL: bit-packed values
        hipLaunchKernelGGL(dq_take_bits, dim3(grid_bits), dim3(kTakeBlock), 0, st, static_cast<const uint32_t*>(src->values),
                           index, n_selected, n_rows, static_cast<uint64_t*>(out_values));
    }
#undef DQ_TAKE_FIXED
    DQ_HIP(hipGetLastError());
    DQ_HIP(hipStreamSynchronize(st));
    return DQ_OK;
  }
  return take_strings(large, src, n_rows, index, n_selected, out_values, values_capacity, out_offsets, data_bytes, st, me);
}

}  // extern "C"
