// dq_segment.hip -- segmented metrics: the scan analyzers' states per group of a key column, on the GPU.
//
// The rows of a chunk carry a segment index seg[r] (dq_freq_lookup_rows against the run's key set; -1: a NULL key).
// dq_segment_order sorts the row numbers stably by segment -- dq_prim.hip's radix sort over the ceil(log2(G + 1))
// significant key bits -- into perm (a segment's rows ascending) and finds the G + 2 segment offsets by binary search
// of the sorted keys; once per chunk, whatever the number of analyzers.  dq_segment_scan reduces up to 64 slots
// (column view, type, op, optional filter bitmap) per segment into the state the column scan keeps for a column task
// (dq_colstats.h's ColStats, plus the filter's own row count).
//
// Reduction shape (a function of the offsets alone, never of the grid).  A segment's sorted rows are cut into tiles of
// kSegTile rows counted from its first row.  One wave reduces one tile: lane l holds rows l, l + 64, l + 128, l + 192
// of the tile and adds them in that order, the lanes meet in dq_lane.h's fixed butterfly, and the tile's moments are
// shifted sums around dq_shift.h's shift (the walk of the column scan, over the tile's four 64-row groups).  A segment
// of one tile is written where it belongs; the tiles of a longer one go to a partial array and one thread merges them
// in ascending tile order with the column scan's Chan merge (stats_merge).  So a long segment is spread over as many
// waves as it has tiles, a workgroup takes four tiles of whatever segments they belong to (four short segments per
// workgroup, not one), and two runs give the same bits.  No floating-point atomic anywhere; no atomic at all.
//
// Cost.  Every row is read once per slot through perm: a gather of 1 - 8 byte values plus a validity and a filter
// bit, all served from 64-byte sectors of which a random gather uses one value; the sort moves 12 bytes per row per
// 8-bit pass.  DESIGN.md section 2 "Segmented metrics" has the roofline reasoning, section 6 the measured figures.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "dq_colstats.h"
#include "dq_hip_host.h"
#include "dq_lane.h"
#include "dq_prim.h"
#include "dq_shift.h"

namespace dq {
namespace {

constexpr int kSegTile = DQ_SEGMENT_TILE;  // rows of a tile
constexpr int kSegGroups = kSegTile / 64;  // 64-row groups of a tile: one row per lane each
constexpr int kSegWaves = 4;               // tiles per workgroup
static_assert(kSegTile % 64 == 0 && kSegGroups >= 1, "a tile is whole 64-row groups");

struct SegSlot {  // dq_segment_slot on the device
  const void* values;
  const uint32_t* validity;
  const uint32_t* filter;
  int32_t type, op;
};

// ---- dq_segment_order ----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void seg_keys(const int32_t* __restrict__ seg, int64_t n, uint32_t G,
                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ rows) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int32_t s = seg[r];
  keys[r] = s < 0 || (uint32_t)s >= G ? G : (uint32_t)s;  // -1 (and anything else outside 0 .. G - 1): the None segment
  rows[r] = (uint32_t)r;
}

// offsets[k] = the first sorted position whose key is >= k (k = 0 .. G + 1; offsets[G + 1] = n)
__global__ __launch_bounds__(256) void seg_offsets(const uint64_t* __restrict__ sorted, int64_t n, int64_t G2,
                                                   int64_t* __restrict__ offsets) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= G2) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < (uint64_t)k) lo = mid + 1;
    else hi = mid;
  }
  offsets[k] = lo;
}

// ---- dq_segment_scan -----------------------------------------------------------------------------------------------

// tiles[s] = the tiles of segment s, parts[s] = the partial records it needs (none for a segment of one tile)
__global__ __launch_bounds__(256) void seg_tile_counts(const int64_t* __restrict__ offsets, int64_t G1,
                                                       int64_t* __restrict__ tiles, int64_t* __restrict__ parts) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s > G1) return;
  const int64_t t = s < G1 ? (offsets[s + 1] - offsets[s] + kSegTile - 1) / kSegTile : 0;  // (entry G1: the totals' slot)
  tiles[s] = t;
  parts[s] = t > 1 ? t : 0;
}

__device__ __forceinline__ bool row_bit(const uint32_t* bm, uint32_t r) { return (bm[r >> 5] >> (r & 31)) & 1u; }

// this lane's value of row r as a double; bits: the value as the wrapping int64 sum takes it (integral types)
__device__ __forceinline__ double seg_value(int32_t type, const void* v, uint32_t r, int64_t& bits) {
  switch (type) {
    case DQ_TYPE_F64: bits = 0; return reinterpret_cast<const double*>(v)[r];
    case DQ_TYPE_F32: bits = 0; return (double)reinterpret_cast<const float*>(v)[r];
    case DQ_TYPE_I64:
    case DQ_TYPE_TIMESTAMP: bits = reinterpret_cast<const int64_t*>(v)[r]; return (double)bits;
    case DQ_TYPE_I32:
    case DQ_TYPE_DATE32: bits = reinterpret_cast<const int32_t*>(v)[r]; return (double)bits;
    case DQ_TYPE_I16: bits = reinterpret_cast<const int16_t*>(v)[r]; return (double)bits;
    default: bits = reinterpret_cast<const int8_t*>(v)[r]; return (double)bits;  // DQ_TYPE_I8
  }
}

__device__ __forceinline__ void seg_store(dq_segment_state* o, const ColStats& s, int64_t applies) {
  o->n = s.n; o->mean = s.mean; o->m2 = s.m2; o->sum = s.sum; o->isum = s.isum; o->count = s.count;
  o->nan_count = s.nan_count; o->fmin = s.fmin; o->fmax = s.fmax; o->pinf_count = s.pinf; o->ninf_count = s.ninf;
  o->applies = applies;
}
__device__ __forceinline__ ColStats seg_load(const dq_segment_state* p) {
  ColStats s;
  s.n = p->n; s.mean = p->mean; s.m2 = p->m2; s.sum = p->sum; s.isum = p->isum; s.count = p->count;
  s.nan_count = p->nan_count; s.fmin = p->fmin; s.fmax = p->fmax; s.pinf = p->pinf_count; s.ninf = p->ninf_count;
  s.isum_hi = 0;
  return s;
}

// One wave per tile.  tile_off / part_off: the exclusive sums of seg_tile_counts' arrays (G1 + 1 entries; entry G1 the
// total).  out: n_slots x G1 states; partials: n_slots x part_cap records.
__global__ __launch_bounds__(64 * kSegWaves) void seg_tiles(const SegSlot* __restrict__ slots, int32_t n_slots,
                                                            const int32_t* __restrict__ perm,
                                                            const int64_t* __restrict__ offsets,
                                                            const int64_t* __restrict__ tile_off,
                                                            const int64_t* __restrict__ part_off, int64_t G1,
                                                            int64_t part_cap, dq_segment_state* __restrict__ out,
                                                            dq_segment_state* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  if (tile >= tile_off[G1]) return;  // (wave-uniform)
  // the segment of the tile: the last s with tile_off[s] <= tile (segments without rows repeat their successor's entry)
  int64_t lo = 0, hi = G1;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (tile_off[mid] <= tile) lo = mid;
    else hi = mid;
  }
  const int64_t s = lo, k = tile - tile_off[s], n_tiles = tile_off[s + 1] - tile_off[s];
  const int64_t first = offsets[s] + k * kSegTile;
  const int32_t rows = (int32_t)min((int64_t)kSegTile, offsets[s + 1] - first);
  uint32_t r[kSegGroups];
  uint64_t in[kSegGroups];  // the tile's rows, as lane masks
#pragma unroll
  for (int j = 0; j < kSegGroups; ++j) {
    const bool ok = 64 * j + lane < rows;
    r[j] = ok ? (uint32_t)perm[first + 64 * j + lane] : 0u;
    in[j] = __builtin_amdgcn_ballot_w64(ok);
  }
  for (int32_t q = 0; q < n_slots; ++q) {
    const SegSlot sl = slots[q];
    dq_segment_state* dst = n_tiles == 1 ? out + (size_t)q * G1 + s : partials + (size_t)q * part_cap + part_off[s] + k;
    uint64_t fm[kSegGroups], vm[kSegGroups];  // rows the filter keeps; of those, the non-null ones
    int64_t applies = 0;
    ColStats st;
    stats_init(st);
#pragma unroll
    for (int j = 0; j < kSegGroups; ++j) {
      const bool f = lane_bit(in[j]) && (!sl.filter || row_bit(sl.filter, r[j]));
      const bool v = f && (!sl.validity || row_bit(sl.validity, r[j]));
      fm[j] = __builtin_amdgcn_ballot_w64(f);
      vm[j] = __builtin_amdgcn_ballot_w64(v);
      applies += __builtin_popcountll(fm[j]);
      st.count += __builtin_popcountll(vm[j]);
    }
    if (sl.op == DQ_SEG_STATS) {
      const bool fp = sl.type == DQ_TYPE_F64 || sl.type == DQ_TYPE_F32;
      double x[kSegGroups];
      int64_t bits[kSegGroups];
      uint64_t mm[kSegGroups], xm[kSegGroups];  // rows in the moments (no +-inf); rows in min / max (no NaN)
      int64_t n_mom = 0;
#pragma unroll
      for (int j = 0; j < kSegGroups; ++j) {
        bits[j] = 0;
        x[j] = lane_bit(vm[j]) ? seg_value(sl.type, sl.values, r[j], bits[j]) : 0.0;
        const uint64_t nanm = __builtin_amdgcn_ballot_w64(x[j] != x[j]) & vm[j];
        const uint64_t inf = __builtin_amdgcn_ballot_w64(!__builtin_isfinite(x[j])) & vm[j] & ~nanm;
        const uint64_t pinf = __builtin_amdgcn_ballot_w64(x[j] > 0.0) & inf;
        st.nan_count += __builtin_popcountll(nanm);
        st.pinf += __builtin_popcountll(pinf);
        st.ninf += __builtin_popcountll(inf & ~pinf);
        mm[j] = vm[j] & ~inf;
        xm[j] = vm[j] & ~nanm;
        n_mom += __builtin_popcountll(mm[j]);
      }
      // the column scan's shift over the tile's groups: the first with kShiftMinRows selected rows starts the walk
      int64_t g0 = 0;
#pragma unroll
      for (int j = kSegGroups - 1; j >= 0; --j)
        if (__builtin_popcountll(vm[j]) >= kShiftMinRows) g0 = j;
      const double shift = groups_shift(
          kSegGroups, g0,
          [&](int64_t g) {
            uint64_t w = vm[0];
#pragma unroll
            for (int j = 1; j < kSegGroups; ++j) w = g == j ? vm[j] : w;
            return w;
          },
          [&](int64_t g) {
            double w = x[0];
#pragma unroll
            for (int j = 1; j < kSegGroups; ++j) w = g == j ? x[j] : w;
            return w;
          });
      double sd = 0.0, sdd = 0.0, mn = st.fmin, mx = st.fmax;
      int64_t is = 0;
#pragma unroll
      for (int j = 0; j < kSegGroups; ++j) {  // this lane's rows in tile order
        if (lane_bit(mm[j])) {
          const double d = x[j] - shift;
          sd += d;
          sdd = __builtin_fma(d, d, sdd);
          is = (int64_t)((uint64_t)is + (uint64_t)bits[j]);
        }
        if (lane_bit(xm[j])) {
          mn = hw_min(mn, x[j]);
          mx = hw_max(mx, x[j]);
        }
      }
      const double S1 = wave_sum_f64(sd), S2 = wave_sum_f64(sdd);
      is = wave_sum_i64(is);
      st.fmin = wave_min(mn);
      st.fmax = wave_max(mx);
      if (n_mom > 0) {  // (n, mean, m2) from the shifted sums, as the column scan closes a range
        const double n = (double)n_mom, m = S1 / n;
        st.n = n;
        st.mean = shift + m;
        const double m2 = __builtin_fma(-S1, m, S2);
        st.m2 = m2 < 0.0 ? 0.0 : m2;  // rounding can leave a constant tile's m2 at -ulp; a NaN stays NaN
        if (fp) st.sum = __builtin_fma(n, shift, S1);
        else st.isum = is;
      }
    }
    if (lane == 0) seg_store(dst, st, applies);
  }
}

// One thread per (slot, segment): a segment without rows gets the empty state, a segment of several tiles its
// partials merged in ascending tile order; a segment of one tile was written by its wave.
__global__ __launch_bounds__(256) void seg_merge(int32_t n_slots, const int64_t* __restrict__ tile_off,
                                                 const int64_t* __restrict__ part_off, int64_t G1, int64_t part_cap,
                                                 dq_segment_state* __restrict__ out,
                                                 const dq_segment_state* __restrict__ partials) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G1 * n_slots) return;
  const int64_t q = i / G1, s = i - q * G1, n_tiles = tile_off[s + 1] - tile_off[s];
  if (n_tiles == 1) return;
  ColStats acc;
  stats_init(acc);
  int64_t applies = 0;
  const dq_segment_state* p = partials + (size_t)q * part_cap + part_off[s];
  for (int64_t k = 0; k < n_tiles; ++k) {
    stats_merge(acc, seg_load(p + k));
    applies += p[k].applies;
  }
  seg_store(out + i, acc, applies);
}

bool seg_type_ok(int32_t t) {
  return t == DQ_TYPE_F64 || t == DQ_TYPE_F32 || t == DQ_TYPE_I64 || t == DQ_TYPE_I32 || t == DQ_TYPE_I16 ||
         t == DQ_TYPE_I8 || t == DQ_TYPE_DATE32 || t == DQ_TYPE_TIMESTAMP;
}

int grid_of(int64_t items, int per) { return (int)std::max<int64_t>(1, (items + per - 1) / per); }

}  // namespace
}  // namespace dq

using namespace dq;

extern "C" {

int32_t dq_segment_tile(void) { return kSegTile; }

dq_status dq_segment_order(const int32_t* seg, int64_t n_rows, int64_t G, int32_t* perm, int64_t* offsets,
                           void* hip_stream) {
  const char* me = "dq_segment_order";
  if (n_rows < 0 || n_rows > 0x7FFFFFFFll) return set_error(DQ_E_INVALID, "%s: n_rows %lld out of range", me, (long long)n_rows);
  if (G < 0) return set_error(DQ_E_INVALID, "%s: G %lld is negative", me, (long long)G);
  if (G + 1 > 0x7FFFFFFFll)
    return set_error(DQ_E_UNSUPPORTED, "%s: %lld segments and the NULL segment exceed int32", me, (long long)G);
  if (!offsets) return set_error(DQ_E_INVALID, "%s: offsets is NULL", me);
  if (n_rows > 0 && (!seg || !perm)) return set_error(DQ_E_INVALID, "%s: seg / perm is NULL", me);
  hipStream_t S = static_cast<hipStream_t>(hip_stream);
  if (n_rows == 0) {
    DQ_HIP(hipMemsetAsync(offsets, 0, (size_t)(G + 2) * sizeof(int64_t), S));
    DQ_HIP(hipStreamSynchronize(S));
    return DQ_OK;
  }
  int bits = 0;  // the significant bits of the keys 0 .. G
  while (((int64_t)1 << bits) <= G) ++bits;
  const size_t n = (size_t)n_rows, sort_bytes = bits ? prim::sort_temp_bytes(n_rows, 4) : 0;
  // keys | sorted keys | row numbers | the sort's scratch
  const size_t o_sorted = n * 8, o_rows = 2 * n * 8, o_tmp = (o_rows + n * 4 + 255) & ~(size_t)255;
  StreamBuf buf;
  DQ_HIP(buf.alloc(o_tmp + sort_bytes, S));
  char* base = static_cast<char*>(buf.get());
  uint64_t* keys = reinterpret_cast<uint64_t*>(base);
  uint64_t* sorted = reinterpret_cast<uint64_t*>(base + o_sorted);
  uint32_t* rows = reinterpret_cast<uint32_t*>(base + o_rows);
  // without a key bit every row is in segment 0 (G = 0: the NULL segment alone): the row numbers are the order
  hipLaunchKernelGGL(seg_keys, dim3(grid_of(n_rows, 256)), dim3(256), 0, S, seg, n_rows, (uint32_t)G, keys,
                     bits ? rows : reinterpret_cast<uint32_t*>(perm));
  DQ_HIP(hipGetLastError());
  if (bits) DQ_HIP(prim::sort_pairs(keys, sorted, rows, perm, 4, n_rows, 0, bits, false, base + o_tmp, sort_bytes, S));
  hipLaunchKernelGGL(seg_offsets, dim3(grid_of(G + 2, 256)), dim3(256), 0, S, bits ? sorted : keys, n_rows, G + 2,
                     offsets);
  DQ_HIP(hipGetLastError());
  DQ_HIP(hipStreamSynchronize(S));
  return DQ_OK;
}

dq_status dq_segment_scan(const dq_segment_slot* slots, int32_t n_slots, const int32_t* perm, const int64_t* offsets,
                          int64_t G1, dq_segment_state* out, void* hip_stream) {
  const char* me = "dq_segment_scan";
  if (n_slots < 1 || n_slots > DQ_SEGMENT_MAX_SLOTS)
    return set_error(DQ_E_INVALID, "%s: n_slots %d out of range (1 .. %d)", me, n_slots, DQ_SEGMENT_MAX_SLOTS);
  if (G1 < 1) return set_error(DQ_E_INVALID, "%s: G1 %lld out of range (at least the NULL segment)", me, (long long)G1);
  if (G1 > 0x7FFFFFFFll) return set_error(DQ_E_UNSUPPORTED, "%s: %lld segments exceed int32", me, (long long)G1);
  if (!slots || !offsets || !out) return set_error(DQ_E_INVALID, "%s: slots / offsets / out is NULL", me);
  SegSlot h[DQ_SEGMENT_MAX_SLOTS];
  for (int32_t q = 0; q < n_slots; ++q) {
    const dq_segment_slot& a = slots[q];
    if (a.op != DQ_SEG_COUNT && a.op != DQ_SEG_STATS) return set_error(DQ_E_INVALID, "%s: slot %d: unknown op %d", me, q, a.op);
    if (a.op == DQ_SEG_STATS) {
      if (!type_valid(a.type)) return set_error(DQ_E_INVALID, "%s: slot %d: unknown type %d", me, q, a.type);
      if (!seg_type_ok(a.type))
        return set_error(DQ_E_UNSUPPORTED, "%s: slot %d: type %d has no segmented statistics", me, q, a.type);
      if (!a.col.values) return set_error(DQ_E_INVALID, "%s: slot %d: values is NULL", me, q);
    }
    if (((uintptr_t)a.col.validity | (uintptr_t)a.filter) & 3)
      return set_error(DQ_E_INVALID, "%s: slot %d: a bitmap is not 4-byte aligned", me, q);
    h[q] = SegSlot{a.col.values, reinterpret_cast<const uint32_t*>(a.col.validity),
                   reinterpret_cast<const uint32_t*>(a.filter), a.type, a.op};
  }
  hipStream_t S = static_cast<hipStream_t>(hip_stream);
  int64_t n_rows = 0;
  DQ_HIP(hipMemcpyAsync(&n_rows, offsets + G1, sizeof(n_rows), hipMemcpyDeviceToHost, S));
  DQ_HIP(hipStreamSynchronize(S));
  if (n_rows < 0 || n_rows > 0x7FFFFFFFll) return set_error(DQ_E_INVALID, "%s: offsets end at %lld rows", me, (long long)n_rows);
  if (n_rows > 0 && !perm) return set_error(DQ_E_INVALID, "%s: perm is NULL", me);
  // a segment has a partial record per tile only if it has several: at most 2 rows / tile records; every segment
  // with a row has a tile: at most rows / tile + min(G1, rows) tiles
  const int64_t part_cap = 2 * (n_rows / kSegTile) + 2, max_tiles = n_rows / kSegTile + std::min(G1, n_rows);
  const size_t b_off = ((size_t)(G1 + 1) * 8 + 255) & ~(size_t)255, b_scan = (prim::scan_temp_bytes(G1 + 1) + 255) & ~(size_t)255;
  const size_t b_slots = (sizeof(SegSlot) * DQ_SEGMENT_MAX_SLOTS + 255) & ~(size_t)255;
  StreamBuf buf;
  DQ_HIP(buf.alloc(2 * b_off + b_scan + b_slots + (size_t)n_slots * part_cap * sizeof(dq_segment_state), S));
  char* base = static_cast<char*>(buf.get());
  int64_t* tile_off = reinterpret_cast<int64_t*>(base);
  int64_t* part_off = reinterpret_cast<int64_t*>(base + b_off);
  void* scan_tmp = base + 2 * b_off;
  SegSlot* d_slots = reinterpret_cast<SegSlot*>(base + 2 * b_off + b_scan);
  dq_segment_state* partials = reinterpret_cast<dq_segment_state*>(base + 2 * b_off + b_scan + b_slots);
  DQ_HIP(hipMemcpyAsync(d_slots, h, sizeof(SegSlot) * n_slots, hipMemcpyHostToDevice, S));
  hipLaunchKernelGGL(seg_tile_counts, dim3(grid_of(G1 + 1, 256)), dim3(256), 0, S, offsets, G1, tile_off, part_off);
  DQ_HIP(hipGetLastError());
  DQ_HIP(prim::exclusive_sum_i64(tile_off, tile_off, G1 + 1, scan_tmp, S));
  DQ_HIP(prim::exclusive_sum_i64(part_off, part_off, G1 + 1, scan_tmp, S));
  if (max_tiles > 0) {
    hipLaunchKernelGGL(seg_tiles, dim3(grid_of(max_tiles, kSegWaves)), dim3(64 * kSegWaves), 0, S, d_slots, n_slots, perm,
                       offsets, tile_off, part_off, G1, part_cap, out, partials);
    DQ_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(seg_merge, dim3(grid_of(G1 * n_slots, 256)), dim3(256), 0, S, n_slots, tile_off, part_off, G1,
                     part_cap, out, partials);
  DQ_HIP(hipGetLastError());
  DQ_HIP(hipStreamSynchronize(S));  // (h and the temporaries are this call's)
  return DQ_OK;
}

}  // extern "C"
