// dq_group.hip -- frequencies of the grouping analyzers on the GPU (sort-based group-by count).
//
// Reference: FrequencyBasedAnalyzer.computeFrequencies (analyzers/GroupingAnalyzers.scala:44-82):
//   SELECT cols, COUNT(*) FROM data WHERE col_1 IS NOT NULL AND ... GROUP BY cols
// plus numRows = data.count(), and the metrics of Uniqueness / Distinctness / CountDistinct /
// Entropy / UniqueValueRatio, which only need the multiset of group counts (Uniqueness.scala:27-29,
// Distinctness.scala:29-31, CountDistinct.scala:25-31, Entropy.scala:29-41, UniqueValueRatio.scala:25-36).
// FrequenciesAndNumRows.sum (GroupingAnalyzers.scala:118-138) = outer join adding counts.
//
// Layout: every row whose grouping columns are all non-null yields one 64-bit key.  A single 8-byte /
// 4-byte numeric column is its own exact key (f64: NaN canonicalised as Spark's UnsafeRow.setDouble
// does; -0.0 and 0.0 stay distinct groups in Spark 2.2).  Otherwise (strings, several columns) the key
// is a 64-bit hash of the tuple, the rows ride along the sort, and every pair of neighbours with equal
// keys is compared exactly: a collision between distinct tuples is reported (DQ_E_UNSUPPORTED), never
// merged silently.  Keys are radix-sorted and run-length encoded into (key, count) groups by dq_prim.hip's
// hand-written kernels; the summary is a fixed-order two-level reduction, so results are deterministic.  A hashed table also
// keeps a second, independently seeded 64-bit hash per group (its representative row's tuple), so that
// dq_freq_merge -- which no longer has the rows -- detects two distinct tuples whose first hashes collide
// (equal first hash, different second hash: DQ_E_UNSUPPORTED) instead of adding their counts.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "dq_arena.h"
#include "dq_device.h"
#include "dq_freq_image.h"
#include "dq_freq_table.h"
#include "dq_hash.h"
#include "dq_hip_host.h"
#include "dq_prim.h"
#include "dq_strkey.h"

namespace dq {
namespace {

// (kMaxGroupCols, GroupCols, the value-bits rule and tuple_equal_rows: dq_freq_table.h)
constexpr int kMaxGroupChunks = 4096;
constexpr int kRowBits = 40;  // row id = chunk << 40 | row

constexpr uint64_t kSeed2 = 0x9E3779B97F4A7C15ull;  // seed of the second (verification) tuple hash

__device__ __forceinline__ bool row_valid(const GroupCols& g, int64_t r) {
  if (g.weight && g.weight[r] <= 0) return false;
  for (int c = 0; c < g.n_cols; ++c)
    if (g.validity[c] && !((g.validity[c][r >> 5] >> (r & 31)) & 1u)) return false;
  return true;
}

// 64-bit hash of the row's tuple (columns in order; strings by bytes and length)
__device__ uint64_t tuple_hash(const GroupCols& g, int64_t r, uint64_t seed = kSeed) {
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
__device__ uint64_t tuple_key(const GroupCols& g, int64_t r) { return tuple_hash(g, r) & g.key_mask; }

__device__ bool tuple_equal(const GroupCols* chunks, uint64_t ra, uint64_t rb) {
  return tuple_equal_rows(chunks[ra >> kRowBits], chunks[rb >> kRowBits], (int64_t)(ra & ((1ull << kRowBits) - 1)),
                          (int64_t)(rb & ((1ull << kRowBits) - 1)));
}

// The non-null rows' keys (and, hashed, their row ids) of a chunk appended to out_keys / out_rows at the launch-wide
// cursor, in no particular order (the radix sort comes next; any row of a group may represent it: its tuple equals
// the others').  A workgroup takes kCompactRows rows per tile, ballots its rows' validity, and reserves the tile's
// slots with one global atomic.  (Replaced group_keys + hipCUB's order-preserving DeviceSelect::Flagged, one per
// output array: 3.0 ms per 1e8 rows and select, r4g2.)
constexpr int kCompactPer = 8;                        // rows per thread and tile
constexpr int kCompactRows = 256 * kCompactPer;
// cursor[0]: the append cursor; cursor[1] / cursor[2]: AND / OR of every appended key (their XOR has the bits in
// which the keys differ: the radix sort skips the common high bits)
// HASHED: keys are tuple hashes (any columns); else one numeric column whose value bits are the keys -- its next
// tile's values and validity words are loaded before this tile's work (in flight behind it)
// SEL: only the rows whose bit is set in `sel` take part -- the chunk's selection bitmap, read as the 32-bit words the
// validity is read as (a little-endian uint64_t word is its two uint32_t halves in row order), so the unhashed path
// ANDs it into the prefetched validity word and the hashed path tests it before the row is hashed
template <bool HASHED, bool SEL>
__global__ __launch_bounds__(256) void group_compact(GroupCols g, int64_t n, int64_t chunk,
                                                     uint64_t* __restrict__ out_keys, uint64_t* __restrict__ out_rows,
                                                     unsigned long long* __restrict__ cursor,
                                                     const uint32_t* __restrict__ sel) {
  __shared__ uint32_t wave_n[4];
  __shared__ unsigned long long tile_base;
  __shared__ unsigned long long wave_and[4], wave_or[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool hashed = HASHED;
  uint64_t k_and = ~0ull, k_or = 0;
  const int64_t tstride = (int64_t)gridDim.x * kCompactRows;
  uint64_t nval[HASHED ? 1 : kCompactPer];
  uint32_t nvw[HASHED ? 1 : kCompactPer];
  auto fetch = [&](int64_t t0) __attribute__((always_inline)) {
    if constexpr (!HASHED) {
#pragma unroll
      for (int u = 0; u < kCompactPer; ++u) {
        const int64_t r = t0 + u * 256 + threadIdx.x;
        nval[u] = 0;
        nvw[u] = 0;
        if (r < n) {
          nval[u] = value_bits(g, 0, r);
          nvw[u] = g.validity[0] ? g.validity[0][r >> 5] : 0xFFFFFFFFu;
          if constexpr (SEL) nvw[u] &= sel[r >> 5];
        }
      }
    }
  };
  fetch((int64_t)blockIdx.x * kCompactRows);
  for (int64_t t0 = (int64_t)blockIdx.x * kCompactRows; t0 < n; t0 += tstride) {
    uint64_t key[kCompactPer];
    uint64_t bal[kCompactPer];
    uint32_t cnt = 0;
    uint64_t cval[HASHED ? 1 : kCompactPer];
    uint32_t cvw[HASHED ? 1 : kCompactPer];
    if constexpr (!HASHED) {
#pragma unroll
      for (int u = 0; u < kCompactPer; ++u) {
        cval[u] = nval[u];
        cvw[u] = nvw[u];
      }
      if (t0 + tstride < n) fetch(t0 + tstride);
    }
#pragma unroll
    for (int u = 0; u < kCompactPer; ++u) {
      const int64_t r = t0 + u * 256 + threadIdx.x;
      bool v;
      if constexpr (HASHED) {
        if constexpr (SEL) v = r < n && ((sel[r >> 5] >> (r & 31)) & 1u) && row_valid(g, r);
        else v = r < n && row_valid(g, r);
        key[u] = v ? tuple_key(g, r) : 0;
      } else {
        v = r < n && ((cvw[u] >> (r & 31)) & 1u);
        key[u] = v ? cval[u] : 0;
      }
      if (v) {
        k_and &= key[u];
        k_or |= key[u];
      }
      bal[u] = __builtin_amdgcn_ballot_w64(v);
      cnt += (uint32_t)__builtin_popcountll(bal[u]);
    }
    if (lane == 0) wave_n[wave] = cnt;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wave_n[w] : 0u;
      total += wave_n[w];
    }
    if (threadIdx.x == 0 && total) tile_base = atomicAdd(cursor, (unsigned long long)total);
    __syncthreads();
    unsigned long long pos = tile_base + before;
#pragma unroll
    for (int u = 0; u < kCompactPer; ++u) {
      if ((bal[u] >> lane) & 1ull) {
        const unsigned long long at =
            pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[u], 0u));
        out_keys[at] = key[u];
        if (hashed) out_rows[at] = ((uint64_t)chunk << kRowBits) | (uint64_t)(t0 + u * 256 + threadIdx.x);
      }
      pos += (unsigned long long)__builtin_popcountll(bal[u]);
    }
    __syncthreads();  // wave_n / tile_base are rewritten by the next tile
  }
  // the workgroup's AND / OR: lanes, then waves, then one atomic pair
  for (int d = 32; d >= 1; d >>= 1) {
    k_and &= __shfl_xor(k_and, d);
    k_or |= __shfl_xor(k_or, d);
  }
  if (lane == 0) {
    wave_and[wave] = k_and;
    wave_or[wave] = k_or;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t a = wave_and[0] & wave_and[1] & wave_and[2] & wave_and[3];
    const uint64_t o = wave_or[0] | wave_or[1] | wave_or[2] | wave_or[3];
    if (a != ~0ull) atomicAnd(&cursor[1], (unsigned long long)a);
    if (o != 0) atomicOr(&cursor[2], (unsigned long long)o);
  }
}

// neighbours with equal hash keys must hold equal tuples.  A wave takes 64 consecutive sorted positions; a position
// that continues a run is compared with the run's first position within the wave (found from the ballot of run
// heads), or -- the wave's first position -- with the one before it: by transitivity every run is checked exactly,
// and the compared-against tuple is shared by the wave's lanes of a run, so its scattered loads hit the cache (a
// column of few distinct values used to load two random strings per pair).  ONE: a single chunk, whose column
// descriptor comes in the kernel arguments (scalar loads) instead of from a per-row lookup in global memory
template <bool ONE>
__global__ void verify_runs(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ rows, int64_t n,
                            const GroupCols* __restrict__ chunks, GroupCols g0, int32_t* __restrict__ collision) {
  const uint64_t rmask = (1ull << kRowBits) - 1ull;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;  // a multiple of 64: waves stay 64-aligned
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < n; i0 += stride) {
    const int64_t i = i0 + lane;
    const bool in = i < n;
    const uint64_t k = in ? keys[i] : 0ull;
    const bool head = !in || i == 0 || keys[i - 1] != k;
    const uint64_t heads = __builtin_amdgcn_ballot_w64(head);
    if (head) continue;
    const uint64_t upto = heads & (lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull));
    const int first = upto ? 63 - __builtin_clzll(upto) : 0;  // the run's first lane in this wave (< lane), or 0
    const int64_t partner = lane == 0 ? i - 1 : i0 + first;
    const uint64_t ra = rows[partner], rb = rows[i];
    const bool eq = ONE ? tuple_equal_rows(g0, g0, (int64_t)(ra & rmask), (int64_t)(rb & rmask)) : tuple_equal(chunks, ra, rb);
    if (!eq) atomicOr(collision, 1);
  }
}

// The compaction-order form of the exact check, for tables of few groups (most rows share their group with many
// others: the sorted-order check then loads one scattered string per row).  It walks the keys and row ids as the
// compaction kernel appended them (each workgroup tile's rows in row order, so a row's own tuple is read nearly
// sequentially), finds the row's group by binary search of its key in the table's sorted group keys (LDS-sampled),
// and compares
// the row with the group's representative row, whose tuple the group's rows share (cache hits).
constexpr int kVSample = 2048;  // group keys sampled into LDS: the search's first steps
template <bool ONE>
__global__ __launch_bounds__(256) void verify_compacted(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ rows,
                                                        int64_t nv, const uint64_t* __restrict__ gkeys, int64_t G,
                                                        const uint64_t* __restrict__ rep, const GroupCols* __restrict__ chunks,
                                                        GroupCols g0, int32_t* __restrict__ collision) {
  __shared__ uint64_t smp[kVSample];  // every stride-th group key (all of them for G <= 2048)
  const uint64_t rmask = (1ull << kRowBits) - 1ull;
  const int64_t stride = (G + kVSample - 1) / kVSample;
  const int ns = (int)((G + stride - 1) / stride);
  for (int s = threadIdx.x; s < ns; s += blockDim.x) smp[s] = gkeys[(int64_t)s * stride];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = keys[i], self = rows[i];
    int lo = 0, hi = ns - 1;  // the last sample <= k (k is one of the group keys, so smp[0] <= k)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (smp[mid] <= k) lo = mid;
      else hi = mid - 1;
    }
    int64_t a = (int64_t)lo * stride, b = (a + stride < G ? a + stride : G) - 1;  // then within its stride
    while (a < b) {
      const int64_t mid = (a + b) >> 1;
      if (gkeys[mid] < k) a = mid + 1;
      else b = mid;
    }
    const uint64_t rp = rep[a];
    if (rp == self) continue;
    const bool eq = ONE ? tuple_equal_rows(g0, g0, (int64_t)(rp & rmask), (int64_t)(self & rmask))
                        : tuple_equal(chunks, rp, self);
    if (!eq) atomicOr(collision, 1);
  }
}

constexpr int kSumBlocks = 1024;
constexpr int64_t kRowOrderVerify = 8;  // compaction-order check when the table has <= 1 group per 8 grouped rows
constexpr int64_t kCompactedMaxGroups = 1 << 16;  // ... and its group keys (the binary search) stay cache-resident
struct SumPart { int64_t unique; double ent; };

// fixed-order partials: block b sums groups b, b + kSumBlocks, ... in a fixed tree
__global__ __launch_bounds__(256) void summary_part(const int64_t* __restrict__ counts, int64_t n, double num_rows,
                                                    SumPart* __restrict__ part) {
  __shared__ int64_t su[256];
  __shared__ double se[256];
  int64_t u = 0;
  double e = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double c = (double)counts[i];
    u += counts[i] == 1 ? 1 : 0;
    // Entropy.scala:31-37: -(count / numRows) * ln(count / numRows), 0 for a zero count
    if (c != 0.0) e += -(c / num_rows) * log(c / num_rows);
  }
  su[threadIdx.x] = u;
  se[threadIdx.x] = e;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) { su[threadIdx.x] += su[threadIdx.x + s]; se[threadIdx.x] += se[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = SumPart{su[0], se[0]};
}

__global__ void summary_final(const SumPart* __restrict__ part, int32_t nparts, SumPart* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    SumPart t{0, 0.0};
    for (int i = 0; i < nparts; ++i) { t.unique += part[i].unique; t.ent += part[i].ent; }
    *out = t;
  }
}

// key of one column of a row (exact value for numeric columns, 64-bit hash of the bytes for strings)
__device__ uint64_t col_key(const GroupCols& g, int c, int64_t r) {
  if (g.type[c] != DQ_TYPE_UTF8 && g.type[c] != DQ_TYPE_LARGE_UTF8 && !is_dec(g.type[c])) return value_bits(g, c, r);
  GroupCols one = g;
  one.n_cols = 1;
  one.values[0] = g.values[c];
  one.offsets[0] = g.offsets[c];
  one.type[0] = g.type[c];
  return tuple_key(one, r);
}

__device__ bool col_equal(const GroupCols* chunks, int c, uint64_t ra, uint64_t rb) {
  const GroupCols& ga = chunks[ra >> kRowBits];
  const GroupCols& gb = chunks[rb >> kRowBits];
  const int64_t a = (int64_t)(ra & ((1ull << kRowBits) - 1)), b = (int64_t)(rb & ((1ull << kRowBits) - 1));
  if (is_dec(ga.type[c])) {
    const uint64_t *va = dec_at(ga, c, a), *vb = dec_at(gb, c, b);
    return va[0] == vb[0] && va[1] == vb[1];
  }
  if (ga.type[c] != DQ_TYPE_UTF8 && ga.type[c] != DQ_TYPE_LARGE_UTF8) return value_bits(ga, c, a) == value_bits(gb, c, b);
  const uint8_t *pa, *pb;
  int64_t la, lb;
  str_of(ga, c, a, pa, la);
  str_of(gb, c, b, pb, lb);
  if (la != lb) return false;
  for (int64_t i = 0; i < la; ++i)
    if (pa[i] != pb[i]) return false;
  return true;
}

// MutualInformation: per joint group g its representative row and the keys of both columns
__global__ void mi_group_keys(const uint64_t* __restrict__ sorted_rows, const int64_t* __restrict__ starts, int64_t G,
                              const GroupCols* __restrict__ chunks, uint64_t* __restrict__ rep, uint64_t* __restrict__ xk,
                              uint64_t* __restrict__ yk, uint64_t* __restrict__ idx) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t r = sorted_rows[starts[g]];
    const GroupCols& gc = chunks[r >> kRowBits];
    const int64_t lr = (int64_t)(r & ((1ull << kRowBits) - 1));
    rep[g] = r;
    xk[g] = col_key(gc, 0, lr);
    yk[g] = col_key(gc, 1, lr);
    idx[g] = (uint64_t)g;
  }
}

// marginal of column c over the joint groups sorted by that column's key: segment heads, an exact
// check of equal-hash neighbours (strings), then segment sums of the joint counts (integer atomics)
__global__ void mi_heads(const uint64_t* __restrict__ sk, const uint64_t* __restrict__ sidx, const uint64_t* __restrict__ rep,
                         int64_t G, const GroupCols* __restrict__ chunks, int c, uint32_t* __restrict__ head,
                         int32_t* __restrict__ collision) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (int64_t)gridDim.x * blockDim.x) {
    const bool h = i == 0 || sk[i] != sk[i - 1];
    head[i] = h ? 1u : 0u;
    if (!h && !col_equal(chunks, c, rep[sidx[i]], rep[sidx[i - 1]])) atomicOr(collision, 1);
  }
}
__global__ void mi_segsum(const uint64_t* __restrict__ sidx, const uint32_t* __restrict__ seg, const int64_t* __restrict__ gc,
                          int64_t G, unsigned long long* __restrict__ segsum) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&segsum[seg[i] - 1], (unsigned long long)gc[sidx[i]]);
}
__global__ void mi_scatter(const uint64_t* __restrict__ sidx, const uint32_t* __restrict__ seg,
                           const unsigned long long* __restrict__ segsum, int64_t G, int64_t* __restrict__ pm) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (int64_t)gridDim.x * blockDim.x)
    pm[sidx[i]] = (int64_t)segsum[seg[i] - 1];
}
// fixed-order partial sums of (pxy / N) * ln((pxy / N) / ((px / N) * (py / N)))  (MutualInformation.scala:53-56)
__global__ __launch_bounds__(256) void mi_part(const int64_t* __restrict__ gc, const int64_t* __restrict__ px,
                                               const int64_t* __restrict__ py, int64_t G, double total,
                                               double* __restrict__ part) {
  __shared__ double se[256];
  double e = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < G; i += (int64_t)gridDim.x * 256) {
    const double pxy = (double)gc[i], a = (double)px[i], b = (double)py[i];
    e += (pxy / total) * log((pxy / total) / ((a / total) * (b / total)));
  }
  se[threadIdx.x] = e;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) se[threadIdx.x] += se[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = se[0];
}
__global__ void mi_final(const double* __restrict__ part, int32_t nparts, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < nparts; ++i) t += part[i];
    *out = t;
  }
}

Arena<DeviceMem> g_arena;  // the scratch of every grouping call (dq_arena.h; Frame, take, read_back: dq_freq_table.h)

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

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(8192, (n + 255) / 256)); }

}  // namespace
}  // namespace dq

namespace dq {
Arena<DeviceMem>& group_arena() { return g_arena; }
}  // namespace dq

using namespace dq;

namespace dq {
namespace {
__global__ void gather_rep(const uint64_t* __restrict__ sorted_rows, const int64_t* __restrict__ starts, int64_t G,
                           uint64_t* __restrict__ rep) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x)
    rep[g] = sorted_rows[starts[g]];
}
// a weighted table (dq_freq_build_weighted): counts[g], on entry the length of group g's run of the sorted row ids,
// becomes the sum of those rows' weights; *total += every group's (one thread per group: a run is the entries that
// share a value, a few)
__global__ void weighted_counts(const uint64_t* __restrict__ sorted_rows, const int64_t* __restrict__ starts, int64_t G,
                                const GroupCols* __restrict__ chunks, int64_t* __restrict__ counts,
                                unsigned long long* __restrict__ total) {
  int64_t mine = 0;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = starts[g], n = counts[g];
    int64_t sum = 0;
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t r = sorted_rows[s + i];
      sum += chunks[r >> kRowBits].weight[r & ((1ull << kRowBits) - 1)];
    }
    counts[g] = sum;
    mine += sum;
  }
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, (unsigned long long)mine);
}
// The dictionary form of a low-cardinality table (dict_table): the keys of an evenly spaced sample of the compacted
// keys (with their row ids), then every compacted key counted against the sample's distinct keys.
__global__ void dict_sample(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ rows, int64_t n, int m,
                            uint64_t* __restrict__ skeys, uint64_t* __restrict__ srows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int64_t r = (int64_t)i * (n / m) + ((int64_t)i * (n % m)) / m;  // floor(i n / m), m <= kDictSample
  skeys[i] = keys[r];
  if (rows) srows[i] = rows[r];
}

constexpr int kDictMax = 2048;      // distinct sample keys the dictionary form takes (LDS: 16 KB keys + 8 KB counts)
constexpr int kDictSample = 16384;  // keys sampled: by default the form needs >= 16 samples per distinct key, so a
                                    // group of >= 1 / 1024 of the keys is missed with probability < e^-16
// the distinct keys of the sorted sample (one workgroup of 1024 threads, 16 consecutive keys each): unique[0 .. *nd)
__global__ __launch_bounds__(1024) void dict_unique(const uint64_t* __restrict__ sorted, int m,
                                                    uint64_t* __restrict__ unique, int64_t* __restrict__ nd) {
  __shared__ int part[1024];
  constexpr int kPer = kDictSample / 1024;
  const int t = threadIdx.x, i0 = t * kPer;
  int heads = 0;
  for (int j = 0; j < kPer; ++j) {
    const int i = i0 + j;
    heads += (i < m && (i == 0 || sorted[i] != sorted[i - 1])) ? 1 : 0;
  }
  part[t] = heads;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // inclusive scan of the per-thread head counts
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int at = part[t] - heads;
  for (int j = 0; j < kPer; ++j) {
    const int i = i0 + j;
    if (i < m && (i == 0 || sorted[i] != sorted[i - 1])) unique[at++] = sorted[i];
  }
  if (t == 1023) nd[0] = part[1023];
}
// rep[g] = the smallest sampled row id of group g (every sampled key is one of dict's nd keys; rep preset to ~0)
__global__ void dict_rep(const uint64_t* __restrict__ skeys, const uint64_t* __restrict__ srows, int m,
                         const uint64_t* __restrict__ dict, int nd, unsigned long long* __restrict__ rep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t k = skeys[i];
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (dict[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  atomicMin(&rep[lo], (unsigned long long)srows[i]);
}
constexpr int kDictPer = 4;         // keys per thread and iteration (independent searches in flight)
// counts[g] += #{compacted keys == dict[g]} (dict: nd sorted distinct keys, pw = the power of two >= nd); a key
// outside the dictionary raises *miss (the caller then sorts instead)
__global__ __launch_bounds__(256) void dict_count(const uint64_t* __restrict__ keys, int64_t n,
                                                  const uint64_t* __restrict__ dict, int nd, int pw,
                                                  unsigned long long* __restrict__ counts, int32_t* __restrict__ miss) {
  __shared__ uint64_t d[kDictMax];
  __shared__ uint32_t c[kDictMax];
  for (int i = threadIdx.x; i < nd; i += 256) {
    d[i] = dict[i];
    c[i] = 0;
  }
  __syncthreads();
  bool missed = false;
  const int64_t stride = (int64_t)gridDim.x * 256 * kDictPer;
  for (int64_t base = (int64_t)blockIdx.x * 256 * kDictPer; base < n; base += stride) {
    uint64_t k[kDictPer];
    int pos[kDictPer];
#pragma unroll
    for (int u = 0; u < kDictPer; ++u) {
      const int64_t i = base + u * 256 + threadIdx.x;
      k[u] = i < n ? __builtin_nontemporal_load(keys + i) : d[0];
      pos[u] = 0;
    }
    for (int step = pw >> 1; step > 0; step >>= 1) {  // the last dictionary key <= k
#pragma unroll
      for (int u = 0; u < kDictPer; ++u) {
        const int j = pos[u] + step;
        if (j < nd && d[j] <= k[u]) pos[u] = j;
      }
    }
#pragma unroll
    for (int u = 0; u < kDictPer; ++u) {
      if (base + u * 256 + threadIdx.x >= n) continue;
      if (d[pos[u]] == k[u]) atomicAdd(&c[pos[u]], 1u);
      else missed = true;
    }
  }
  if (missed) miss[0] = 1;
  __syncthreads();
  for (int i = threadIdx.x; i < nd; i += 256)
    if (c[i]) atomicAdd(&counts[i], (unsigned long long)c[i]);
}

// second hash of every group's representative row (hashed tables built from data)
__global__ void group_keys2(const uint64_t* __restrict__ rep, int64_t G, const GroupCols* __restrict__ chunks,
                            uint64_t* __restrict__ keys2) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t r = rep[g];
    keys2[g] = tuple_hash(chunks[r >> kRowBits], (int64_t)(r & ((1ull << kRowBits) - 1)), kSeed2);
  }
}
__global__ void iota_u64(uint64_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (uint64_t)i;
}
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
__global__ void iota_u32(uint32_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (uint32_t)i;
}
__global__ void gather_top(const uint32_t* __restrict__ idx, int32_t n, const uint64_t* __restrict__ keys,
                           const int64_t* __restrict__ counts, const uint64_t* __restrict__ rep,
                           uint64_t* __restrict__ ok, int64_t* __restrict__ oc, uint64_t* __restrict__ orp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint32_t g = idx[i];
    ok[i] = keys[g];
    oc[i] = counts[g];
    orp[i] = rep ? rep[g] : ~0ull;
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

// MutualInformation from a self-contained two-column table: group g's per-column keys from the store (row g)
__global__ void store_col_keys(GroupCols st, int64_t G, uint64_t* __restrict__ xk, uint64_t* __restrict__ yk) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
    xk[g] = col_key(st, 0, g);
    yk[g] = col_key(st, 1, g);
  }
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
__device__ __forceinline__ bool is_str_type(int32_t t) { return t == DQ_TYPE_UTF8 || t == DQ_TYPE_LARGE_UTF8; }
// null-safe equality of column c: row r of a, row q of p.  NULL = NULL, NULL != any value, and the bytes under a NULL
// slot are never loaded; values by tuple_equal_rows' rule (the two sides of a string column may differ in offset width)
__device__ __forceinline__ bool match_equal(const MatchCols& a, const MatchCols& p, int c, int64_t r, int64_t q) {
  const bool va = !a.validity[c] || ((a.validity[c][r >> 5] >> (r & 31)) & 1u);
  const bool vp = !p.validity[c] || ((p.validity[c][q >> 5] >> (q & 31)) & 1u);
  if (!va || !vp) return va == vp;
  const int32_t ta = a.type[c], tp = p.type[c];
  if (is_str_type(ta)) {
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
}  // namespace
}  // namespace dq

// weighted_chunks (with sorted_rows): the counts are sums of weights, added up into *d_total (zeroed by the caller)
static dq_status rle_into(Frame& fr, dq_freq_table* t, const uint64_t* sorted, int64_t n,
                          const uint64_t* sorted_rows = nullptr, const GroupCols* weighted_chunks = nullptr,
                          unsigned long long* d_total = nullptr) {
  int64_t *nruns = nullptr, *starts = nullptr;
  void* tmp = nullptr;
  if (dq_status s = take(fr, nruns, 1)) return s;
  DQ_HIP(t->d_keys.alloc(std::max<int64_t>(1, n)));
  DQ_HIP(t->d_counts.alloc(std::max<int64_t>(1, n)));
  if (n == 0) { t->n_groups = 0; return DQ_OK; }
  if (dq_status s = take(fr, tmp, prim::runs_temp_bytes(n))) return s;
  if (dq_status s = take(fr, starts, n)) return s;
  DQ_HIP(prim::runs(sorted, n, t->d_keys.get(), starts, t->d_counts.get(), nruns, tmp, t->stream));
  if (dq_status s = read_back(&t->n_groups, nruns, t->stream)) return s;
  if (sorted_rows && t->n_groups > 0) {  // representative row of every group (Histogram renders its value)
    DQ_HIP(t->d_rep.alloc(t->n_groups));
    hipLaunchKernelGGL(gather_rep, dim3(grid_for(t->n_groups)), dim3(256), 0, t->stream, sorted_rows, starts,
                       t->n_groups, t->d_rep.get());
    DQ_HIP(hipGetLastError());
    if (weighted_chunks) {
      hipLaunchKernelGGL(weighted_counts, dim3(grid_for(t->n_groups)), dim3(256), 0, t->stream, sorted_rows, starts,
                         t->n_groups, weighted_chunks, t->d_counts.get(), d_total);
      DQ_HIP(hipGetLastError());
    }
    DQ_HIP(hipStreamSynchronize(t->stream));
  }
  return DQ_OK;
}

static dq_status collision_status(int32_t coll) {
  return coll ? set_error(DQ_E_UNSUPPORTED, "dq_freq_build: 64-bit tuple-hash collision between distinct values") : DQ_OK;
}

// the exact check of equal-hash neighbours in sorted order (verify_runs); d_flag: 8 bytes for the collision flag
static dq_status verify_sorted(dq_freq_table* t, const uint64_t* sorted_keys, const uint64_t* sorted_rows, int64_t nv,
                               const std::vector<GroupCols>& gcs, const GroupCols* d_chunks, int32_t* d_flag) {
  int32_t coll = 0;
  if (dq_status s = read_flag(d_flag, t->stream, &coll, [&] {
        with_bool(gcs.size() == 1, [&](auto one) {
          hipLaunchKernelGGL(verify_runs<decltype(one)::value>, dim3(grid_for(nv)), dim3(256), 0, t->stream, sorted_keys,
                             sorted_rows, nv, d_chunks, gcs[0], d_flag);
        });
      }))
    return s;
  return collision_status(coll);
}

// The dictionary form of a table (no sort): when an evenly spaced sample of the compacted keys holds at most
// 1 / 16 as many distinct keys (at most kDictMax), every key is counted against the sample's distinct keys in one
// pass; the groups are then those keys in ascending order -- what the sort and its runs yield -- with the smallest
// sampled row id of each as its representative.  A key outside the sample (a group the sample missed) sets
// *done = false and the caller sorts.  DQ_GROUP_DICT=0 turns it off, =1 lifts the size thresholds (tests).
static dq_status dict_table(Frame& fr, dq_freq_table* t, const uint64_t* keys, const uint64_t* rows, int64_t nv,
                            int end_bit, bool* done) {
  *done = false;
  const char* knob = std::getenv("DQ_GROUP_DICT");
  const bool forced = knob && knob[0] == '1';
  if (knob && knob[0] == '0') return DQ_OK;
  // only where the sort would run 5+ digit passes (tuple hashes, wide numeric keys) over 1 M+ keys: a table the
  // form declines pays ~0.15 ms (the sample's sort and read-back), measured against 4.0 ms for 1e8 27-bit keys
  if (!forced && (nv < (int64_t)1 << 20 || end_bit <= 32)) return DQ_OK;
  const hipStream_t S = t->stream;
  const int m = (int)std::min<int64_t>(kDictSample, nv);
  uint64_t *sk = nullptr, *sks = nullptr, *sr = nullptr, *dict = nullptr;
  int64_t* nr = nullptr;  // the number of distinct sample keys, then (second word) the miss flag
  void* tmp = nullptr;
  if (dq_status s = take_each(fr, m, sk, sks)) return s;
  if (dq_status s = take(fr, nr, 2)) return s;
  if (rows)
    if (dq_status s = take(fr, sr, m)) return s;
  const size_t tb = prim::sort_temp_bytes(m, 0);
  if (dq_status s = take(fr, tmp, tb)) return s;
  hipLaunchKernelGGL(dict_sample, dim3((m + 255) / 256), dim3(256), 0, S, keys, rows, nv, m, sk, sr);
  DQ_HIP(hipGetLastError());
  // keys only: a table the form does not take costs this sort of 16 K keys, one small kernel and one read-back
  DQ_HIP(prim::sort_pairs(sk, sks, nullptr, nullptr, 0, m, 0, end_bit, false, tmp, tb, S));
  if (dq_status s = take(fr, dict, m)) return s;
  hipLaunchKernelGGL(dict_unique, dim3(1), dim3(1024), 0, S, sks, m, dict, nr);
  DQ_HIP(hipGetLastError());
  int64_t nd = 0;
  if (dq_status s = read_back(&nd, nr, S)) return s;
  if (nd < 1 || nd > kDictMax || (!forced && nd * 16 > m)) return DQ_OK;
  int pw = 1;
  while (pw < nd) pw <<= 1;
  // the table's arrays stay local until every key is known to be in the dictionary
  DevPtr<uint64_t> d_keys, d_rep;
  DevPtr<int64_t> d_counts;
  int32_t* const d_miss = reinterpret_cast<int32_t*>(nr + 1);
  DQ_HIP(d_keys.alloc(nd));
  DQ_HIP(d_counts.alloc(nd));
  DQ_HIP(hipMemcpyAsync(d_keys.get(), dict, (size_t)nd * 8, hipMemcpyDeviceToDevice, S));
  DQ_HIP(hipMemsetAsync(d_counts.get(), 0, (size_t)nd * 8, S));
  DQ_HIP(hipMemsetAsync(d_miss, 0, 4, S));
  if (rows) {
    DQ_HIP(d_rep.alloc(nd));
    DQ_HIP(hipMemsetAsync(d_rep.get(), 0xFF, (size_t)nd * 8, S));
    hipLaunchKernelGGL(dict_rep, dim3((m + 255) / 256), dim3(256), 0, S, sk, sr, m, d_keys.get(), (int)nd,
                       d_rep.as<unsigned long long>());
    DQ_HIP(hipGetLastError());
  }
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (nv + 256 * kDictPer - 1) / (256 * kDictPer)));
  hipLaunchKernelGGL(dict_count, dim3(grid), dim3(256), 0, S, keys, nv, d_keys.get(), (int)nd, pw,
                     d_counts.as<unsigned long long>(), d_miss);
  DQ_HIP(hipGetLastError());
  int32_t miss = 0;
  if (dq_status s = read_back(&miss, d_miss, S)) return s;
  if (miss) return DQ_OK;  // a group outside the sample: back to the sort
  t->d_keys = std::move(d_keys);
  t->d_counts = std::move(d_counts);
  t->d_rep = std::move(d_rep);
  t->n_groups = nd;
  *done = true;
  return DQ_OK;
}

static int64_t wave_copy_len() {  // DQ_FREQ_WAVE_COPY: the lane / wave switch length of the string gather (sweeps)
  const char* e = std::getenv("DQ_FREQ_WAVE_COPY");  // (read per call: tools/freq_state_bench.py sweeps it)
  const long long v = e ? std::atoll(e) : 0;
  return v > 0 ? v : kWaveCopyLen;
}

// the chunk descriptor of one chunk's row of views (n_cols of them); a gather of non-null rows carries no validity
static GroupCols view_cols(const int32_t* types, int n_cols, const dq_column_view* row, uint64_t key_mask,
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

// Column c (type code `type`) of the tuples at row ids d_rep[0 .. G) of the chunks d_chunks, gathered into *out
// (allocated here, owned by the caller's StoreCol).  The caller has checked the row ids; scan_tmp is its frame's
// buffer of prim::scan_temp_bytes(G + 1) bytes (one for all the columns it gathers).
static dq_status gather_column(hipStream_t S, const GroupCols* d_chunks, const uint64_t* d_rep, int64_t G, int c,
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

extern "C" {

struct MiRequest { double total; double* value; int32_t* defined; };
static dq_status mi_from_joint(Frame& fr, dq_freq_table* t, const uint64_t* sorted_keys, const uint64_t* sorted_rows,
                               int64_t nv, const GroupCols* d_chunks, const MiRequest& mi);

static dq_status freq_build_impl(const int32_t* types, int32_t n_cols, const dq_column_view* cols,
                                 const int64_t* chunk_rows, int32_t n_chunks, int32_t device, void* hip_stream,
                                 dq_freq_table** out, const MiRequest* mi, const int64_t* const* weights = nullptr,
                                 const uint64_t* const* selection = nullptr) {
  if (!out) return set_error(DQ_E_INVALID, "dq_freq_build: out is NULL");
  *out = nullptr;
  if (n_cols < 1 || n_cols > kMaxGroupCols || !types)
    return set_error(DQ_E_INVALID, "dq_freq_build: 1..%d grouping columns", kMaxGroupCols);
  if (n_chunks < 0 || n_chunks > kMaxGroupChunks || (n_chunks > 0 && (!cols || !chunk_rows)))
    return set_error(DQ_E_INVALID, "dq_freq_build: bad chunks (at most %d)", kMaxGroupChunks);
  for (int k = 0; weights && k < n_chunks; ++k)
    if (chunk_rows[k] > 0 && (!weights[k] || ((uintptr_t)weights[k] & 7)))
      return set_error(DQ_E_INVALID, "dq_freq_build_weighted: chunk %d has no (or misaligned) weights", k);
  for (int k = 0; selection && k < n_chunks; ++k)
    if ((uintptr_t)selection[k] & 7)
      return set_error(DQ_E_INVALID, "dq_freq_build_where: chunk %d's selection is not 8-byte aligned", k);
  for (int c = 0; c < n_cols; ++c) {
    if (!type_valid(types[c]))
      return set_error(DQ_E_TYPE, "dq_freq_build: column %d has unknown type %d", c, types[c]);
  }
  int64_t total = 0;
  for (int k = 0; k < n_chunks; ++k) {
    if (chunk_rows[k] < 0 || chunk_rows[k] >= (1ll << kRowBits)) return set_error(DQ_E_INVALID, "chunk rows");
    total += chunk_rows[k];
  }
  if (total >= (1ll << 31)) return set_error(DQ_E_UNSUPPORTED, "dq_freq_build: at most 2^31 - 1 rows per table");
  DQ_HIP(hipSetDevice(device));
  auto* t = new dq_freq_table();
  std::unique_ptr<dq_freq_table> guard(t);
  t->device = device;
  t->stream = reinterpret_cast<hipStream_t>(hip_stream);
  t->types.assign(types, types + n_cols);
  // one fixed-width column: grouped by its exact value bits (strings and tuples: by hash, checked exactly)
  const bool numeric1 = n_cols == 1 && types[0] != DQ_TYPE_UTF8 && types[0] != DQ_TYPE_LARGE_UTF8 && !is_decimal(types[0]);
  t->hashed = numeric1 && !mi ? 0 : 1;
  if (weights && !t->hashed)
    return set_error(DQ_E_UNSUPPORTED, "dq_freq_build_weighted: a single fixed-width column is its own key");

  // test hook: keep only some bits of the primary tuple hash, to force collisions between distinct tuples
  const uint64_t key_mask = test_hash_mask();
  std::vector<GroupCols> gcs(std::max(1, n_chunks));
  for (int k = 0; k < n_chunks; ++k) {
    gcs[k] = view_cols(types, n_cols, cols + (size_t)k * n_cols, key_mask, true);
    if (weights) gcs[k].weight = weights[k];
  }
  Frame fr(g_arena, device);
  const hipStream_t S = t->stream;
  uint64_t *sel_keys = nullptr, *sel_rows = nullptr, *sorted_keys = nullptr, *sorted_rows = nullptr;
  unsigned long long* nsel = nullptr;  // count, AND, OR of the appended keys; later the checks' collision flag
  GroupCols* d_chunks = nullptr;
  void* tmp = nullptr;
  if (dq_status s = take(fr, nsel, 3)) return s;
  int32_t* const d_flag = reinterpret_cast<int32_t*>(nsel);
  if (dq_status s = take(fr, sel_keys, std::max<int64_t>(1, total))) return s;
  if (t->hashed)
    if (dq_status s = take(fr, sel_rows, std::max<int64_t>(1, total))) return s;
  const unsigned long long cur0[3] = {0ull, ~0ull, 0ull};
  DQ_HIP(hipMemcpyAsync(nsel, cur0, sizeof(cur0), hipMemcpyHostToDevice, S));
  for (int k = 0; k < n_chunks; ++k) {
    const int64_t n = chunk_rows[k];
    if (n == 0) continue;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + kCompactRows - 1) / kCompactRows));
    // (a chunk without a selection runs the unfiltered instantiation)
    const uint32_t* const sel = selection ? reinterpret_cast<const uint32_t*>(selection[k]) : nullptr;
    with_bool(t->hashed != 0, [&](auto hashed) {  // (sel_rows is NULL for an exact-key table)
      with_bool(sel != nullptr, [&](auto filtered) {
        hipLaunchKernelGGL((group_compact<decltype(hashed)::value, decltype(filtered)::value>), dim3(grid), dim3(256), 0, S,
                           gcs[k], n, (int64_t)k, sel_keys, sel_rows, nsel, sel);
      });
    });
    DQ_HIP(hipGetLastError());
  }
  unsigned long long cur[3];
  if (dq_status s = read_back(&cur, nsel, S)) return s;
  const int64_t nv = (int64_t)cur[0];
  // the keys agree above their highest differing bit: sorting bits [0, end_bit) gives the same order as all 64
  // (small-range integer columns: 2 digit passes instead of 6)
  const uint64_t differ = nv > 0 ? (uint64_t)(cur[1] ^ cur[2]) : 0ull;
  const int end_bit = differ ? 64 - __builtin_clzll(differ) : 1;
  t->n_values = nv;
  if (t->hashed) {
    if (dq_status s = take(fr, d_chunks, gcs.size())) return s;
    DQ_HIP(hipMemcpyAsync(d_chunks, gcs.data(), gcs.size() * sizeof(GroupCols), hipMemcpyHostToDevice, S));
  }
  static const char* force = std::getenv("DQ_GROUP_VERIFY");  // A/B knob: "sorted" / "compacted"
  bool dict = false;  // low cardinality: the dictionary form (no sort; the check in compaction order)
  if (!mi && !weights && nv > 0 && !(force && force[0] == 's'))  // (its counts are numbers of rows)
    if (dq_status s = dict_table(fr, t, sel_keys, sel_rows, nv, end_bit, &dict)) return s;
  if (dq_status s = take(fr, sorted_keys, std::max<int64_t>(1, nv))) return s;
  if (nv > 0 && !dict) {
    if (t->hashed) {
      if (dq_status s = take(fr, sorted_rows, nv)) return s;
      const size_t tb = prim::sort_temp_bytes(nv, 8);
      if (dq_status s = take(fr, tmp, tb)) return s;
      DQ_HIP(prim::sort_pairs(sel_keys, sorted_keys, sel_rows, sorted_rows, 8, nv, 0, end_bit, false, tmp, tb, S));
      // exact check of equal-hash neighbours in sorted order here for MutualInformation; the frequency table's runs
      // choose between the two forms below
      if (mi)
        if (dq_status s = verify_sorted(t, sorted_keys, sorted_rows, nv, gcs, d_chunks, d_flag)) return s;
    } else {
      const size_t tb = prim::sort_temp_bytes(nv, 0);
      if (dq_status s = take(fr, tmp, tb)) return s;
      DQ_HIP(prim::sort_pairs(sel_keys, sorted_keys, nullptr, nullptr, 0, nv, 0, end_bit, false, tmp, tb, S));
    }
  }
  if (mi) return mi_from_joint(fr, t, sorted_keys, sorted_rows, nv, d_chunks, *mi);
  if (weights && nv > 0) {  // groups' counts and num_values: sums of weights
    unsigned long long* d_total = nullptr;
    if (dq_status s = take(fr, d_total, 1)) return s;
    DQ_HIP(hipMemsetAsync(d_total, 0, 8, S));
    if (dq_status s = rle_into(fr, t, sorted_keys, nv, sorted_rows, d_chunks, d_total)) return s;
    if (dq_status s = read_back(&t->n_values, d_total, S)) return s;
  } else if (!dict) {
    if (dq_status s = rle_into(fr, t, sorted_keys, nv, t->hashed ? sorted_rows : nullptr)) return s;
  }
  if (t->hashed && nv > 0) {
    // few groups (rows repeat their group's tuple many times): each row checked against its group's representative
    // in compaction order; otherwise equal-hash neighbours in sorted order (which the dictionary form has not made)
    const bool compacted = dict || (force ? force[0] == 'c'
                                          : t->n_groups <= kCompactedMaxGroups && t->n_groups * kRowOrderVerify <= nv);
    if (compacted) {
      int32_t coll = 0;
      if (dq_status s = read_flag(d_flag, S, &coll, [&] {
            with_bool(gcs.size() == 1, [&](auto one) {
              hipLaunchKernelGGL(verify_compacted<decltype(one)::value>, dim3(grid_for(nv)), dim3(256), 0, S, sel_keys,
                                 sel_rows, nv, t->d_keys.get(), t->n_groups, t->d_rep.get(), d_chunks, gcs[0], d_flag);
            });
          }))
        return s;
      if (dq_status s = collision_status(coll)) return s;
    } else if (dq_status s = verify_sorted(t, sorted_keys, sorted_rows, nv, gcs, d_chunks, d_flag)) {
      return s;
    }
  }
  if (t->hashed) {
    DQ_HIP(t->d_keys2.alloc(std::max<int64_t>(1, t->n_groups)));
    if (t->n_groups > 0) {
      hipLaunchKernelGGL(group_keys2, dim3(grid_for(t->n_groups)), dim3(256), 0, S, t->d_rep.get(), t->n_groups, d_chunks,
                         t->d_keys2.get());
      DQ_HIP(hipGetLastError());
      DQ_HIP(hipStreamSynchronize(S));
    }
  }
  *out = guard.release();
  return DQ_OK;
}

// the temporary of the MutualInformation stages over n keys (runs, sorts and scans share it)
static size_t mi_temp_bytes(int64_t n) {
  return std::max({prim::runs_temp_bytes(n), prim::sort_temp_bytes(n, 8), prim::scan_temp_bytes(n)});
}

// the marginals and the sum over G joint groups (counts gc; group g's representative row id rep[g], per-column keys
// xk / yk, idx[g] = g): shared by the one-pass path (rows of the input) and the state path (rows of the store);
// tmp: the caller's buffer of at least mi_temp_bytes(G) bytes
static dq_status mi_from_groups(Frame& fr, hipStream_t S, int64_t G, const int64_t* gc, const uint64_t* rep,
                                const uint64_t* xk, const uint64_t* yk, const uint64_t* idx, const GroupCols* d_chunks,
                                void* tmp, const MiRequest& mi) {
  uint64_t *sk = nullptr, *sidx = nullptr;
  unsigned long long* segsum = nullptr;
  int64_t *px = nullptr, *py = nullptr;
  uint32_t *head = nullptr, *seg = nullptr;
  double *res = nullptr, *part = nullptr;
  int32_t* coll = nullptr;
  if (dq_status s = take_each(fr, G, sk, sidx, segsum, px, py, head, seg)) return s;
  if (dq_status s = take(fr, res, 1)) return s;
  if (dq_status s = take(fr, coll, 2)) return s;
  if (dq_status s = take(fr, part, kSumBlocks)) return s;
  const size_t tb = mi_temp_bytes(G);
  DQ_HIP(hipMemsetAsync(coll, 0, 8, S));
  for (int c = 0; c < 2; ++c) {
    DQ_HIP(prim::sort_pairs(c == 0 ? xk : yk, sk, idx, sidx, 8, G, 0, 64, false, tmp, tb, S));
    hipLaunchKernelGGL(mi_heads, dim3(grid_for(G)), dim3(256), 0, S, sk, sidx, rep, G, d_chunks, c, head, coll);
    DQ_HIP(hipGetLastError());
    DQ_HIP(prim::inclusive_sum_u32(head, seg, G, tmp, S));
    DQ_HIP(hipMemsetAsync(segsum, 0, G * 8, S));
    hipLaunchKernelGGL(mi_segsum, dim3(grid_for(G)), dim3(256), 0, S, sidx, seg, gc, G, segsum);
    DQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(mi_scatter, dim3(grid_for(G)), dim3(256), 0, S, sidx, seg, segsum, G, c == 0 ? px : py);
    DQ_HIP(hipGetLastError());
  }
  const int nb = (int)std::min<int64_t>(kSumBlocks, (G + 255) / 256);
  hipLaunchKernelGGL(mi_part, dim3(nb), dim3(256), 0, S, gc, px, py, G, mi.total, part);
  DQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(mi_final, dim3(1), dim3(64), 0, S, part, nb, res);
  DQ_HIP(hipGetLastError());
  int32_t collided = 0;
  DQ_HIP(hipMemcpyAsync(&collided, coll, 4, hipMemcpyDeviceToHost, S));
  if (dq_status s = read_back(mi.value, res, S)) return s;
  if (collided) return set_error(DQ_E_UNSUPPORTED, "dq_mutual_information: 64-bit key collision between distinct values");
  *mi.defined = 1;
  return DQ_OK;
}

static dq_status mi_from_joint(Frame& fr, dq_freq_table* t, const uint64_t* sorted_keys, const uint64_t* sorted_rows,
                               int64_t nv, const GroupCols* d_chunks, const MiRequest& mi) {
  *mi.defined = 0;
  *mi.value = 0.0;
  if (nv == 0) return DQ_OK;  // sum over an empty join is NULL -> metricFromEmpty
  const hipStream_t S = t->stream;
  uint64_t *gk = nullptr, *rep = nullptr, *xk = nullptr, *yk = nullptr, *idx = nullptr;
  int64_t *gc = nullptr, *starts = nullptr, *nruns = nullptr;
  void* tmp = nullptr;  // for the runs here and, over G <= nv groups, the marginals' sorts and scans
  if (dq_status s = take_each(fr, nv, gk, gc, starts, rep, xk, yk, idx)) return s;
  if (dq_status s = take(fr, nruns, 1)) return s;
  if (dq_status s = take(fr, tmp, mi_temp_bytes(nv))) return s;
  // joint groups: keys, counts and first positions of the runs of the sorted joint keys
  DQ_HIP(prim::runs(sorted_keys, nv, gk, starts, gc, nruns, tmp, S));
  int64_t G = 0;
  if (dq_status s = read_back(&G, nruns, S)) return s;
  hipLaunchKernelGGL(mi_group_keys, dim3(grid_for(G)), dim3(256), 0, S, sorted_rows, starts, G, d_chunks, rep, xk, yk, idx);
  DQ_HIP(hipGetLastError());
  return mi_from_groups(fr, S, G, gc, rep, xk, yk, idx, d_chunks, tmp, mi);
}

dq_status dq_freq_build(const int32_t* types, int32_t n_cols, const dq_column_view* cols, const int64_t* chunk_rows,
                        int32_t n_chunks, int32_t device, void* hip_stream, dq_freq_table** out) {
  return freq_build_impl(types, n_cols, cols, chunk_rows, n_chunks, device, hip_stream, out, nullptr);
}

dq_status dq_freq_build_where(const int32_t* types, int32_t n_cols, const dq_column_view* cols, const int64_t* chunk_rows,
                              const uint64_t* const* selection, int32_t n_chunks, int32_t device, void* hip_stream,
                              dq_freq_table** out) {
  return freq_build_impl(types, n_cols, cols, chunk_rows, n_chunks, device, hip_stream, out, nullptr, nullptr, selection);
}

dq_status dq_freq_build_weighted(const int32_t* types, int32_t n_cols, const dq_column_view* cols,
                                 const int64_t* chunk_rows, const int64_t* const* weights, int32_t n_chunks,
                                 int32_t device, void* hip_stream, dq_freq_table** out) {
  if (n_chunks > 0 && !weights) return set_error(DQ_E_INVALID, "dq_freq_build_weighted: weights is NULL");
  return freq_build_impl(types, n_cols, cols, chunk_rows, n_chunks, device, hip_stream, out, nullptr, weights);
}

dq_status dq_mutual_information(const int32_t* types, const dq_column_view* cols, const int64_t* chunk_rows,
                                int32_t n_chunks, int64_t num_rows, int32_t device, void* hip_stream, double* value,
                                int32_t* defined) {
  if (!value || !defined) return set_error(DQ_E_INVALID, "dq_mutual_information: NULL output");
  MiRequest mi{(double)num_rows, value, defined};
  dq_freq_table* unused = nullptr;
  dq_status s = freq_build_impl(types, 2, cols, chunk_rows, n_chunks, device, hip_stream, &unused, &mi);
  if (unused) dq_freq_destroy(unused);
  return s;
}

dq_status dq_mutual_information_where(const int32_t* types, const dq_column_view* cols, const int64_t* chunk_rows,
                                      const uint64_t* const* selection, int32_t n_chunks, int64_t num_rows,
                                      int32_t device, void* hip_stream, double* value, int32_t* defined) {
  if (!value || !defined) return set_error(DQ_E_INVALID, "dq_mutual_information_where: NULL output");
  MiRequest mi{(double)num_rows, value, defined};
  dq_freq_table* unused = nullptr;
  dq_status s = freq_build_impl(types, 2, cols, chunk_rows, n_chunks, device, hip_stream, &unused, &mi, nullptr, selection);
  if (unused) dq_freq_destroy(unused);
  return s;
}

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
  Frame fr(g_arena, a->device);
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
    hipLaunchKernelGGL(iota_u64, dim3(grid_for(n)), dim3(256), 0, S, pos, n);
    DQ_HIP(hipGetLastError());
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

dq_status dq_freq_summarize(const dq_freq_table* t, int64_t num_rows, dq_freq_summary* out) {
  if (!t || !out) return set_error(DQ_E_INVALID, "dq_freq_summarize: NULL argument");
  DQ_HIP(hipSetDevice(t->device));
  std::memset(out, 0, sizeof(*out));
  out->num_groups = t->n_groups;
  out->num_values = t->n_values;
  if (t->n_groups == 0) return DQ_OK;
  Frame fr(g_arena, t->device);
  SumPart *part = nullptr, *res = nullptr;
  if (dq_status s = take(fr, part, kSumBlocks)) return s;
  if (dq_status s = take(fr, res, 1)) return s;
  const int nb = (int)std::min<int64_t>(kSumBlocks, (t->n_groups + 255) / 256);
  hipLaunchKernelGGL(summary_part, dim3(nb), dim3(256), 0, t->stream, t->d_counts.get(), t->n_groups, (double)num_rows,
                     part);
  DQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(summary_final, dim3(1), dim3(64), 0, t->stream, part, nb, res);
  DQ_HIP(hipGetLastError());
  SumPart h{};
  if (dq_status s = read_back(&h, res, t->stream)) return s;
  out->num_unique = h.unique;
  out->entropy = h.ent;
  return DQ_OK;
}

int64_t dq_freq_num_groups(const dq_freq_table* t) { return t ? t->n_groups : -1; }

dq_status dq_freq_export(const dq_freq_table* t, uint64_t* keys, int64_t* counts, int64_t cap) {
  if (!t || cap < t->n_groups || (t->n_groups > 0 && (!keys || !counts)))
    return set_error(DQ_E_INVALID, "dq_freq_export: bad arguments");
  DQ_HIP(hipSetDevice(t->device));
  if (t->n_groups > 0) {
    DQ_HIP(hipMemcpyAsync(keys, t->d_keys.get(), t->n_groups * 8, hipMemcpyDeviceToHost, t->stream));
    DQ_HIP(hipMemcpyAsync(counts, t->d_counts.get(), t->n_groups * 8, hipMemcpyDeviceToHost, t->stream));
  }
  DQ_HIP(hipStreamSynchronize(t->stream));
  return DQ_OK;
}

void dq_freq_destroy(dq_freq_table* t) { delete t; }

dq_status dq_freq_top(const dq_freq_table* t, int32_t n, uint64_t* keys, int64_t* counts, uint64_t* rep_rows,
                      int32_t* n_out) {
  if (!t || n < 0 || !n_out || (n > 0 && (!keys || !counts || !rep_rows)))
    return set_error(DQ_E_INVALID, "dq_freq_top: bad arguments");
  const int32_t m = (int32_t)std::min<int64_t>(n, t->n_groups);
  *n_out = m;
  if (m == 0) return DQ_OK;
  DQ_HIP(hipSetDevice(t->device));
  Frame fr(g_arena, t->device);
  const hipStream_t S = t->stream;
  const int64_t G = t->n_groups;
  uint32_t *idx = nullptr, *sidx = nullptr;
  uint64_t *sc = nullptr, *ok = nullptr, *orp = nullptr;
  int64_t* oc = nullptr;
  void* tmp = nullptr;
  if (dq_status s = take_each(fr, G, idx, sidx, sc)) return s;
  if (dq_status s = take_each(fr, m, ok, oc, orp)) return s;
  hipLaunchKernelGGL(iota_u32, dim3(grid_for(G)), dim3(256), 0, S, idx, G);
  DQ_HIP(hipGetLastError());
  // counts descending, ties in key order (stable radix sort over groups already in key order); every count is in
  // [1, n_values], so the bits above n_values' highest set bit are zero in all of them
  const int end_bit = t->n_values > 0 ? 64 - __builtin_clzll((unsigned long long)t->n_values) : 1;
  const size_t tb = prim::sort_temp_bytes(G, 4);
  if (dq_status s = take(fr, tmp, tb)) return s;
  DQ_HIP(prim::sort_pairs(t->d_counts.as<const uint64_t>(), sc, idx, sidx, 4, G, 0, end_bit, true, tmp, tb, S));
  hipLaunchKernelGGL(gather_top, dim3((m + 255) / 256), dim3(256), 0, S, sidx, m, t->d_keys.get(), t->d_counts.get(),
                     t->d_rep.get(), ok, oc, orp);
  DQ_HIP(hipGetLastError());
  DQ_HIP(hipMemcpyAsync(keys, ok, (size_t)m * 8, hipMemcpyDeviceToHost, S));
  DQ_HIP(hipMemcpyAsync(counts, oc, (size_t)m * 8, hipMemcpyDeviceToHost, S));
  DQ_HIP(hipMemcpyAsync(rep_rows, orp, (size_t)m * 8, hipMemcpyDeviceToHost, S));
  DQ_HIP(hipStreamSynchronize(S));
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
  Frame fr(g_arena, t->device);
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

// the sections of t's image (offsets as FreqImageView), its total length returned
static int64_t image_layout(const dq_freq_table* t, FreqImageView* v) {
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

dq_status dq_freq_mutual_information(const dq_freq_table* t, int64_t num_rows, double* value, int32_t* defined) {
  if (!t || !value || !defined) return set_error(DQ_E_INVALID, "dq_freq_mutual_information: NULL argument");
  if (t->types.size() != 2) return set_error(DQ_E_STATE, "dq_freq_mutual_information: a table over %zu columns, not 2", t->types.size());
  if (!t->has_store)
    return set_error(DQ_E_STATE, "dq_freq_mutual_information: the table does not own its values (dq_freq_materialize it first)");
  *defined = 0;
  *value = 0.0;
  const int64_t G = t->n_groups;
  if (G == 0) return DQ_OK;  // sum over an empty join is NULL -> metricFromEmpty
  DQ_HIP(hipSetDevice(t->device));
  Frame fr(g_arena, t->device);
  const hipStream_t S = t->stream;
  uint64_t *rep = nullptr, *xk = nullptr, *yk = nullptr;
  GroupCols* d_store = nullptr;
  void* tmp = nullptr;
  if (dq_status s = take_each(fr, G, rep, xk, yk)) return s;
  if (dq_status s = take(fr, d_store, 1)) return s;
  if (dq_status s = take(fr, tmp, mi_temp_bytes(G))) return s;
  const GroupCols st = store_cols(t);
  DQ_HIP(hipMemcpyAsync(d_store, &st, sizeof(st), hipMemcpyHostToDevice, S));
  DQ_HIP(hipStreamSynchronize(S));
  // group g is row g of the store: its row id and its index are both g
  hipLaunchKernelGGL(iota_u64, dim3(grid_for(G)), dim3(256), 0, S, rep, G);
  DQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(store_col_keys, dim3(grid_for(G)), dim3(256), 0, S, st, G, xk, yk);
  DQ_HIP(hipGetLastError());
  const MiRequest mi{(double)num_rows, value, defined};
  return mi_from_groups(fr, S, G, t->d_counts.get(), rep, xk, yk, rep, d_store, tmp, mi);
}

dq_status dq_freq_take_values(const dq_freq_table* t, const uint64_t* keys, int32_t n, int32_t col, void* values,
                              int64_t values_cap, int64_t* offsets, int64_t* values_bytes) {
  if (!t || n < 0 || !values_bytes || (n > 0 && !keys) || col < 0 || col >= (int)t->types.size())
    return set_error(DQ_E_INVALID, "dq_freq_take_values: bad arguments");
  if (!t->has_store) return set_error(DQ_E_STATE, "dq_freq_take_values: the table does not own its values");
  const int es = dq_freq_elem_size(t->types[col]);
  if (es == 0 && !offsets) return set_error(DQ_E_INVALID, "dq_freq_take_values: a string column needs offsets[n + 1]");
  DQ_HIP(hipSetDevice(t->device));
  Frame fr(g_arena, t->device);
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

static dq_status unique_rows_impl(const dq_freq_table* t, const int32_t* types, const dq_column_view* cols,
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
  auto is_str = [](int32_t ty) { return ty == DQ_TYPE_UTF8 || ty == DQ_TYPE_LARGE_UTF8; };
  std::vector<int32_t> ty(t->types);
  for (int c = 0; c < n_cols; ++c) {
    if (types) ty[c] = types[c];
    // the probe hashes what the build hashed: the same type, or a string column of the other offset width
    if (ty[c] != t->types[c] && !(is_str(ty[c]) && is_str(t->types[c])))
      return set_error(DQ_E_INVALID, "dq_freq_unique_rows: column %d has type %d, the table's has %d", c, ty[c], t->types[c]);
    const dq_column_view& v = cols[c];
    if (!v.values || ((uintptr_t)v.values & 3) || ((uintptr_t)v.validity & 3) || (is_str(ty[c]) && !v.offsets))
      return set_error(DQ_E_INVALID, "dq_freq_unique_rows: column %d: missing or misaligned buffer", c);
  }
  DQ_HIP(hipSetDevice(t->device));
  const hipStream_t S = reinterpret_cast<hipStream_t>(hip_stream);
  const GroupCols g = view_cols(ty.data(), n_cols, cols, test_hash_mask(), true);
  Frame fr(g_arena, t->device);
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
  DQ_HIP(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, S));
  DQ_HIP(hipStreamSynchronize(S));
  if (h[2]) return set_error(DQ_E_INVALID, "dq_freq_unique_rows: a row whose key is no group of the table (built from other data)");
  if (num_unique) *num_unique = (int64_t)h[0];
  if (num_grouped) *num_grouped = (int64_t)h[1];
  return DQ_OK;
}

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

// dq_freq_contains_rows (group NULL: the bitmaps) and dq_freq_lookup_rows (group: the index of every row's group, no
// bitmap) are one search: the same checks in the same order, the same splitters, the same kernel
static dq_status contains_impl(const char* me, const dq_freq_table* t, const int32_t* types, const dq_column_view* cols,
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
  auto is_str = [](int32_t ty) { return ty == DQ_TYPE_UTF8 || ty == DQ_TYPE_LARGE_UTF8; };
  std::vector<int32_t> ty(t->types);
  for (int c = 0; c < n_cols; ++c) {
    if (types) ty[c] = types[c];
    // the same type (a decimal's precision and scale are part of its code), or a string column of the other offset
    // width; nothing is widened
    if (ty[c] != t->types[c] && !(is_str(ty[c]) && is_str(t->types[c])))
      return set_error(DQ_E_INVALID, "%s: column %d has type %d, the table's has %d", me, c, ty[c], t->types[c]);
    const dq_column_view& v = cols[c];
    if (!v.values || ((uintptr_t)v.values & 3) || ((uintptr_t)v.validity & 3) || (is_str(ty[c]) && !v.offsets))
      return set_error(DQ_E_INVALID, "%s: column %d: missing or misaligned buffer", me, c);
  }
  DQ_HIP(hipSetDevice(t->device));
  const hipStream_t S = reinterpret_cast<hipStream_t>(hip_stream);
  const GroupCols g = view_cols(ty.data(), n_cols, cols, test_hash_mask(), true);
  GroupCols st;
  std::memset(&st, 0, sizeof(st));
  if (t->hashed) st = store_cols(t);
  Frame fr(g_arena, t->device);
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
  DQ_HIP(hipMemcpyAsync(h, d_tot, sizeof(h), hipMemcpyDeviceToHost, S));
  DQ_HIP(hipStreamSynchronize(S));
  if (num_contained) *num_contained = (int64_t)h[0];
  if (num_applies) *num_applies = (int64_t)h[1];
  return DQ_OK;
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
  auto is_str = [](int32_t ty) { return ty == DQ_TYPE_UTF8 || ty == DQ_TYPE_LARGE_UTF8; };
  auto known = [](int32_t ty) {
    const int32_t b = DQ_TYPE_BASE(ty);
    return b >= DQ_TYPE_F64 && b <= DQ_TYPE_DECIMAL128 && (b == DQ_TYPE_DECIMAL128 || ty == b);
  };
  for (int c = 0; c < n_cols; ++c) {
    // the same type (a decimal's precision and scale are part of its code), or two string columns; nothing is widened
    if (!known(types[c]) || !known(payload_types[c]) ||
        (types[c] != payload_types[c] && !(is_str(types[c]) && is_str(payload_types[c]))))
      return set_error(DQ_E_INVALID, "%s: column %d has type %d, the payload's has %d", me, c, types[c], payload_types[c]);
  }
  MatchCols a, p;
  std::memset(&a, 0, sizeof(a));
  std::memset(&p, 0, sizeof(p));
  for (int c = 0; n_rows > 0 && c < n_cols; ++c) {
    const dq_column_view &v = cols[c], &u = payload[c];
    if (!v.values || ((uintptr_t)v.values & 3) || ((uintptr_t)v.validity & 3) || (is_str(types[c]) && !v.offsets))
      return set_error(DQ_E_INVALID, "%s: column %d: missing or misaligned buffer", me, c);
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
  Frame fr(g_arena, device);
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
  DQ_HIP(hipMemcpyAsync(h, d_tot, sizeof(h), hipMemcpyDeviceToHost, S));
  DQ_HIP(hipStreamSynchronize(S));
  if (num_matched) *num_matched = (int64_t)h[0];
  if (num_found) *num_found = (int64_t)h[1];
  if (num_applies) *num_applies = (int64_t)h[2];
  for (int c = 0; num_mismatch && c < n_cols; ++c) num_mismatch[c] = (int64_t)h[3 + c];
  return DQ_OK;
}

}  // extern "C"
