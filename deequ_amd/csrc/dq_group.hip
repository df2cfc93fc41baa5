// dq_group.hip -- building a frequency table from data for the grouping analyzers (sort-based group-by count), with
// what reads one for them: MutualInformation, the summary, the top-N and the export.  The table as a persisted state
// (merge, value store, image) is dq_freq_store.hip, the probes of other rows against a table are dq_probe.hip, and
// what they share with this file -- the table, the row's validity, hash and key -- is dq_freq_table.h.
//
// Reference: FrequencyBasedAnalyzer.computeFrequencies (analyzers/GroupingAnalyzers.scala:44-82):
//   SELECT cols, COUNT(*) FROM data WHERE col_1 IS NOT NULL AND ... GROUP BY cols
// plus numRows = data.count(), and the metrics of Uniqueness / Distinctness / CountDistinct /
// Entropy / UniqueValueRatio, which only need the multiset of group counts (Uniqueness.scala:27-29,
// Distinctness.scala:29-31, CountDistinct.scala:25-31, Entropy.scala:29-41, UniqueValueRatio.scala:25-36).
//
// Layout: every row whose grouping columns are all non-null yields one 64-bit key.  A single 8-byte /
// 4-byte numeric column is its own exact key (f64: NaN canonicalised as Spark's UnsafeRow.setDouble
// does; -0.0 and 0.0 stay distinct groups in Spark 2.2).  Otherwise (strings, several columns) the key
// is a 64-bit hash of the tuple, the rows ride along the sort, and every pair of neighbours with equal
// keys is compared exactly: a collision between distinct tuples is reported (DQ_E_UNSUPPORTED), never
// merged silently.  Keys are radix-sorted and run-length encoded into (key, count) groups by dq_prim.hip's
// hand-written kernels; the summary is a fixed-order two-level reduction, so results are deterministic.  A hashed table also
// keeps a second, independently seeded 64-bit hash per group (its representative row's tuple), for dq_freq_merge,
// which no longer has the rows (dq_freq_store.hip).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <memory>
#include <vector>

#include "dq_device.h"
#include "dq_freq_table.h"
#include "dq_prim.h"

namespace dq {
namespace {

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

// MutualInformation from a self-contained two-column table: group g's per-column keys from the store (row g)
__global__ void store_col_keys(GroupCols st, int64_t G, uint64_t* __restrict__ xk, uint64_t* __restrict__ yk) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
    xk[g] = col_key(st, 0, g);
    yk[g] = col_key(st, 1, g);
  }
}

Arena<DeviceMem> g_arena;  // the scratch of every grouping call (dq_arena.h; Frame, take, read_back: dq_freq_table.h)

// weighted_chunks (with sorted_rows): the counts are sums of weights, added up into *d_total (zeroed by the caller)
dq_status rle_into(Frame& fr, dq_freq_table* t, const uint64_t* sorted, int64_t n,
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

dq_status collision_status(int32_t coll) {
  return coll ? set_error(DQ_E_UNSUPPORTED, "dq_freq_build: 64-bit tuple-hash collision between distinct values") : DQ_OK;
}

// the exact check of equal-hash neighbours in sorted order (verify_runs); d_flag: 8 bytes for the collision flag
dq_status verify_sorted(dq_freq_table* t, const uint64_t* sorted_keys, const uint64_t* sorted_rows, int64_t nv,
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
dq_status dict_table(Frame& fr, dq_freq_table* t, const uint64_t* keys, const uint64_t* rows, int64_t nv,
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

struct MiRequest { double total; double* value; int32_t* defined; };

// the temporary of the MutualInformation stages over n keys (runs, sorts and scans share it)
size_t mi_temp_bytes(int64_t n) {
  return std::max({prim::runs_temp_bytes(n), prim::sort_temp_bytes(n, 8), prim::scan_temp_bytes(n)});
}

// the marginals and the sum over G joint groups (counts gc; group g's representative row id rep[g], per-column keys
// xk / yk, idx[g] = g): shared by the one-pass path (rows of the input) and the state path (rows of the store);
// tmp: the caller's buffer of at least mi_temp_bytes(G) bytes
dq_status mi_from_groups(Frame& fr, hipStream_t S, int64_t G, const int64_t* gc, const uint64_t* rep,
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

dq_status mi_from_joint(Frame& fr, dq_freq_table* t, const uint64_t* sorted_keys, const uint64_t* sorted_rows,
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

dq_status freq_build_impl(const int32_t* types, int32_t n_cols, const dq_column_view* cols,
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

}  // namespace

Arena<DeviceMem>& group_arena() { return g_arena; }

dq_status fill_iota_u64(uint64_t* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(iota_u64, dim3(grid_for(n)), dim3(256), 0, s, out, n);
  DQ_HIP(hipGetLastError());
  return DQ_OK;
}

}  // namespace dq

using namespace dq;

extern "C" {

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
  if (dq_status s = fill_iota_u64(rep, G, S)) return s;
  hipLaunchKernelGGL(store_col_keys, dim3(grid_for(G)), dim3(256), 0, S, st, G, xk, yk);
  DQ_HIP(hipGetLastError());
  const MiRequest mi{(double)num_rows, value, defined};
  return mi_from_groups(fr, S, G, t->d_counts.get(), rep, xk, yk, rep, d_store, tmp, mi);
}

}  // extern "C"
