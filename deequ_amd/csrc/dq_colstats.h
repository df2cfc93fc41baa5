// dq_colstats.h -- the Chan-mergeable statistics of one numeric column over a set of rows, and their merge: one copy
// for the column scan (dq_kernels.hip) and the segmented scan (dq_segment.hip).
#pragma once

#include <cstdint>

#include "dq_lane.h"

namespace dq {

// ------------------------------------------------------------------------------------------
// Chan-mergeable column statistics
// ------------------------------------------------------------------------------------------
struct ColStats {
  double n, mean, m2, sum;
  int64_t isum, count, nan_count;
  double fmin, fmax;
  int64_t pinf, ninf;  // selected +-inf values of an F64 column (outside n / mean / m2 / sum)
  int64_t isum_hi;     // D128: (isum, isum_hi) = the exact 128-bit sum (wrapping)
};

__device__ __forceinline__ void stats_init(ColStats& s) {
  s.n = 0.0; s.mean = 0.0; s.m2 = 0.0; s.sum = 0.0;
  s.isum = 0; s.count = 0; s.nan_count = 0;
  s.fmin = __longlong_as_double(0x7FF0000000000000ll);   // +inf
  s.fmax = __longlong_as_double((long long)0xFFF0000000000000ull);  // -inf
  s.pinf = 0; s.ninf = 0;
  s.isum_hi = 0;
}

// a <- a (+) b ; exact Chan/Welford combination (same algebra as StandardDeviationState.sum)
__device__ __forceinline__ void stats_merge(ColStats& a, const ColStats& b) {
  double n = a.n + b.n;
  if (b.n != 0.0) {
    if (a.n == 0.0) {
      a.mean = b.mean; a.m2 = b.m2;
    } else {
      double delta = b.mean - a.mean;
      double r = b.n / n;
      a.mean = a.mean + delta * r;
      a.m2 = a.m2 + b.m2 + delta * delta * a.n * r;
    }
  }
  a.n = n;
  a.sum += b.sum;
  {  // 128-bit add (the high word only matters for decimal columns)
    const uint64_t lo = (uint64_t)a.isum + (uint64_t)b.isum;
    a.isum_hi = (int64_t)((uint64_t)a.isum_hi + (uint64_t)b.isum_hi + (lo < (uint64_t)a.isum ? 1u : 0u));
    a.isum = (int64_t)lo;
  }
  a.count += b.count;
  a.nan_count += b.nan_count;
  a.fmin = hw_min(a.fmin, b.fmin);
  a.fmax = hw_max(a.fmax, b.fmax);
  a.pinf += b.pinf;
  a.ninf += b.ninf;
}

}  // namespace dq
