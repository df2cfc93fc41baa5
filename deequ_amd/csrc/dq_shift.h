// dq_shift.h -- the shift of the shifted moment sums, one rule for the column, decimal and Correlation passes.
//
// Every pass sums z = x - shift and z^2 over a row range with ONE wave-uniform shift per (range, column) and closes
// with m2 = S2 - S1^2 / n (the pair pass: ck = Sab - Sa Sb / n as well).  The shift is the mean of the finite
// selected values of one 64-row group of the range.  Accuracy: that group's k values are part of the range, so
// (shift - mean)^2 <= m2 / k and n (shift - mean)^2 <= (n / k) m2 for any data (n: the range's selected rows): the
// cancellation in the closing formula costs ~(n / k) ulp.  k is the group's finite selected values, not its 64
// rows: under a sparse validity bitmap or `where` it can be 1, and one far value alone in a range's first group
// then cost 2e-11 of m2 (4e-11 in the pair pass, 2e-11 of the correlation) at 20 K-row ranges.  So the group is
// the first with at least kShiftMinRows selected rows, and only a range without one takes its first group with
// any (tests/test_moments_adversarial.py, measured errors in DESIGN.md section 2; tests/test_pair_lane.py drift
// test against a double-double reference; full-scale C2 / C4 / C5 in tests/fullscale_parity.py).
#pragma once

#include "dq_lane.h"

namespace dq {

// selected rows a 64-row group needs to give its range's shift while the range has such a group
constexpr int kShiftMinRows = 32;

// the first 64-row group of [row0, row1) with at least kShiftMinRows selected rows (row0 if there is none),
// from the bitmap words alone: lane l counts group l of each 4096-row stretch (row0 % 64 == 0; the words read
// are those the range's own pass reads).  Wave-uniform.
__device__ inline int64_t shift_group_start(const uint32_t* validity, const uint32_t* mask, int64_t row0, int64_t row1,
                                            int lane) {
  if (!validity && !mask) return row0;
  for (int64_t base = row0; base < row1; base += 64 * 64) {
    const int64_t r = base + 64 * lane;
    const int c = r < row1 ? __builtin_popcountll(sel_word<true>(validity, mask, r >> 5, row1 - r)) : 0;
    const uint64_t ok = __builtin_amdgcn_ballot_w64(c >= kShiftMinRows);
    if (ok != 0) return base + 64 * (int64_t)__builtin_amdgcn_readfirstlane(__builtin_ctzll(ok));
  }
  return row0;
}

// The shift of a column in [row0, row1) (wave-uniform; 0 if the range has no finite selected value): the groups
// are walked cyclically from shift_group_start, a group with no selected row is skipped on its bitmap words
// alone, and the first with a finite selected value gives its mean (fixed butterfly order).  value(r): this
// lane's value of row r as a double.  In the range's last group r runs past row1: value() must not read past
// the range there, and what it returns is not used.  The pair pass passes range-local rows and pointers (row0 = 0).
// The walk itself, over any `groups` 64-row groups: sel(g) the selection word of group g (wave-uniform), value(g)
// this lane's value of its row of group g.  range_shift below is the walk over a contiguous row range; the segmented
// scan (dq_segment.hip) walks the groups of a tile of gathered rows, whose selection words are ballots.
template <typename S, typename V>
__device__ __forceinline__ double groups_shift(int64_t groups, int64_t g0, S&& sel, V&& value) {
  for (int64_t i = 0; i < groups; ++i) {
    const int64_t g = g0 + i < groups ? g0 + i : g0 + i - groups;  // groups g0 .., then 0 .. g0 - 1
    const uint64_t s = sel(g);
    if (s == 0) continue;
    const double x = value(g);
    const uint64_t fm = __builtin_amdgcn_ballot_w64(__builtin_isfinite(x)) & s;
    if (fm != 0) return wave_uniform(wave_sum_f64(lane_bit(fm) ? x : 0.0) / (double)__builtin_popcountll(fm));
  }
  return 0.0;
}

template <typename V>
__device__ inline double range_shift(const uint32_t* validity, const uint32_t* mask, int64_t row0, int64_t row1, int lane,
                                     V&& value) {
  const int64_t groups = (row1 - row0 + 63) >> 6, g0 = (shift_group_start(validity, mask, row0, row1, lane) - row0) >> 6;
  return groups_shift(
      groups, g0, [&](int64_t g) { return sel_word(validity, mask, (row0 + 64 * g) >> 5, row1 - (row0 + 64 * g)); },
      [&](int64_t g) { return value(row0 + 64 * g + lane); });
}

}  // namespace dq
