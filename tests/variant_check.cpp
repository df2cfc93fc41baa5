// Host build of the column-pass variant table (deequ_amd/csrc/dq_device.h kVariants), driven by
// tests/test_variant_table.py.  Prints one row per variant: "index kind stats hll dtype name", then one line
// "find <index> <cv_find of the row's own description>" per variant (the inverse lookup at run time; the header's
// static_asserts check the same at compile time).
#include <cstdio>

#include "../deequ_amd/csrc/dq_device.h"

int main() {
  for (int v = 0; v < dq::kNumVariants; ++v)
    std::printf("%d %d %d %d %d %s\n", v, (int)dq::cv_kind(v), (int)dq::cv_stats(v), (int)dq::cv_hll(v),
                (int)dq::cv_dtype(v), dq::kVariants[v].name);
  for (int v = 0; v < dq::kNumVariants; ++v)
    std::printf("find %d %d\n", v, (int)dq::cv_find(dq::cv_kind(v), dq::cv_stats(v), dq::cv_hll(v), dq::cv_dtype(v)));
  std::printf("find none %d\n", (int)dq::cv_find(dq::CK_UTF8, true, false, false));  // no such variant
  return 0;
}
