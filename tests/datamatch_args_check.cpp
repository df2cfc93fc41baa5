// datamatch_args_check.cpp -- the argument validation of dq_freq_lookup_rows and dq_rows_match
// (deequ_amd/csrc/dq_probe.hip) on the host, under ASan + UBSan: every invalid argument that returns before the device
// is touched.  dq_freq_lookup_rows checks in dq_freq_contains_rows's order (n_rows, alignment, NULL group / cols /
// table); dq_rows_match checks n_cols, n_rows, n_payload_rows, alignment, NULL arguments, the types, the views'
// buffers -- none of these calls needs a table or a GPU.  A stand-alone program: dq_probe.hip's host side is compiled
// into it (tests/test_datamatch_args_host.py), dq::set_error is the one below, nothing is loaded into Python.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "dqscan.h"

namespace dq {
static char g_err[512];
dq_status set_error(dq_status code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace dq

static int g_checks = 0, g_failed = 0;

static void expect(const char* what, dq_status got, dq_status want, const char* text) {
  ++g_checks;
  const bool ok = got == want && (!text || std::strstr(dq::g_err, text));
  if (!ok) {
    ++g_failed;
    std::printf("FAIL %s: status %d (want %d), message '%s' (want '%s')\n", what, got, want, dq::g_err, text ? text : "");
  }
  dq::g_err[0] = 0;
}

int main() {
  alignas(16) uint64_t word[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // never dereferenced: these calls return before a launch
  uint64_t* const ok = word;
  uint64_t* const odd = reinterpret_cast<uint64_t*>(reinterpret_cast<uintptr_t>(word) + 4);
  int32_t* const grp = reinterpret_cast<int32_t*>(word + 4);
  int32_t* const grp_odd = reinterpret_cast<int32_t*>(reinterpret_cast<uintptr_t>(word + 4) + 2);
  dq_column_view view;
  std::memset(&view, 0, sizeof(view));
  int64_t nf = -7;
  const dq_freq_table* none = nullptr;

  // ---- dq_freq_lookup_rows
  expect("lookup n_rows < 0", dq_freq_lookup_rows(none, nullptr, &view, -1, nullptr, grp, nullptr, &nf), DQ_E_INVALID,
         "dq_freq_lookup_rows: 0 <= n_rows < 2^31");
  expect("lookup n_rows = 2^31", dq_freq_lookup_rows(none, nullptr, &view, 1ll << 31, nullptr, grp, nullptr, &nf),
         DQ_E_INVALID, "n_rows < 2^31");
  expect("lookup n_rows = INT64_MIN", dq_freq_lookup_rows(none, nullptr, &view, INT64_MIN, nullptr, grp, nullptr, &nf),
         DQ_E_INVALID, "n_rows < 2^31");
  expect("lookup filter misaligned", dq_freq_lookup_rows(none, nullptr, &view, 1, odd, grp, nullptr, &nf), DQ_E_INVALID,
         "8-byte aligned");
  expect("lookup group misaligned", dq_freq_lookup_rows(none, nullptr, &view, 1, nullptr, grp_odd, nullptr, &nf),
         DQ_E_INVALID, "group must be a 4-byte aligned");
  expect("lookup group misaligned, no rows", dq_freq_lookup_rows(none, nullptr, &view, 0, nullptr, grp_odd, nullptr, &nf),
         DQ_E_INVALID, "group must be a 4-byte aligned");
  expect("lookup group NULL", dq_freq_lookup_rows(none, nullptr, &view, 1, nullptr, nullptr, nullptr, &nf), DQ_E_INVALID,
         "group is NULL");
  expect("lookup cols NULL", dq_freq_lookup_rows(none, nullptr, nullptr, 1, nullptr, grp, nullptr, &nf), DQ_E_INVALID,
         "cols is NULL");
  expect("lookup table NULL", dq_freq_lookup_rows(none, nullptr, &view, 64, ok, grp, nullptr, &nf), DQ_E_INVALID,
         "dq_freq_lookup_rows: table is NULL");
  expect("lookup table NULL, no rows", dq_freq_lookup_rows(none, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &nf),
         DQ_E_INVALID, "table is NULL");

  // ---- dq_rows_match
  int64_t nm = -7, nfound = -7, na = -7, mis[17];
  for (int i = 0; i < 17; ++i) mis[i] = -7;
  int32_t f64[17], i64[17], i32[17], utf8[17], large[17], dec102[17], dec103[17], dict[17];
  dq_column_view views[17], bad[17];
  std::memset(views, 0, sizeof(views));
  for (int i = 0; i < 17; ++i) {
    f64[i] = DQ_TYPE_F64, i64[i] = DQ_TYPE_I64, i32[i] = DQ_TYPE_I32, utf8[i] = DQ_TYPE_UTF8, large[i] = DQ_TYPE_LARGE_UTF8;
    dec102[i] = DQ_DECIMAL128(10, 2), dec103[i] = DQ_DECIMAL128(10, 3), dict[i] = DQ_TYPE_DICT_UTF8;
    views[i].values = word;  // (a pointer the entry checks and never follows here)
    views[i].offsets = word;
  }
  auto match = [&](const int32_t* ta, const dq_column_view* ca, const int32_t* tp, const dq_column_view* cp, int32_t k,
                   int64_t n, int64_t g, const int32_t* group, const uint64_t* filter, uint64_t* matched, uint64_t* found,
                   uint64_t* applies) {
    return dq_rows_match(ta, ca, tp, cp, k, n, g, group, filter, matched, found, applies, 0, nullptr, &nm, &nfound, &na, mis);
  };
  expect("n_cols = 0", match(f64, views, f64, views, 0, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "1 <= n_cols <= 16, got 0");
  expect("n_cols = 17", match(f64, views, f64, views, 17, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "1 <= n_cols <= 16, got 17");
  expect("n_cols < 0", match(f64, views, f64, views, -1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID, "n_cols");
  expect("n_rows < 0", match(f64, views, f64, views, 1, -1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "dq_rows_match: 0 <= n_rows < 2^31");
  expect("n_rows = 2^31", match(f64, views, f64, views, 1, 1ll << 31, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "n_rows < 2^31");
  expect("n_rows = INT64_MIN", match(f64, views, f64, views, 1, INT64_MIN, 1, grp, nullptr, ok, nullptr, nullptr),
         DQ_E_INVALID, "n_rows < 2^31");
  expect("n_payload_rows < 0", match(f64, views, f64, views, 1, 1, -1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "n_payload_rows < 0");
  expect("matched misaligned", match(f64, views, f64, views, 1, 1, 1, grp, nullptr, odd, nullptr, nullptr), DQ_E_INVALID,
         "8-byte aligned");
  expect("found misaligned", match(f64, views, f64, views, 1, 1, 1, grp, nullptr, ok, odd, nullptr), DQ_E_INVALID,
         "8-byte aligned");
  expect("applies misaligned", match(f64, views, f64, views, 1, 1, 1, grp, nullptr, ok, nullptr, odd), DQ_E_INVALID,
         "8-byte aligned");
  expect("filter misaligned", match(f64, views, f64, views, 1, 1, 1, grp, odd, ok, nullptr, nullptr), DQ_E_INVALID,
         "8-byte aligned");
  expect("matched misaligned, no rows", match(f64, views, f64, views, 1, 0, 0, grp, nullptr, odd, nullptr, nullptr),
         DQ_E_INVALID, "8-byte aligned");
  expect("group misaligned", match(f64, views, f64, views, 1, 1, 1, grp_odd, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "group must be a 4-byte aligned");
  expect("types NULL", match(nullptr, views, f64, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "types is NULL");
  expect("payload types NULL", match(f64, views, nullptr, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr),
         DQ_E_INVALID, "types is NULL");
  expect("matched NULL", match(f64, views, f64, views, 1, 1, 1, grp, nullptr, nullptr, ok, ok), DQ_E_INVALID,
         "matched is NULL");
  expect("group NULL", match(f64, views, f64, views, 1, 1, 1, nullptr, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "group is NULL");
  expect("cols NULL", match(f64, nullptr, f64, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "cols is NULL");
  expect("payload NULL", match(f64, views, f64, nullptr, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "cols is NULL");
  // a type mismatch names the column and both codes: no widening, a decimal's scale is part of its type, a dictionary
  // column is not taken; the two string widths agree (the call then fails later, on the missing buffer)
  char want[96];
  std::snprintf(want, sizeof(want), "column 1 has type %d, the payload's has %d", DQ_TYPE_I32, DQ_TYPE_I64);
  int32_t mixed[2] = {DQ_TYPE_I64, DQ_TYPE_I32};
  expect("i32 against i64", match(mixed, views, i64, views, 2, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID, want);
  std::snprintf(want, sizeof(want), "column 0 has type %d, the payload's has %d", DQ_DECIMAL128(10, 3), DQ_DECIMAL128(10, 2));
  expect("decimal scale", match(dec103, views, dec102, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID, want);
  std::snprintf(want, sizeof(want), "column 0 has type %d, the payload's has %d", DQ_TYPE_UTF8, DQ_TYPE_I64);
  expect("utf8 against i64", match(utf8, views, i64, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID, want);
  expect("dict_utf8", match(dict, views, dict, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "column 0 has type 13");
  const int32_t zero[1] = {0};
  expect("type 0", match(zero, views, zero, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "column 0 has type 0");
  expect("type mismatch, no rows", match(i32, views, i64, views, 1, 0, 0, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "column 0 has type");
  // the views' buffers
  std::memcpy(bad, views, sizeof(views));
  bad[1].values = nullptr;
  expect("values NULL", match(f64, bad, f64, views, 2, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "dq_rows_match: column 1: missing or misaligned buffer");
  expect("payload values NULL", match(f64, views, f64, bad, 2, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "payload column 1: missing or misaligned buffer");
  std::memcpy(bad, views, sizeof(views));
  bad[0].validity = reinterpret_cast<const uint8_t*>(word) + 2;
  expect("validity misaligned", match(f64, bad, f64, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "column 0: missing or misaligned buffer");
  std::memcpy(bad, views, sizeof(views));
  bad[0].offsets = nullptr;
  expect("utf8 without offsets", match(utf8, bad, large, views, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr), DQ_E_INVALID,
         "dq_rows_match: column 0: missing or misaligned buffer");
  expect("payload large_utf8 without offsets", match(utf8, views, large, bad, 1, 1, 1, grp, nullptr, ok, nullptr, nullptr),
         DQ_E_INVALID, "payload column 0: missing or misaligned buffer");

  // nothing was written: not the counts, not the words
  ++g_checks;
  bool wrote = nf != -7 || nm != -7 || nfound != -7 || na != -7;
  for (int i = 0; i < 17; ++i) wrote = wrote || mis[i] != -7;
  for (int i = 0; i < 8; ++i) wrote = wrote || word[i] != 0;
  if (wrote) {
    ++g_failed;
    std::printf("FAIL a refused call wrote its outputs\n");
  }
  if (g_failed) {
    std::printf("failed %d of %d\n", g_failed, g_checks);
    return 1;
  }
  std::printf("ok %d checks\n", g_checks);
  return 0;
}
