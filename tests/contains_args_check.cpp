// contains_args_check.cpp -- the argument validation of dq_freq_contains_rows (deequ_amd/csrc/dq_probe.hip) on the
// host, under ASan + UBSan: every combination of invalid arguments that returns before the device is touched.  The
// entry checks, in this order and before any HIP call: n_rows, the bitmaps' alignment, NULL contained, NULL cols,
// NULL table -- so none of these calls needs a table or a GPU.  A stand-alone program: dq_probe.hip's host side is
// compiled into it (tests/test_refint_args_host.py), dq::set_error is the one below, nothing is loaded into Python.
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
  alignas(8) uint64_t word[4] = {0, 0, 0, 0};  // never dereferenced by the entry: these calls return before a launch
  uint64_t* const ok = word;
  uint64_t* const odd = reinterpret_cast<uint64_t*>(reinterpret_cast<uintptr_t>(word) + 4);
  dq_column_view view;
  std::memset(&view, 0, sizeof(view));
  int64_t nc = -7, na = -7;
  const dq_freq_table* none = nullptr;

  // n_rows: negative, 2^31 and beyond, with a 1-row buffer -- rejected on the argument alone
  expect("n_rows < 0", dq_freq_contains_rows(none, nullptr, &view, -1, nullptr, ok, nullptr, nullptr, &nc, &na),
         DQ_E_INVALID, "n_rows < 2^31");
  expect("n_rows = 2^31", dq_freq_contains_rows(none, nullptr, &view, 1ll << 31, nullptr, ok, nullptr, nullptr, &nc, &na),
         DQ_E_INVALID, "n_rows < 2^31");
  expect("n_rows = 2^40", dq_freq_contains_rows(none, nullptr, &view, 1ll << 40, nullptr, ok, ok, nullptr, &nc, &na),
         DQ_E_INVALID, "n_rows < 2^31");
  expect("n_rows = INT64_MIN", dq_freq_contains_rows(none, nullptr, &view, INT64_MIN, nullptr, ok, ok, nullptr, &nc, &na),
         DQ_E_INVALID, "n_rows < 2^31");
  // misaligned bitmaps: contained, applies, filter -- each alone, and with n_rows = 0
  expect("contained misaligned", dq_freq_contains_rows(none, nullptr, &view, 1, nullptr, odd, nullptr, nullptr, &nc, &na),
         DQ_E_INVALID, "8-byte aligned");
  expect("applies misaligned", dq_freq_contains_rows(none, nullptr, &view, 1, nullptr, ok, odd, nullptr, &nc, &na),
         DQ_E_INVALID, "8-byte aligned");
  expect("filter misaligned", dq_freq_contains_rows(none, nullptr, &view, 1, odd, ok, ok, nullptr, &nc, &na),
         DQ_E_INVALID, "8-byte aligned");
  expect("contained misaligned, no rows", dq_freq_contains_rows(none, nullptr, &view, 0, nullptr, odd, nullptr, nullptr, &nc, &na),
         DQ_E_INVALID, "8-byte aligned");
  // NULL contained / cols with rows to write
  expect("contained NULL", dq_freq_contains_rows(none, nullptr, &view, 1, nullptr, nullptr, ok, nullptr, &nc, &na),
         DQ_E_INVALID, "contained is NULL");
  expect("cols NULL", dq_freq_contains_rows(none, nullptr, nullptr, 1, nullptr, ok, ok, nullptr, &nc, &na),
         DQ_E_INVALID, "cols is NULL");
  // NULL table: with rows, without rows, without the optional outputs
  expect("table NULL", dq_freq_contains_rows(none, nullptr, &view, 64, ok, ok, ok, nullptr, &nc, &na),
         DQ_E_INVALID, "table is NULL");
  expect("table NULL, no rows", dq_freq_contains_rows(none, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &nc, &na),
         DQ_E_INVALID, "table is NULL");
  expect("table NULL, no counts", dq_freq_contains_rows(none, nullptr, &view, 1, nullptr, ok, nullptr, nullptr, nullptr, nullptr),
         DQ_E_INVALID, "table is NULL");
  // nothing was written: not the counts, not the words
  ++g_checks;
  if (nc != -7 || na != -7 || word[0] | word[1] | word[2] | word[3]) {
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
