// drift_args_check.cpp -- the argument validation of dq_freq_distance and dq_freq_ks (deequ_amd/csrc/dq_dist.hip) on
// the host, under ASan + UBSan: the calls that return before the device is touched and need no table -- a NULL result,
// a NULL table on either side -- and that a refused call writes nothing.  (What the entries say about two real
// tables -- types, arity, a table without its values -- needs tables, which live on the device: tests/test_drift_gpu.py.)
// A stand-alone program: the host side of dq_dist.hip and of what it links is compiled into it
// (tests/test_drift_host.py), dq::set_error is the one below, nothing is loaded into Python.
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
  const dq_freq_table* none = nullptr;
  // never dereferenced: every call below returns on a NULL before it reads a table
  const dq_freq_table* some = reinterpret_cast<const dq_freq_table*>(static_cast<uintptr_t>(64));
  dq_freq_distance_result res;
  std::memset(&res, 0x5A, sizeof(res));
  dq_freq_distance_result untouched;
  std::memset(&untouched, 0x5A, sizeof(untouched));
  double ks = -7.0;
  int32_t defined = -7;

  expect("distance: out NULL", dq_freq_distance(none, none, nullptr, nullptr), DQ_E_INVALID, "out is NULL");
  expect("distance: out NULL, tables given", dq_freq_distance(some, some, nullptr, nullptr), DQ_E_INVALID, "out is NULL");
  expect("distance: both NULL", dq_freq_distance(none, none, nullptr, &res), DQ_E_INVALID, "table is NULL");
  expect("distance: a NULL", dq_freq_distance(none, some, nullptr, &res), DQ_E_INVALID, "table is NULL");
  expect("distance: b NULL", dq_freq_distance(some, none, nullptr, &res), DQ_E_INVALID, "table is NULL");
  expect("ks: ks NULL", dq_freq_ks(some, some, nullptr, nullptr, &defined), DQ_E_INVALID, "is NULL");
  expect("ks: defined NULL", dq_freq_ks(some, some, nullptr, &ks, nullptr), DQ_E_INVALID, "is NULL");
  expect("ks: both NULL", dq_freq_ks(none, none, nullptr, &ks, &defined), DQ_E_INVALID, "table is NULL");
  expect("ks: a NULL", dq_freq_ks(none, some, nullptr, &ks, &defined), DQ_E_INVALID, "table is NULL");
  expect("ks: b NULL", dq_freq_ks(some, none, nullptr, &ks, &defined), DQ_E_INVALID, "table is NULL");
  // nothing was written by a refused call
  ++g_checks;
  if (std::memcmp(&res, &untouched, sizeof(res)) != 0 || ks != -7.0 || defined != -7) {
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
