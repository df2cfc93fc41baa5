// segment_args_check.cpp -- the argument validation of dq_segment_order and dq_segment_scan
// (deequ_amd/csrc/dq_segment.hip) on the host, under ASan + UBSan: the calls that return before the device is touched
// -- NULL pointers, negative sizes, n_slots out of range, an unknown op or type, G + 1 beyond int32 -- and that a
// refused call writes nothing.  (What the entries compute needs a device: tests/test_segment_gpu.py.)
// A stand-alone program: the host side of dq_segment.hip and of what it links is compiled into it
// (tests/test_segment_args_host.py), dq::set_error is the one below, nothing is loaded into Python.
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
  // never dereferenced: every call below returns before it reads or writes a buffer
  auto fake = [](uintptr_t a) { return reinterpret_cast<void*>(a); };
  const int32_t* seg = static_cast<const int32_t*>(fake(256));
  int32_t* perm = static_cast<int32_t*>(fake(512));
  int64_t* offsets = static_cast<int64_t*>(fake(1024));
  dq_segment_state* out = static_cast<dq_segment_state*>(fake(2048));
  const int64_t big = 0x7FFFFFFFll;

  expect("order: n_rows negative", dq_segment_order(seg, -1, 4, perm, offsets, nullptr), DQ_E_INVALID, "n_rows");
  expect("order: n_rows beyond int32", dq_segment_order(seg, big + 1, 4, perm, offsets, nullptr), DQ_E_INVALID, "n_rows");
  expect("order: G negative", dq_segment_order(seg, 8, -1, perm, offsets, nullptr), DQ_E_INVALID, "negative");
  expect("order: G + 1 beyond int32", dq_segment_order(seg, 8, big, perm, offsets, nullptr), DQ_E_UNSUPPORTED, "exceed int32");
  expect("order: offsets NULL", dq_segment_order(seg, 8, 4, perm, nullptr, nullptr), DQ_E_INVALID, "offsets is NULL");
  expect("order: offsets NULL, no rows", dq_segment_order(nullptr, 0, 4, nullptr, nullptr, nullptr), DQ_E_INVALID, "offsets is NULL");
  expect("order: seg NULL", dq_segment_order(nullptr, 8, 4, perm, offsets, nullptr), DQ_E_INVALID, "is NULL");
  expect("order: perm NULL", dq_segment_order(seg, 8, 4, nullptr, offsets, nullptr), DQ_E_INVALID, "is NULL");

  dq_segment_slot slots[DQ_SEGMENT_MAX_SLOTS + 1];
  std::memset(slots, 0, sizeof(slots));
  for (auto& s : slots) s.op = DQ_SEG_COUNT;
  expect("scan: n_slots 0", dq_segment_scan(slots, 0, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "n_slots");
  expect("scan: n_slots negative", dq_segment_scan(slots, -3, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "n_slots");
  expect("scan: n_slots 65", dq_segment_scan(slots, DQ_SEGMENT_MAX_SLOTS + 1, perm, offsets, 5, out, nullptr), DQ_E_INVALID,
         "n_slots");
  expect("scan: G1 0", dq_segment_scan(slots, 1, perm, offsets, 0, out, nullptr), DQ_E_INVALID, "G1");
  expect("scan: G1 negative", dq_segment_scan(slots, 1, perm, offsets, -2, out, nullptr), DQ_E_INVALID, "G1");
  expect("scan: G1 beyond int32", dq_segment_scan(slots, 1, perm, offsets, big + 1, out, nullptr), DQ_E_UNSUPPORTED,
         "exceed int32");
  expect("scan: slots NULL", dq_segment_scan(nullptr, 1, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "is NULL");
  expect("scan: offsets NULL", dq_segment_scan(slots, 1, perm, nullptr, 5, out, nullptr), DQ_E_INVALID, "is NULL");
  expect("scan: out NULL", dq_segment_scan(slots, 1, perm, offsets, 5, nullptr, nullptr), DQ_E_INVALID, "is NULL");
  slots[1].op = 0;
  expect("scan: op 0", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "slot 1: unknown op");
  slots[1].op = 99;
  expect("scan: op 99", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "slot 1: unknown op");
  slots[1].op = DQ_SEG_STATS;
  slots[1].col.values = fake(4096);
  slots[1].type = 0;
  expect("scan: type 0", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "slot 1: unknown type");
  slots[1].type = DQ_TYPE_MAX + 1;
  expect("scan: type past the enum", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "unknown type");
  slots[1].type = DQ_TYPE_UTF8;
  expect("scan: string statistics", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_UNSUPPORTED,
         "no segmented statistics");
  slots[1].type = DQ_DECIMAL128(10, 2);
  expect("scan: decimal statistics", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_UNSUPPORTED,
         "no segmented statistics");
  slots[1].type = DQ_TYPE_F64;
  slots[1].col.values = nullptr;
  expect("scan: values NULL", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "values is NULL");
  slots[1].col.values = fake(4096);
  slots[1].filter = static_cast<const uint64_t*>(fake(4098));
  expect("scan: misaligned filter", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "aligned");
  slots[1].filter = nullptr;
  slots[0].col.validity = static_cast<const uint8_t*>(fake(4097));
  expect("scan: misaligned validity", dq_segment_scan(slots, 2, perm, offsets, 5, out, nullptr), DQ_E_INVALID, "aligned");

  ++g_checks;
  if (dq_segment_tile() != DQ_SEGMENT_TILE || DQ_SEGMENT_TILE % 64 != 0) {
    ++g_failed;
    std::printf("FAIL dq_segment_tile() is %d, the header says %d\n", dq_segment_tile(), DQ_SEGMENT_TILE);
  }
  if (g_failed) {
    std::printf("failed %d of %d\n", g_failed, g_checks);
    return 1;
  }
  std::printf("ok %d checks\n", g_checks);
  return 0;
}
