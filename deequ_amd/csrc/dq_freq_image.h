// dq_freq_image.h -- the byte image of a frequency table (dq_freq_to_bytes / dq_freq_from_bytes): its layout and
// the host-only parser that checks an untrusted image before anything is allocated or copied.  No HIP here: the
// parser builds for the CPU alone (tests/freq_image_check.cpp runs it under ASan + UBSan).
//
// Layout (every integer little-endian, as written by the host; sections follow each other without gaps beyond the
// padding named here):
//   0   u8[4]  magic "DQFT"
//   4   u32    version (1)
//   8   u32    byte-order marker 0x01020304 as the writer's native u32 (a reader of the other order sees 0x04030201)
//   12  i32    n_cols (1..8)
//   16  i32    types[n_cols], each a dqscan.h type code (a DECIMAL128 code carries precision and scale);
//              one i32 of zero padding when n_cols is odd
//       i32    hashed (0 / 1), i32 reserved (0)
//       i64    n_groups (< 2^31), i64 n_values
//       u64    keys[n_groups]    strictly ascending
//       i64    counts[n_groups]  each >= 1, their sum n_values
//       u64    keys2[n_groups]   hashed tables only: the second tuple hash
//   then, hashed tables only, the value store, one section per grouping column in order:
//     fixed-width column: n_groups values of dq_freq_elem_size(type) bytes (a BOOL is one byte 0 / 1), zero-padded to
//                         a multiple of 8 bytes
//     utf8 / large_utf8:  i64 n_bytes, i64 offsets[n_groups + 1] (offsets[0] = 0, ascending, offsets[n_groups] =
//                         n_bytes), then n_bytes bytes, zero-padded to a multiple of 8 bytes
//   and nothing after the last section.  An unhashed table (one fixed-width numeric column) has no store: its keys
//   are its values.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/dqscan.h"

namespace dq {

constexpr int kFreqImageMaxCols = 8;
constexpr uint32_t kFreqImageVersion = 1;
constexpr uint32_t kFreqImageOrder = 0x01020304u;

// bytes of one stored value of a grouping column: 0 for strings (offsets + bytes), -1 for a type code the grouping
// path does not know
inline int dq_freq_elem_size(int32_t t) {
  if (t >= DQ_TYPE_F64 && t <= DQ_TYPE_TIMESTAMP) {
    switch (t) {
      case DQ_TYPE_F64: case DQ_TYPE_I64: case DQ_TYPE_TIMESTAMP: return 8;
      case DQ_TYPE_UTF8: case DQ_TYPE_LARGE_UTF8: return 0;
      case DQ_TYPE_I16: return 2;
      case DQ_TYPE_I8: case DQ_TYPE_BOOL: return 1;
      default: return 4;  // I32, F32, DATE32
    }
  }
  if ((t & ~0xFFFFFF) != 0 || DQ_TYPE_BASE(t) != DQ_TYPE_DECIMAL128) return -1;
  const int p = DQ_DECIMAL_PRECISION(t), s = DQ_DECIMAL_SCALE(t);
  return p >= 1 && p <= 38 && s <= p ? 16 : -1;
}

// where the sections of a checked image lie (byte offsets from its start)
struct FreqImageView {
  int32_t n_cols = 0;
  int32_t types[kFreqImageMaxCols] = {};
  int32_t hashed = 0;
  int64_t n_groups = 0, n_values = 0;
  int64_t keys = 0, counts = 0, keys2 = 0;   // keys2: 0 for unhashed tables
  int64_t col_offsets[kFreqImageMaxCols] = {};  // strings: the offsets array; else 0
  int64_t col_values[kFreqImageMaxCols] = {};   // the values (fixed width) or the bytes (strings)
  int64_t col_bytes[kFreqImageMaxCols] = {};    // their length without padding
};

// bytes of the image's header up to and including n_values
inline int64_t freq_image_header_bytes(int32_t n_cols) { return 16 + 4 * (int64_t)((n_cols + 1) & ~1) + 8 + 16; }
inline int64_t freq_image_pad8(int64_t n) { return (n + 7) & ~(int64_t)7; }

// Checks the image bytes[0 .. n) and fills *view: DQ_OK, or DQ_E_STATE with a message in err (at most err_cap bytes,
// NUL-terminated).  Reads nothing outside [bytes, bytes + n).
dq_status freq_image_parse(const uint8_t* bytes, int64_t n, FreqImageView* view, char* err, size_t err_cap);

}  // namespace dq
