// dq_upload_host.h -- the CPU side of an upload: the copy pieces dq_upload (dq_ingest.cpp) and dq_upload_stage
// (dq_upload_host.cpp) cut a chunk's host columns into, and the thread pool that copies them.  Host only: no HIP
// header, so a stand-alone program drives it without a runtime (tests/upload_to_check.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/dqscan.h"

namespace dq {
dq_status set_error(dq_status code, const char* fmt, ...);  // (dq_internal.h; thread-local last error)

namespace up {

constexpr int64_t kAlign = 256;  // every buffer of a slot starts 256-byte aligned (values need 16)

inline int64_t align_up(int64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// bytes per value of a fixed-width type (BOOL: bit-packed, 0)
inline int64_t value_width(int32_t type) {
  switch (type) {
    case DQ_TYPE_F64: case DQ_TYPE_I64: case DQ_TYPE_TIMESTAMP: return 8;
    case DQ_TYPE_I32: case DQ_TYPE_F32: case DQ_TYPE_DATE32: return 4;
    case DQ_TYPE_I16: return 2;
    case DQ_TYPE_I8: return 1;
    default: return DQ_TYPE_BASE(type) == DQ_TYPE_DECIMAL128 ? 16 : 0;
  }
}

// parallel copy of a list of pieces over up to `threads` CPU threads.  A piece is a memcpy, or -- for an
// Arrow slice -- a rebase of its string offsets (minus the slice's first offset) or a shift of its
// validity bitmap (the slice's row 0 at bit `shift` of the first source byte).
struct Piece {
  char* dst;
  const char* src;
  int64_t bytes;           // destination bytes
  int kind = 0;            // 0 memcpy, 1 int32 offsets - base, 2 int64 offsets - base, 3 bitmap >> shift
  int64_t base = 0;        // kinds 1, 2
  int shift = 0;           // kind 3 (1..7)
  int64_t src_bytes = 0;   // kind 3: readable source bytes
  // kind 4: dictionary indices widened to int32 and range-checked (dq_dict_check_indices' loop)
  int idx_type = 0;                  // DQ_TYPE_I8 / I16 / I32, negative: unsigned
  int64_t n_entries = 0;
  const uint8_t* valid = nullptr;    // the rows' bitmap (row 0 at bit valid_bit) or NULL
  int valid_bit = 0;
  std::atomic<int64_t>* bad = nullptr;  // the lowest offending row, or INT64_MAX
  // kind 5: fixed-width values of `width` bytes, a NULL row's value written 0 (dq_upload_stage); kind 6: the same
  // for decimal128 with every valid row's unscaled value checked against 10^precision (`bad` as for kind 4)
  int width = 0;
  int precision = 0;
};

// Rows [r0, r1) of a dictionary index array of `type` widened to int32 (out may be NULL) and checked against
// [0, n_entries) where the row's validity bit (bit r + bit of `validity`, NULL: every row) is set; a NULL row's
// index is written 0.  Returns the first offending row (its index in *bad_value), or -1.
inline int64_t widen_check(int type, const void* src, int64_t r0, int64_t r1, const uint8_t* validity, int bit,
                           int64_t n_entries, int32_t* out, int64_t* bad_value) {
  auto run = [&](auto tag) -> int64_t {
    using T = decltype(tag);
    const char* p = static_cast<const char*>(src);
    for (int64_t r = r0; r < r1; ++r) {
      T t;
      std::memcpy(&t, p + r * (int64_t)sizeof(T), sizeof(T));
      const int64_t v = (int64_t)t, b = r + bit;
      const bool valid = !validity || ((validity[b >> 3] >> (b & 7)) & 1);
      if (valid && (v < 0 || v >= n_entries)) {
        if (bad_value) *bad_value = v;
        return r;
      }
      if (out) out[r] = valid ? (int32_t)v : 0;
    }
    return -1;
  };
  switch (type) {
    case DQ_TYPE_I8: return run(int8_t{});
    case DQ_TYPE_I16: return run(int16_t{});
    case DQ_TYPE_I32: return run(int32_t{});
    case -DQ_TYPE_I8: return run(uint8_t{});
    default: return run(uint16_t{});  // -DQ_TYPE_I16 (index_type_ok)
  }
}
inline bool index_type_ok(int t) {
  return t == DQ_TYPE_I8 || t == DQ_TYPE_I16 || t == DQ_TYPE_I32 || t == -DQ_TYPE_I8 || t == -DQ_TYPE_I16;
}

// |unscaled value| >= 10^precision for the 16 little-endian two's-complement bytes at `src` (precision 1..38)
inline bool decimal_exceeds(const char* src, int precision) {
  uint64_t lo, hi;
  std::memcpy(&lo, src, 8);
  std::memcpy(&hi, src + 8, 8);
  unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
  if (hi >> 63) v = ~v + 1;  // (-2^127 stays 2^127: over every limit)
  unsigned __int128 limit = 1;
  for (int k = 0; k < precision; ++k) limit *= 10;
  return v >= limit;
}

inline void note_bad(std::atomic<int64_t>* bad, int64_t r) {
  int64_t cur = bad->load();
  while (r < cur && !bad->compare_exchange_weak(cur, r)) {}
}

inline void copy_part(const Piece& p, int64_t a, int64_t b) {  // destination bytes [a, b) of piece p
  switch (p.kind) {
    case 0: std::memcpy(p.dst + a, p.src + a, (size_t)(b - a)); break;
    case 1: {
      const int32_t base = (int32_t)p.base;
      for (int64_t i = a / 4; i < b / 4; ++i) {
        int32_t v;
        std::memcpy(&v, p.src + 4 * i, 4);
        v -= base;
        std::memcpy(p.dst + 4 * i, &v, 4);
      }
      break;
    }
    case 2:
      for (int64_t i = a / 8; i < b / 8; ++i) {
        int64_t v;
        std::memcpy(&v, p.src + 8 * i, 8);
        v -= p.base;
        std::memcpy(p.dst + 8 * i, &v, 8);
      }
      break;
    case 4: {
      int64_t v = 0;
      const int64_t r = widen_check(p.idx_type, p.src, a / 4, b / 4, p.valid, p.valid_bit, p.n_entries,
                                    reinterpret_cast<int32_t*>(p.dst), &v);
      if (r >= 0) {
        int64_t cur = p.bad->load();
        while (r < cur && !p.bad->compare_exchange_weak(cur, r)) {}
      }
      break;
    }
    case 5:
    case 6: {
      // a share boundary is a multiple of 8 bytes: a 16-byte value may lie across it, so a NULL row is cleared
      // over its part of [a, b) and a value is checked by the share that holds its first byte
      std::memcpy(p.dst + a, p.src + a, (size_t)(b - a));
      const int64_t w = p.width;
      for (int64_t r = a / w; r * w < b; ++r) {
        const int64_t bit = r + p.valid_bit;
        if (p.valid && !((p.valid[bit >> 3] >> (bit & 7)) & 1)) {
          const int64_t lo = std::max(a, r * w), hi = std::min(b, (r + 1) * w);
          std::memset(p.dst + lo, 0, (size_t)(hi - lo));
        } else if (p.kind == 6 && r * w >= a && decimal_exceeds(p.src + r * w, p.precision)) {
          note_bad(p.bad, r);
        }
      }
      break;
    }
    default: {
      const uint8_t* src = reinterpret_cast<const uint8_t*>(p.src);
      for (int64_t i = a; i < b; ++i) {
        const uint32_t lo = src[i], hi = i + 1 < p.src_bytes ? src[i + 1] : 0u;
        p.dst[i] = (char)(uint8_t)((lo >> p.shift) | (hi << (8 - p.shift)));
      }
    }
  }
}

inline void parallel_copy(const std::vector<Piece>& pieces, int threads) {
  int64_t total = 0;
  for (const Piece& p : pieces) total += p.bytes;
  constexpr int64_t kGrain = 8 << 20;
  const int n = (int)std::max<int64_t>(1, std::min<int64_t>(threads, total / kGrain));
  if (n <= 1) {
    for (const Piece& p : pieces)
      if (p.bytes) copy_part(p, 0, p.bytes);
    return;
  }
  // split the concatenated byte range [0, total) into n contiguous shares; inside a piece the share
  // boundaries are rounded down to 8 bytes (whole offsets), the same way on both sides of a boundary
  auto work = [&](int t) {
    const int64_t lo = total * t / n, hi = total * (t + 1) / n;
    int64_t at = 0;
    for (const Piece& p : pieces) {
      if (at + p.bytes > lo && at < hi) {
        const int64_t a = lo <= at ? 0 : ((lo - at) & ~int64_t(7));
        const int64_t b = hi >= at + p.bytes ? p.bytes : ((hi - at) & ~int64_t(7));
        if (a < b) copy_part(p, a, b);
      }
      at += p.bytes;
      if (at >= hi) break;
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < n; ++t) pool.emplace_back(work, t);
  work(0);
  for (std::thread& th : pool) th.join();
}

// ---- the host half of dq_upload_to (dq_upload_payload / dq_upload_stage, dq_upload_host.cpp) ----

inline bool is_string(int32_t t) { return t == DQ_TYPE_UTF8 || t == DQ_TYPE_LARGE_UTF8; }
inline bool is_decimal(int32_t t) { return DQ_TYPE_BASE(t) == DQ_TYPE_DECIMAL128; }

inline bool row_valid(const dq_host_column& h, int64_t r) {
  const int64_t b = r + h.validity_bit;
  return !h.validity || ((h.validity[b >> 3] >> (b & 7)) & 1);
}

inline int64_t offset_at(const dq_host_column& h, int64_t r) {
  if (h.type == DQ_TYPE_UTF8) {
    int32_t v;
    std::memcpy(&v, static_cast<const char*>(h.offsets) + 4 * r, 4);
    return v;
  }
  int64_t v;
  std::memcpy(&v, static_cast<const char*>(h.offsets) + 8 * r, 8);
  return v;
}

// What dq_arrow_import / dq_arrow_import_dictionary promise about a host column, checked before anything reads
// through it: (n_rows, byte counts and buffers agree with the type).
inline dq_status check_column(const char* me, int32_t c, const dq_host_column& h) {
  const int64_t n = h.n_rows;
  if (n < 0 || h.validity_bit < 0 || h.validity_bit > 7 || h.offset_base < 0)
    return set_error(DQ_E_INVALID, "%s: column %d: bad row count / slice rebase", me, c);
  if (h.validity && h.validity_bytes != (n + 7) / 8)
    return set_error(DQ_E_INVALID, "%s: column %d: validity of %lld bytes for %lld rows", me, c,
                     (long long)h.validity_bytes, (long long)n);
  int64_t want = -1;
  if (h.type == DQ_TYPE_DICT_UTF8) {
    if (!index_type_ok(h.reserved) || h.offsets)
      return set_error(DQ_E_INVALID, "%s: column %d: not a dictionary index column of dq_arrow_import_dictionary", me, c);
    want = 4 * n;
  } else if (h.type == DQ_TYPE_BOOL) {
    want = (n + 7) / 8;
  } else if (value_width(h.type) > 0) {
    if (is_decimal(h.type) && (DQ_DECIMAL_PRECISION(h.type) < 1 || DQ_DECIMAL_PRECISION(h.type) > 38))
      return set_error(DQ_E_INVALID, "%s: column %d: decimal precision %d", me, c, DQ_DECIMAL_PRECISION(h.type));
    want = n * value_width(h.type);
  } else if (!is_string(h.type)) {
    return set_error(DQ_E_INVALID, "%s: column %d: type code %d", me, c, h.type);
  }
  if (want >= 0 && (h.value_bytes != want || (n > 0 && !h.values)))
    return set_error(DQ_E_INVALID, "%s: column %d: %lld value bytes for %lld rows", me, c, (long long)h.value_bytes,
                     (long long)n);
  if (is_string(h.type) && n > 0) {
    const int64_t w = h.type == DQ_TYPE_UTF8 ? 4 : 8;
    if (!h.offsets || h.offset_bytes != (n + 1) * w || h.value_bytes < 0 || (h.value_bytes > 0 && !h.values))
      return set_error(DQ_E_INVALID, "%s: column %d: string column without its offsets / data", me, c);
  }
  return DQ_OK;
}

// The bytes of a string column's non-NULL rows; its offsets must start at offset_base, never decrease and end at
// offset_base + value_bytes (so that no row reads outside the data).
inline dq_status string_payload(const char* me, int32_t c, const dq_host_column& h, int64_t* bytes) {
  *bytes = 0;
  if (h.n_rows == 0) return DQ_OK;
  int64_t prev = offset_at(h, 0), kept = 0;
  if (prev != h.offset_base) return set_error(DQ_E_INVALID, "%s: column %d: offsets do not start at the slice's base", me, c);
  for (int64_t r = 0; r < h.n_rows; ++r) {
    const int64_t next = offset_at(h, r + 1);
    if (next < prev || next - h.offset_base > h.value_bytes)
      return set_error(DQ_E_INVALID, "%s: column %d: string offsets decrease or leave the data at row %lld", me, c,
                       (long long)r);
    if (row_valid(h, r)) kept += next - prev;
    prev = next;
  }
  if (prev - h.offset_base != h.value_bytes)
    return set_error(DQ_E_INVALID, "%s: column %d: string offsets end at %lld of %lld data bytes", me, c,
                     (long long)(prev - h.offset_base), (long long)h.value_bytes);
  *bytes = kept;
  return DQ_OK;
}

inline void clear_tail_bits(char* bitmap, int64_t n) {  // the bits past row n - 1 of its last byte
  if (n & 7) bitmap[n >> 3] = (char)((uint8_t)bitmap[n >> 3] & (uint8_t)((1u << (n & 7)) - 1u));
}


inline dq_status payload(const dq_host_column* cols, int32_t n_cols, int64_t* value_bytes) {
  const char* me = "dq_upload_payload";
  if (n_cols < 0 || (n_cols > 0 && (!cols || !value_bytes))) return set_error(DQ_E_INVALID, "%s: bad argument", me);
  for (int32_t c = 0; c < n_cols; ++c) {
    if (dq_status s = check_column(me, c, cols[c])) return s;
    value_bytes[c] = cols[c].value_bytes;
    if (is_string(cols[c].type))
      if (dq_status s = string_payload(me, c, cols[c], &value_bytes[c])) return s;
  }
  return DQ_OK;
}

inline dq_status stage(const dq_host_column* cols, int32_t n_cols, const dq_upload_dest* dests, void* staging,
                          int64_t staging_bytes, int32_t host_threads, int64_t* positions, int64_t* staged_bytes) {
  const char* me = "dq_upload_to";
  if (n_cols < 0 || staging_bytes < 0 || (n_cols > 0 && (!cols || !dests || !positions)) || !staged_bytes ||
      (staging_bytes > 0 && !staging))
    return set_error(DQ_E_INVALID, "%s: bad argument", me);
  char* const stage = static_cast<char*>(staging);
  const int threads = host_threads > 0 ? host_threads : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  // the layout: every destination buffer's whole image, 256-byte aligned, in column order (values, validity, offsets)
  std::vector<int64_t> payload((size_t)std::max(1, n_cols));
  int64_t at = 0;
  for (int32_t c = 0; c < n_cols; ++c) {
    const dq_host_column& h = cols[c];
    const dq_upload_dest& d = dests[c];
    if (dq_status s = check_column(me, c, h)) return s;
    payload[(size_t)c] = h.value_bytes;
    if (is_string(h.type))
      if (dq_status s = string_payload(me, c, h, &payload[(size_t)c])) return s;
    const int64_t n = h.n_rows;
    const int64_t need[3] = {payload[(size_t)c], d.validity ? (n + 7) / 8 : 0,
                             is_string(h.type) ? (n + 1) * (h.type == DQ_TYPE_UTF8 ? 4 : 8) : 0};
    const void* ptr[3] = {d.values, d.validity, d.offsets};
    const int64_t len[3] = {d.value_bytes, d.validity_bytes, d.offset_bytes};
    for (int k = 0; k < 3; ++k) {
      positions[3 * (size_t)c + k] = -1;
      if (len[k] < 0 || (ptr[k] ? len[k] < need[k] : need[k] > 0 && k != 1))
        return set_error(DQ_E_INVALID, "%s: column %d: destination buffer %d holds %lld bytes, the rows need %lld", me, c,
                         k, (long long)(ptr[k] ? len[k] : 0), (long long)need[k]);
      if (!ptr[k] || len[k] == 0) continue;
      positions[3 * (size_t)c + k] = at;
      at = align_up(at + len[k]);
    }
    if (!d.validity && h.validity)  // a column declared without NULLs must have none
      for (int64_t r = 0; r < n; ++r)
        if (!row_valid(h, r))
          return set_error(DQ_E_INVALID, "%s: column %d: NULL at row %lld of a column declared non-nullable", me, c,
                           (long long)r);
  }
  if (at > staging_bytes)
    return set_error(DQ_E_INVALID, "%s: chunk needs %lld bytes, slot holds %lld", me, (long long)at, (long long)staging_bytes);
  std::vector<std::atomic<int64_t>> bad((size_t)std::max(1, n_cols));
  for (auto& b : bad) b.store(INT64_MAX);
  std::vector<Piece> pieces;
  for (int32_t c = 0; c < n_cols; ++c) {
    const dq_host_column& h = cols[c];
    const dq_upload_dest& d = dests[c];
    const int64_t n = h.n_rows;
    const int64_t* pos = &positions[3 * (size_t)c];
    const int64_t vbytes = (n + 7) / 8;
    // the padding behind the rows of every buffer (a buffer the pieces do not fill at all is cleared whole)
    if (pos[0] >= 0) std::memset(stage + pos[0] + payload[(size_t)c], 0, (size_t)(d.value_bytes - payload[(size_t)c]));
    if (pos[1] >= 0) std::memset(stage + pos[1] + vbytes, 0, (size_t)(d.validity_bytes - vbytes));
    if (pos[2] >= 0) std::memset(stage + pos[2], 0, (size_t)d.offset_bytes);
    if (n == 0) continue;
    if (pos[1] >= 0) {
      if (!h.validity) {  // nullable, no bitmap: every row valid
        std::memset(stage + pos[1], 0xFF, (size_t)vbytes);
      } else {
        Piece p{stage + pos[1], reinterpret_cast<const char*>(h.validity), vbytes};
        if (h.validity_bit) {
          p.kind = 3;
          p.shift = h.validity_bit;
          p.src_bytes = (h.validity_bit + n + 7) / 8;
        }
        pieces.push_back(p);
      }
    }
    if (is_string(h.type)) {
      const int64_t w = h.type == DQ_TYPE_UTF8 ? 4 : 8;
      if (payload[(size_t)c] == h.value_bytes) {  // no bytes under a NULL row: the data as it is, the offsets rebased
        if (h.value_bytes) pieces.push_back(Piece{stage + pos[0], static_cast<const char*>(h.values), h.value_bytes});
        Piece p{stage + pos[2], static_cast<const char*>(h.offsets), (n + 1) * w};
        if (h.offset_base) {
          p.kind = w == 4 ? 1 : 2;
          p.base = h.offset_base;
        }
        pieces.push_back(p);
      } else {  // drop the bytes under NULL rows: rows are copied one by one (string_payload checked the offsets)
        char* out = stage + pos[0];
        char* offs = stage + pos[2];
        int64_t kept = 0;
        for (int64_t r = 0; r < n; ++r) {
          const int64_t o0 = offset_at(h, r), o1 = offset_at(h, r + 1);
          if (row_valid(h, r) && o1 > o0) {
            std::memcpy(out + kept, static_cast<const char*>(h.values) + (o0 - h.offset_base), (size_t)(o1 - o0));
            kept += o1 - o0;
          }
          if (w == 4) {
            const int32_t v = (int32_t)kept;
            std::memcpy(offs + 4 * (r + 1), &v, 4);
          } else {
            std::memcpy(offs + 8 * (r + 1), &kept, 8);
          }
        }
      }
      continue;
    }
    Piece p{stage + pos[0], static_cast<const char*>(h.values), h.value_bytes};
    if (h.type == DQ_TYPE_DICT_UTF8) {
      p.kind = 4;
      p.idx_type = h.reserved;
      p.n_entries = h.offset_base;
      p.valid = h.validity;
      p.valid_bit = h.validity_bit;
      p.bad = &bad[(size_t)c];
    } else if (h.type == DQ_TYPE_BOOL) {
      if (h.validity_bit) {
        p.kind = 3;
        p.shift = h.validity_bit;
        p.src_bytes = (h.validity_bit + n + 7) / 8;
      }
    } else if (is_decimal(h.type) || h.validity) {
      p.kind = is_decimal(h.type) ? 6 : 5;
      p.width = (int)value_width(h.type);
      p.precision = DQ_DECIMAL_PRECISION(h.type);
      p.valid = h.validity;
      p.valid_bit = h.validity_bit;
      p.bad = &bad[(size_t)c];
    }
    pieces.push_back(p);
  }
  parallel_copy(pieces, threads);
  for (int32_t c = 0; c < n_cols; ++c) {
    const dq_host_column& h = cols[c];
    const int64_t n = h.n_rows;
    const int64_t* pos = &positions[3 * (size_t)c];
    if (n == 0) continue;
    if (pos[1] >= 0) clear_tail_bits(stage + pos[1], n);
    if (h.type == DQ_TYPE_BOOL) {  // a NULL row's value is false
      clear_tail_bits(stage + pos[0], n);
      if (pos[1] >= 0 && h.validity)
        for (int64_t i = 0; i < (n + 7) / 8; ++i) stage[pos[0] + i] = (char)(stage[pos[0] + i] & stage[pos[1] + i]);
    }
    const int64_t r = bad[(size_t)c].load();
    if (r == INT64_MAX) continue;
    if (h.type == DQ_TYPE_DICT_UTF8) {  // an index outside its dictionary: nothing is uploaded
      int64_t v = 0;
      (void)widen_check(h.reserved, h.values, r, r + 1, h.validity, h.validity_bit, h.offset_base, nullptr, &v);
      return set_error(DQ_E_INVALID, "%s: column %d: dictionary index %lld at row %lld is outside the dictionary's "
                       "%lld entries", me, c, (long long)v, (long long)r, (long long)h.offset_base);
    }
    return set_error(DQ_E_INVALID, "%s: column %d: the unscaled value at row %lld exceeds the precision of decimal(%d,%d)",
                     me, c, (long long)r, DQ_DECIMAL_PRECISION(h.type), DQ_DECIMAL_SCALE(h.type));
  }
  *staged_bytes = at;
  return DQ_OK;
}


}  // namespace up
}  // namespace dq
