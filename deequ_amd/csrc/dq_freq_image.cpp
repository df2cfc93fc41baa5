// dq_freq_image.cpp -- the checks of a frequency table's byte image (layout: dq_freq_image.h).  Host only, no HIP:
// every read goes through Reader, which never leaves [bytes, bytes + n).
#include "dq_freq_image.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace dq {
namespace {

dq_status bad(char* err, size_t cap, const char* fmt, ...) {
  if (err && cap) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(err, cap, fmt, ap);
    va_end(ap);
  }
  return DQ_E_STATE;
}

struct Reader {
  const uint8_t* p;
  int64_t n;
  // [at, at + len) lies inside the image (len >= 0; no overflow: both are below 2^62 where it is called)
  bool has(int64_t at, int64_t len) const { return at >= 0 && len >= 0 && at <= n && len <= n - at; }
  uint32_t u32(int64_t at) const { uint32_t v; std::memcpy(&v, p + at, 4); return v; }
  uint64_t u64(int64_t at) const { uint64_t v; std::memcpy(&v, p + at, 8); return v; }
};

constexpr int64_t kMaxGroups = (int64_t)1 << 31;

}  // namespace

dq_status freq_image_parse(const uint8_t* bytes, int64_t n, FreqImageView* view, char* err, size_t err_cap) {
  if (!bytes || !view || n < 0) return bad(err, err_cap, "frequency image: no bytes");
  const Reader r{bytes, n};
  *view = FreqImageView();
  if (!r.has(0, 16)) return bad(err, err_cap, "frequency image: truncated header (%lld bytes)", (long long)n);
  if (std::memcmp(bytes, "DQFT", 4) != 0) return bad(err, err_cap, "frequency image: wrong magic");
  if (r.u32(8) != kFreqImageOrder) return bad(err, err_cap, "frequency image: written in another byte order");
  if (r.u32(4) != kFreqImageVersion) return bad(err, err_cap, "frequency image: version %u, expected %u", r.u32(4), kFreqImageVersion);
  const int32_t n_cols = (int32_t)r.u32(12);
  if (n_cols < 1 || n_cols > kFreqImageMaxCols) return bad(err, err_cap, "frequency image: %d grouping columns", n_cols);
  const int64_t head = freq_image_header_bytes(n_cols);
  if (!r.has(0, head)) return bad(err, err_cap, "frequency image: truncated header (%lld bytes)", (long long)n);
  view->n_cols = n_cols;
  bool strings = false;
  for (int c = 0; c < n_cols; ++c) {
    const int32_t t = (int32_t)r.u32(16 + 4 * c);
    const int es = dq_freq_elem_size(t);
    if (es < 0) return bad(err, err_cap, "frequency image: column %d has unknown type code %d", c, t);
    strings = strings || es == 0 || es == 16;
    view->types[c] = t;
  }
  int64_t at = 16 + 4 * (int64_t)((n_cols + 1) & ~1);
  const uint32_t hashed = r.u32(at);
  if (hashed > 1) return bad(err, err_cap, "frequency image: hashed flag %u", hashed);
  if (!hashed && (n_cols != 1 || strings))
    return bad(err, err_cap, "frequency image: an unhashed table over strings, decimals or several columns");
  view->hashed = (int32_t)hashed;
  const uint64_t ng = r.u64(at + 8), nvals = r.u64(at + 16);
  if (ng >= (uint64_t)kMaxGroups) return bad(err, err_cap, "frequency image: %llu groups (at most 2^31 - 1)", (unsigned long long)ng);
  if (nvals > (uint64_t)INT64_MAX) return bad(err, err_cap, "frequency image: negative n_values");
  const int64_t G = (int64_t)ng;
  view->n_groups = G;
  view->n_values = (int64_t)nvals;
  at = head;
  // keys, counts, keys2: G < 2^31 entries of 8 bytes each
  const int n_arrays = hashed ? 3 : 2;
  if (!r.has(at, (int64_t)n_arrays * G * 8)) return bad(err, err_cap, "frequency image: truncated keys / counts");
  view->keys = at;
  view->counts = at + G * 8;
  view->keys2 = hashed ? at + 2 * G * 8 : 0;
  at += (int64_t)n_arrays * G * 8;
  uint64_t sum = 0;
  for (int64_t g = 0; g < G; ++g) {
    if (g > 0 && r.u64(view->keys + 8 * g) <= r.u64(view->keys + 8 * (g - 1)))
      return bad(err, err_cap, "frequency image: keys not strictly ascending at group %lld", (long long)g);
    const int64_t c = (int64_t)r.u64(view->counts + 8 * g);
    if (c < 1) return bad(err, err_cap, "frequency image: count %lld of group %lld", (long long)c, (long long)g);
    sum += (uint64_t)c;  // G < 2^31 counts below 2^63: a sum past n_values is caught before it can wrap twice
    if (sum > nvals) return bad(err, err_cap, "frequency image: counts add up to more than n_values");
  }
  if (sum != nvals) return bad(err, err_cap, "frequency image: counts add up to %llu, n_values is %llu",
                               (unsigned long long)sum, (unsigned long long)nvals);
  if (hashed) {
    for (int c = 0; c < n_cols; ++c) {
      const int es = dq_freq_elem_size(view->types[c]);
      if (es > 0) {
        const int64_t len = G * es;  // < 2^35
        if (!r.has(at, freq_image_pad8(len))) return bad(err, err_cap, "frequency image: truncated values of column %d", c);
        view->col_values[c] = at;
        view->col_bytes[c] = len;
        at += freq_image_pad8(len);
        continue;
      }
      if (!r.has(at, 8 + (G + 1) * 8)) return bad(err, err_cap, "frequency image: truncated offsets of column %d", c);
      const int64_t nbytes = (int64_t)r.u64(at);
      at += 8;
      view->col_offsets[c] = at;
      if (r.u64(at) != 0) return bad(err, err_cap, "frequency image: offsets of column %d do not start at 0", c);
      int64_t prev = 0;
      for (int64_t g = 1; g <= G; ++g) {
        const int64_t o = (int64_t)r.u64(at + 8 * g);
        if (o < prev) return bad(err, err_cap, "frequency image: offsets of column %d decrease at group %lld", c, (long long)g);
        prev = o;
      }
      at += (G + 1) * 8;
      if (prev != nbytes)
        return bad(err, err_cap, "frequency image: offsets of column %d end at %lld, its bytes at %lld", c, (long long)prev,
                   (long long)nbytes);
      // the byte length has to fit what is left (checked before it is padded: no overflow)
      if (!r.has(at, prev) || !r.has(at, freq_image_pad8(prev)))
        return bad(err, err_cap, "frequency image: string bytes of column %d (%lld) exceed the image", c, (long long)prev);
      view->col_values[c] = at;
      view->col_bytes[c] = prev;
      at += freq_image_pad8(prev);
    }
  }
  if (at != n) return bad(err, err_cap, "frequency image: %lld bytes, its sections end at %lld", (long long)n, (long long)at);
  return DQ_OK;
}

}  // namespace dq
