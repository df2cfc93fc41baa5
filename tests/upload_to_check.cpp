// upload_to_check.cpp -- the host half of dq_upload_to (deequ_amd/csrc/dq_upload_host.cpp: dq_upload_payload /
// dq_upload_stage, no HIP) under host ASan + UBSan: a stand-alone program (its own main, the library's set_error
// restated here), built with g++ by tests/test_arrow_table_host.py.  Every source array and the staging buffer live in
// heap blocks of exactly their size, so a read or write past one is a sanitizer report; every image is compared with a
// row-by-row restatement.  No device is touched.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/dqscan.h"

namespace dq {
static char g_msg[512];
dq_status set_error(dq_status code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace dq

static int g_fail = 0;
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, dq::g_msg); \
      ++g_fail;                                                                  \
    }                                                                            \
  } while (0)

static uint64_t g_rng = 88172645463325252ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

static char* heap(const std::vector<uint8_t>& v) {  // a block of exactly v's bytes
  char* p = static_cast<char*>(std::malloc(v.size() + (v.empty() ? 1 : 0)));
  if (!v.empty()) std::memcpy(p, v.data(), v.size());
  return p;
}

static int64_t padded(int64_t n) { return (n + 15) / 16 * 16 + 16; }
static int64_t bitmap_bytes(int64_t n) { return ((n + 7) / 8 + 7) / 8 * 8 + 8; }

static bool bit_at(const std::vector<uint8_t>& bm, int64_t i) { return (bm[(size_t)(i >> 3)] >> (i & 7)) & 1; }

// A source bitmap of `bit` + n random bits (the bits before row 0 and past the last row are random too).
static std::vector<uint8_t> random_bits(int64_t bit, int64_t n) {
  std::vector<uint8_t> v((size_t)((bit + n + 7) / 8));
  for (auto& b : v) b = (uint8_t)rnd();
  return v;
}

struct Staged {
  std::vector<char> values, validity, offsets;
  dq_status status;
};

static Staged stage_one(const dq_host_column& h, bool nullable, int threads) {
  Staged out{};
  int64_t payload = 0;
  out.status = dq_upload_payload(&h, 1, &payload);
  if (out.status != DQ_OK) return out;
  const bool str = h.type == DQ_TYPE_UTF8 || h.type == DQ_TYPE_LARGE_UTF8;
  dq_upload_dest d{};
  char tag = 0;
  d.values = &tag;
  d.value_bytes = padded(h.type == DQ_TYPE_BOOL ? bitmap_bytes(h.n_rows) : payload);
  if (nullable) d.validity = &tag, d.validity_bytes = bitmap_bytes(h.n_rows);
  if (str) d.offsets = &tag, d.offset_bytes = padded((h.n_rows + 1) * (h.type == DQ_TYPE_UTF8 ? 4 : 8));
  auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
  const int64_t size = up(d.value_bytes) + up(d.validity_bytes) + up(d.offset_bytes);
  char* stage = static_cast<char*>(std::malloc((size_t)size));
  std::memset(stage, 0xA5, (size_t)size);
  int64_t pos[3], used = 0;
  out.status = dq_upload_stage(&h, 1, &d, stage, size, threads, pos, &used);
  if (out.status == DQ_OK) {
    CHECK(used <= size);
    out.values.assign(stage + pos[0], stage + pos[0] + d.value_bytes);
    if (pos[1] >= 0) out.validity.assign(stage + pos[1], stage + pos[1] + d.validity_bytes);
    if (pos[2] >= 0) out.offsets.assign(stage + pos[2], stage + pos[2] + d.offset_bytes);
  }
  std::free(stage);
  return out;
}

static void check_bitmap(const std::vector<char>& got, const std::vector<uint8_t>& src, int64_t bit, int64_t n) {
  CHECK((int64_t)got.size() == bitmap_bytes(n));
  for (int64_t i = 0; i < (int64_t)got.size() * 8; ++i) {
    const bool g = ((uint8_t)got[(size_t)(i >> 3)] >> (i & 7)) & 1;
    if (g != (i < n && bit_at(src, bit + i))) {
      CHECK(!"bitmap bit");
      return;
    }
  }
}

template <typename T>
static void fixed_case(int32_t type, int64_t bit, int64_t n, int threads) {
  std::vector<uint8_t> valid = random_bits(bit, n), raw((size_t)(n * (int64_t)sizeof(T)));
  for (auto& b : raw) b = (uint8_t)(rnd() | 1);
  char* v = heap(raw);
  char* bm = heap(valid);
  dq_host_column h{};
  h.type = type; h.nullable = 1; h.n_rows = n; h.values = v; h.value_bytes = (int64_t)raw.size();
  h.validity = reinterpret_cast<const uint8_t*>(bm); h.validity_bytes = (n + 7) / 8; h.validity_bit = (int32_t)bit;
  if (n == 0) h.values = nullptr, h.validity = nullptr, h.validity_bytes = 0;
  Staged s = stage_one(h, true, threads);
  CHECK(s.status == DQ_OK);
  if (s.status == DQ_OK) {
    CHECK((int64_t)s.values.size() == padded(n * (int64_t)sizeof(T)));
    for (int64_t i = 0; i < (int64_t)s.values.size(); ++i) {
      const int64_t r = i / (int64_t)sizeof(T);
      const char want = r < n && bit_at(valid, bit + r) ? (char)raw[(size_t)i] : (char)0;
      if (s.values[(size_t)i] != want) {
        CHECK(!"fixed-width value byte");
        break;
      }
    }
    if (n) check_bitmap(s.validity, valid, bit, n);
  }
  std::free(v);
  std::free(bm);
}

static void bool_case(int64_t bit, int64_t n) {
  std::vector<uint8_t> valid = random_bits(bit, n), vals = random_bits(bit, n);
  char* v = heap(vals);
  char* bm = heap(valid);
  dq_host_column h{};
  h.type = DQ_TYPE_BOOL; h.nullable = 1; h.n_rows = n; h.values = v; h.value_bytes = (n + 7) / 8;
  h.validity = reinterpret_cast<const uint8_t*>(bm); h.validity_bytes = (n + 7) / 8; h.validity_bit = (int32_t)bit;
  if (n == 0) h.values = nullptr, h.validity = nullptr, h.validity_bytes = 0;
  Staged s = stage_one(h, true, 2);
  CHECK(s.status == DQ_OK && (int64_t)s.values.size() == padded(bitmap_bytes(n)));
  if (s.status == DQ_OK) {
    for (int64_t i = 0; i < (int64_t)s.values.size() * 8; ++i) {
      const bool g = ((uint8_t)s.values[(size_t)(i >> 3)] >> (i & 7)) & 1;
      if (g != (i < n && bit_at(vals, bit + i) && bit_at(valid, bit + i))) {
        CHECK(!"boolean value bit");
        break;
      }
    }
    if (n) check_bitmap(s.validity, valid, bit, n);
  }
  std::free(v);
  std::free(bm);
}

template <typename O>
static void string_case(int32_t type, int64_t bit, int64_t n, int64_t first) {
  // `first` rows lie before the slice; lengths 0..5; NULL slots keep their bytes
  std::vector<uint8_t> valid = random_bits(bit, n);
  std::vector<O> offs((size_t)(first + n + 1));
  offs[0] = 0;
  for (size_t r = 1; r < offs.size(); ++r) offs[r] = offs[r - 1] + (O)(rnd() % 6);
  std::vector<uint8_t> data((size_t)offs.back());
  for (auto& b : data) b = (uint8_t)('a' + rnd() % 26);
  std::vector<uint8_t> ob(offs.size() * sizeof(O));
  std::memcpy(ob.data(), offs.data(), ob.size());
  char* o = heap(ob);
  char* d = heap(data);
  char* bm = heap(valid);
  dq_host_column h{};
  h.type = type; h.nullable = 1; h.n_rows = n;
  h.offsets = o + first * (int64_t)sizeof(O); h.offset_bytes = (n + 1) * (int64_t)sizeof(O);
  h.offset_base = offs[(size_t)first];
  h.value_bytes = offs[(size_t)(first + n)] - offs[(size_t)first];
  h.values = h.value_bytes ? d + offs[(size_t)first] : nullptr;
  h.validity = reinterpret_cast<const uint8_t*>(bm); h.validity_bytes = (n + 7) / 8; h.validity_bit = (int32_t)bit;
  if (n == 0) h.offsets = nullptr, h.offset_bytes = 0, h.validity = nullptr, h.validity_bytes = 0, h.offset_base = 0;
  Staged s = stage_one(h, true, 2);
  CHECK(s.status == DQ_OK);
  if (s.status == DQ_OK) {
    std::vector<char> want_data;
    std::vector<O> want_offs((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
      if (bit_at(valid, bit + r))
        want_data.insert(want_data.end(), data.begin() + offs[(size_t)(first + r)], data.begin() + offs[(size_t)(first + r + 1)]);
      want_offs[(size_t)r + 1] = (O)want_data.size();
    }
    CHECK((int64_t)s.values.size() == padded((int64_t)want_data.size()));
    CHECK((int64_t)s.offsets.size() == padded((n + 1) * (int64_t)sizeof(O)));
    CHECK(want_data.empty() || std::memcmp(s.values.data(), want_data.data(), want_data.size()) == 0);
    for (size_t i = want_data.size(); i < s.values.size(); ++i) CHECK(s.values[i] == 0);
    CHECK(std::memcmp(s.offsets.data(), want_offs.data(), want_offs.size() * sizeof(O)) == 0);
    for (size_t i = want_offs.size() * sizeof(O); i < s.offsets.size(); ++i) CHECK(s.offsets[i] == 0);
    if (n) check_bitmap(s.validity, valid, bit, n);
  }
  std::free(o);
  std::free(d);
  std::free(bm);
}

template <typename T>
static void index_case(int32_t code, int64_t bit, int64_t n) {
  const int64_t entries = 100;
  std::vector<uint8_t> valid = random_bits(bit, n), raw((size_t)(n * (int64_t)sizeof(T)));
  std::vector<T> idx((size_t)n);
  for (int64_t r = 0; r < n; ++r) idx[(size_t)r] = bit_at(valid, bit + r) ? (T)(rnd() % entries) : (T)120;  // NULL: out of range
  if (n) std::memcpy(raw.data(), idx.data(), raw.size());
  char* v = heap(raw);
  char* bm = heap(valid);
  dq_host_column h{};
  h.type = DQ_TYPE_DICT_UTF8; h.nullable = 1; h.n_rows = n; h.values = v; h.value_bytes = 4 * n; h.reserved = code;
  h.offset_base = entries;
  h.validity = reinterpret_cast<const uint8_t*>(bm); h.validity_bytes = (n + 7) / 8; h.validity_bit = (int32_t)bit;
  if (n == 0) h.values = nullptr, h.validity = nullptr, h.validity_bytes = 0;
  Staged s = stage_one(h, true, 2);
  CHECK(s.status == DQ_OK && (int64_t)s.values.size() == padded(4 * n));
  if (s.status == DQ_OK) {
    for (int64_t r = 0; r < (int64_t)s.values.size() / 4; ++r) {
      int32_t g;
      std::memcpy(&g, s.values.data() + 4 * r, 4);
      CHECK(g == (r < n && bit_at(valid, bit + r) ? (int32_t)idx[(size_t)r] : 0));
    }
  }
  // the first valid row out of range: refused, naming it
  for (int64_t r = 0; r < n; ++r) {
    if (!bit_at(valid, bit + r)) continue;
    const T bad = (T)100;
    std::memcpy(v + r * (int64_t)sizeof(T), &bad, sizeof(T));
    Staged t = stage_one(h, true, 2);
    char want[64];
    std::snprintf(want, sizeof want, "index 100 at row %lld ", (long long)r);
    CHECK(t.status == DQ_E_INVALID && std::strstr(dq::g_msg, want));
    break;
  }
  std::free(v);
  std::free(bm);
}

static void put128(std::vector<uint8_t>& raw, int64_t r, __int128 u) { std::memcpy(raw.data() + 16 * r, &u, 16); }

static void decimal_case(int p, int64_t n, int threads) {
  __int128 lim = 1;
  for (int k = 0; k < p; ++k) lim *= 10;
  std::vector<uint8_t> raw((size_t)(16 * n)), valid = random_bits(0, n);
  for (int64_t r = 0; r < n; ++r) {
    const __int128 u = r % 3 == 0 ? lim - 1 : r % 3 == 1 ? -(lim - 1) : (__int128)(int32_t)rnd() % lim;
    put128(raw, r, bit_at(valid, r) ? u : lim * (r % 2 ? 1 : -1));  // NULL slots hold values out of range
  }
  char* v = heap(raw);
  char* bm = heap(valid);
  dq_host_column h{};
  h.type = DQ_DECIMAL128(p, 0); h.nullable = 1; h.n_rows = n; h.values = v; h.value_bytes = 16 * n;
  h.validity = reinterpret_cast<const uint8_t*>(bm); h.validity_bytes = (n + 7) / 8;
  Staged s = stage_one(h, true, threads);
  CHECK(s.status == DQ_OK);
  if (s.status == DQ_OK)
    for (int64_t r = 0; r < n; ++r) {
      static const char zero[16] = {0};
      if (std::memcmp(s.values.data() + 16 * r, bit_at(valid, r) ? v + 16 * r : zero, 16) != 0) {
        CHECK(!"decimal value");
        break;
      }
    }
  // +-10^p at the last valid row, then also at the first: the lowest row is named
  int64_t lo = -1, hi = -1;
  for (int64_t r = 0; r < n; ++r)
    if (bit_at(valid, r)) {
      if (lo < 0) lo = r;
      hi = r;
    }
  if (hi >= 0) {
    for (int sign : {1, -1}) {
      for (int64_t row : {hi, lo}) {
        const __int128 bad = lim * sign;
        std::memcpy(v + 16 * row, &bad, 16);
        Staged t = stage_one(h, true, threads);
        char want[64];
        std::snprintf(want, sizeof want, "row %lld ", (long long)row);
        CHECK(t.status == DQ_E_INVALID && std::strstr(dq::g_msg, want));
      }
      const __int128 fine = (lim - 1) * sign;
      std::memcpy(v + 16 * hi, &fine, 16);
      std::memcpy(v + 16 * lo, &fine, 16);
      CHECK(stage_one(h, true, threads).status == DQ_OK);
    }
  }
  std::free(v);
  std::free(bm);
}

int main() {
  const int64_t rows[] = {0, 1, 7, 8, 9, 63, 64, 65, 1000};
  const int64_t bits[] = {0, 1, 7, 8 % 8, 13 % 8};  // (a row offset of 8 / 13: the byte part is in the pointer)
  for (int64_t n : rows)
    for (int64_t bit : bits) {
      fixed_case<int8_t>(DQ_TYPE_I8, bit, n, 2);
      fixed_case<int16_t>(DQ_TYPE_I16, bit, n, 2);
      fixed_case<int32_t>(DQ_TYPE_DATE32, bit, n, 2);
      fixed_case<double>(DQ_TYPE_F64, bit, n, 2);
      bool_case(bit, n);
      string_case<int32_t>(DQ_TYPE_UTF8, bit, n, 0);
      string_case<int32_t>(DQ_TYPE_UTF8, bit, n, 11);
      string_case<int64_t>(DQ_TYPE_LARGE_UTF8, bit, n, 5);
      index_case<int8_t>(DQ_TYPE_I8, bit, n);
      index_case<int16_t>(DQ_TYPE_I16, bit, n);
      index_case<int32_t>(DQ_TYPE_I32, bit, n);
      index_case<uint8_t>(-DQ_TYPE_I8, bit, n);
      index_case<uint16_t>(-DQ_TYPE_I16, bit, n);
    }
  for (int p : {1, 18, 19, 38})
    for (int64_t n : {1, 9, 65, 1000}) decimal_case(p, n, 2);
  // large enough for the thread pool to split the pieces (shares end on 8 bytes: inside a 16-byte value)
  decimal_case(38, 1200001, 3);
  fixed_case<int64_t>(DQ_TYPE_I64, 5, 2500003, 3);
  {  // malformed host columns are refused, not read
    dq_host_column h{};
    int64_t payload = 0;
    h.type = DQ_TYPE_I32; h.n_rows = 4; h.value_bytes = 12;
    CHECK(dq_upload_payload(&h, 1, &payload) == DQ_E_INVALID);
    int32_t offs[3] = {0, 5, 3};
    char data[5] = {0};
    h = dq_host_column{};
    h.type = DQ_TYPE_UTF8; h.n_rows = 2; h.offsets = offs; h.offset_bytes = 12; h.values = data; h.value_bytes = 3;
    CHECK(dq_upload_payload(&h, 1, &payload) == DQ_E_INVALID);
    h.type = 99;
    CHECK(dq_upload_payload(&h, 1, &payload) == DQ_E_INVALID);
  }
  if (g_fail) return 1;
  std::printf("ok upload_to host half\n");
  return 0;
}
