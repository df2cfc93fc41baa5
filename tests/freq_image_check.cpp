// freq_image_check.cpp -- the frequency-table image parser (deequ_amd/csrc/dq_freq_image.cpp) against valid and
// corrupted images, built for the CPU alone with ASan + UBSan (tests/test_freq_image_host.py).  Every image is
// parsed from a heap buffer of exactly its length, so a read outside [bytes, bytes + n) is a sanitizer report.
// Prints one line per failed expectation and "ok <checks>" at the end; exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "dq_freq_image.h"

using dq::FreqImageView;

static int g_checks = 0, g_failed = 0;

static dq_status parse(const std::vector<uint8_t>& img, FreqImageView* v, std::string* msg = nullptr) {
  // an exact-size heap copy (an empty image still gets a valid pointer)
  uint8_t* p = new uint8_t[img.size() ? img.size() : 1];
  if (!img.empty()) std::memcpy(p, img.data(), img.size());
  char err[256] = "";
  const dq_status s = dq::freq_image_parse(p, (int64_t)img.size(), v, err, sizeof(err));
  delete[] p;
  if (msg) *msg = err;
  return s;
}

static void expect(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    ++g_failed;
    std::printf("FAILED: %s\n", what);
  }
}

struct Writer {
  std::vector<uint8_t> b;
  void raw(const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
  void u32(uint32_t v) { raw(&v, 4); }
  void u64(uint64_t v) { raw(&v, 8); }
  void pad8() { while (b.size() % 8) b.push_back(0); }
};

// a hashed table over (utf8, i32, decimal(20,4)) with three groups, and where its sections lie
struct Sample {
  std::vector<uint8_t> img;
  size_t types, hashed, n_groups, n_values, keys, counts, keys2, str_bytes_len, str_offsets, str_bytes, i32s, decs;
};
static Sample sample() {
  Sample s;
  Writer w;
  w.raw("DQFT", 4);
  w.u32(1);
  w.u32(0x01020304u);
  w.u32(3);
  s.types = w.b.size();
  w.u32(DQ_TYPE_UTF8);
  w.u32(DQ_TYPE_I32);
  w.u32(DQ_DECIMAL128(20, 4));
  w.u32(0);  // padding: n_cols is odd
  s.hashed = w.b.size();
  w.u32(1);
  w.u32(0);
  s.n_groups = w.b.size();
  w.u64(3);
  s.n_values = w.b.size();
  w.u64(2 + 1 + 7);
  s.keys = w.b.size();
  for (uint64_t k : {5ull, 9ull, 0xFFFFFFFFFFFFFFF0ull}) w.u64(k);
  s.counts = w.b.size();
  for (uint64_t c : {2ull, 1ull, 7ull}) w.u64(c);
  s.keys2 = w.b.size();
  for (uint64_t k : {77ull, 3ull, 12ull}) w.u64(k);
  const char* bytes = "abcdefghijklm";  // 13 bytes: "abc", "", "defghijklm"
  s.str_bytes_len = w.b.size();
  w.u64(13);
  s.str_offsets = w.b.size();
  for (uint64_t o : {0ull, 3ull, 3ull, 13ull}) w.u64(o);
  s.str_bytes = w.b.size();
  w.raw(bytes, 13);
  w.pad8();
  s.i32s = w.b.size();
  for (uint32_t v : {1u, 2u, 3u}) w.u32(v);
  w.pad8();
  s.decs = w.b.size();
  for (int i = 0; i < 6; ++i) w.u64(100 + i);
  s.img = w.b;
  return s;
}

// an unhashed table over one i64 column (no store) with two groups
static std::vector<uint8_t> sample_unhashed(uint32_t type = DQ_TYPE_I64) {
  Writer w;
  w.raw("DQFT", 4);
  w.u32(1);
  w.u32(0x01020304u);
  w.u32(1);
  w.u32(type);
  w.u32(0);
  w.u32(0);
  w.u32(0);
  w.u64(2);
  w.u64(5);
  w.u64(1);
  w.u64(2);
  w.u64(4);
  w.u64(1);
  return w.b;
}

static void put64(std::vector<uint8_t>& b, size_t at, uint64_t v) { std::memcpy(b.data() + at, &v, 8); }
static void put32(std::vector<uint8_t>& b, size_t at, uint32_t v) { std::memcpy(b.data() + at, &v, 4); }

int main() {
  const Sample s = sample();
  FreqImageView v;
  std::string msg;
  expect(parse(s.img, &v, &msg) == DQ_OK, "the valid hashed image parses");
  if (!msg.empty()) std::printf("  (%s)\n", msg.c_str());
  expect(v.n_cols == 3 && v.hashed == 1 && v.n_groups == 3 && v.n_values == 10, "header fields");
  expect(v.types[0] == DQ_TYPE_UTF8 && v.types[1] == DQ_TYPE_I32 && v.types[2] == DQ_DECIMAL128(20, 4), "types");
  expect((size_t)v.keys == s.keys && (size_t)v.counts == s.counts && (size_t)v.keys2 == s.keys2, "key / count sections");
  expect((size_t)v.col_offsets[0] == s.str_offsets && (size_t)v.col_values[0] == s.str_bytes && v.col_bytes[0] == 13,
         "string section");
  expect((size_t)v.col_values[1] == s.i32s && v.col_bytes[1] == 12, "i32 section");
  expect((size_t)v.col_values[2] == s.decs && v.col_bytes[2] == 48, "decimal section");
  expect(parse(sample_unhashed(), &v) == DQ_OK && v.hashed == 0 && v.n_groups == 2 && v.keys2 == 0, "the valid unhashed image parses");

  // every truncation length, 0 .. size - 1, of both images; and bytes appended
  for (size_t n = 0; n < s.img.size(); ++n)
    expect(parse(std::vector<uint8_t>(s.img.begin(), s.img.begin() + n), &v) == DQ_E_STATE, "a truncated hashed image");
  const std::vector<uint8_t> un = sample_unhashed();
  for (size_t n = 0; n < un.size(); ++n)
    expect(parse(std::vector<uint8_t>(un.begin(), un.begin() + n), &v) == DQ_E_STATE, "a truncated unhashed image");
  {
    std::vector<uint8_t> b = s.img;
    b.resize(b.size() + 8, 0);
    expect(parse(b, &v) == DQ_E_STATE, "bytes after the last section");
  }

  struct Case { const char* what; std::function<void(std::vector<uint8_t>&)> edit; };
  const Case cases[] = {
      {"wrong magic", [&](std::vector<uint8_t>& b) { b[0] = 'X'; }},
      {"wrong version", [&](std::vector<uint8_t>& b) { put32(b, 4, 2); }},
      {"the other byte order", [&](std::vector<uint8_t>& b) { put32(b, 8, 0x04030201u); }},
      {"n_cols = 0", [&](std::vector<uint8_t>& b) { put32(b, 12, 0); }},
      {"n_cols = 9", [&](std::vector<uint8_t>& b) { put32(b, 12, 9); }},
      {"n_cols negative", [&](std::vector<uint8_t>& b) { put32(b, 12, 0x80000000u); }},
      {"type code 0", [&](std::vector<uint8_t>& b) { put32(b, s.types, 0); }},
      {"type code 13", [&](std::vector<uint8_t>& b) { put32(b, s.types + 4, 13); }},
      {"decimal precision 39", [&](std::vector<uint8_t>& b) { put32(b, s.types + 8, DQ_DECIMAL128(39, 4)); }},
      {"decimal scale above precision", [&](std::vector<uint8_t>& b) { put32(b, s.types + 8, DQ_DECIMAL128(5, 6)); }},
      {"type code with high bits", [&](std::vector<uint8_t>& b) { put32(b, s.types + 4, DQ_TYPE_I32 | 0x01000000); }},
      {"hashed flag 2", [&](std::vector<uint8_t>& b) { put32(b, s.hashed, 2); }},
      {"unhashed over three columns", [&](std::vector<uint8_t>& b) { put32(b, s.hashed, 0); }},
      {"n_groups = 2^31", [&](std::vector<uint8_t>& b) { put64(b, s.n_groups, 1ull << 31); }},
      {"n_groups = 2^63 (sizes overflow)", [&](std::vector<uint8_t>& b) { put64(b, s.n_groups, 1ull << 63); }},
      {"n_groups = 2^61 (sizes overflow)", [&](std::vector<uint8_t>& b) { put64(b, s.n_groups, 1ull << 61); }},
      {"n_groups beyond the image", [&](std::vector<uint8_t>& b) { put64(b, s.n_groups, 1000); }},
      {"n_groups one too many", [&](std::vector<uint8_t>& b) { put64(b, s.n_groups, 4); }},
      {"n_groups one too few", [&](std::vector<uint8_t>& b) { put64(b, s.n_groups, 2); }},
      {"n_values negative", [&](std::vector<uint8_t>& b) { put64(b, s.n_values, ~0ull); }},
      {"equal keys", [&](std::vector<uint8_t>& b) { put64(b, s.keys + 8, 5); }},
      {"descending keys", [&](std::vector<uint8_t>& b) { put64(b, s.keys + 16, 6); }},
      {"count 0", [&](std::vector<uint8_t>& b) { put64(b, s.counts, 0); put64(b, s.counts + 8, 3); }},
      {"count negative", [&](std::vector<uint8_t>& b) { put64(b, s.counts + 8, (uint64_t)-1); }},
      {"count sum above n_values", [&](std::vector<uint8_t>& b) { put64(b, s.counts + 16, 8); }},
      {"count sum below n_values", [&](std::vector<uint8_t>& b) { put64(b, s.counts + 16, 6); }},
      {"count sum wraps to n_values", [&](std::vector<uint8_t>& b) {
         put64(b, s.counts, 0x7FFFFFFFFFFFFFFFull); put64(b, s.counts + 8, 0x7FFFFFFFFFFFFFFFull); put64(b, s.counts + 16, 12); }},
      {"offsets do not start at 0", [&](std::vector<uint8_t>& b) { put64(b, s.str_offsets, 1); }},
      {"offsets decrease", [&](std::vector<uint8_t>& b) { put64(b, s.str_offsets + 8, 4); }},
      {"offsets negative", [&](std::vector<uint8_t>& b) { put64(b, s.str_offsets + 8, (uint64_t)-5); }},
      {"offsets end before the byte length", [&](std::vector<uint8_t>& b) { put64(b, s.str_offsets + 24, 12); }},
      {"offsets end after the byte length", [&](std::vector<uint8_t>& b) { put64(b, s.str_offsets + 24, 14); }},
      {"byte length beyond the image", [&](std::vector<uint8_t>& b) { put64(b, s.str_bytes_len, 1000); put64(b, s.str_offsets + 24, 1000); }},
      {"byte length 2^63 - 1 (padding overflows)", [&](std::vector<uint8_t>& b) {
         put64(b, s.str_bytes_len, 0x7FFFFFFFFFFFFFFFull); put64(b, s.str_offsets + 24, 0x7FFFFFFFFFFFFFFFull); }},
      {"byte length shifts the later sections", [&](std::vector<uint8_t>& b) { put64(b, s.str_bytes_len, 21); put64(b, s.str_offsets + 24, 21); }},
  };
  for (const Case& c : cases) {
    std::vector<uint8_t> b = s.img;
    c.edit(b);
    msg.clear();
    const dq_status st = parse(b, &v, &msg);
    expect(st == DQ_E_STATE && !msg.empty(), c.what);
  }
  expect(parse(sample_unhashed(DQ_TYPE_UTF8), &v) == DQ_E_STATE, "unhashed over a string column");
  expect(parse(sample_unhashed(DQ_DECIMAL128(10, 2)), &v) == DQ_E_STATE, "unhashed over a decimal column");
  expect(dq::freq_image_parse(nullptr, 0, &v, nullptr, 0) == DQ_E_STATE, "no bytes");
  {
    // a misaligned image (the parser reads by memcpy) and a NULL message buffer
    std::vector<uint8_t> b(s.img.size() + 1);
    std::memcpy(b.data() + 1, s.img.data(), s.img.size());
    expect(dq::freq_image_parse(b.data() + 1, (int64_t)s.img.size(), &v, nullptr, 0) == DQ_OK, "a misaligned image parses");
  }
  if (g_failed) return 1;
  std::printf("ok %d\n", g_checks);
  return 0;
}
