// schema_rules_check.cpp -- a stand-alone host driver of deequ_amd/csrc/dq_schema.h (the rules the verdict kernel
// runs), meant to be built with -fsanitize=address,undefined and run on a CPU (tests/test_schema_host.py does).
// Every value is copied into a heap buffer of exactly its size, so a read past its end is an ASan report.
//
// stdin, one request per line (hex = the value's bytes in hex, "-" for none):
//   I <hex>                       -> "N" | "V <int>"                      schema_to_int
//   D <p> <s> <hex>               -> "N" | "V <hi hex> <lo hex>"          schema_to_decimal
//   T <mask hex> <hex>            -> "U" (mask refused) | "N" | "V <us>"  schema_compile_mask + schema_parse_timestamp
//   C <hex>                       -> "V <count>"                          schema_char_count
//   R <seed> <count>              -> "R <checksum>": random byte strings (digits, signs, points, exponents, blanks
//                                    and arbitrary bytes) through every rule and a set of masks
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dq_schema.h"

#define DQ_DEC_TABLE static const
#include "dq_dec_tables.inc"

namespace {

std::vector<uint8_t> unhex(const char* p) {
  std::vector<uint8_t> out;
  const auto nib = [](char c) { return (unsigned)(c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10); };
  for (; p[0] && p[1] && p[0] != '-' && p[0] != '\n' && p[0] != ' '; p += 2) out.push_back((uint8_t)(nib(p[0]) << 4 | nib(p[1])));
  return out;
}

struct Exact {  // the value in a heap block of exactly its size
  uint8_t* p;
  int64_t n;
  explicit Exact(const std::vector<uint8_t>& v) : p(v.empty() ? nullptr : (uint8_t*)std::malloc(v.size())), n((int64_t)v.size()) {
    if (p) std::memcpy(p, v.data(), v.size());
  }
  ~Exact() { std::free(p); }
};

uint64_t rng_state;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 2685821237ull * 1000003ull) >> 33);
}

}  // namespace

int main() {
  const dq::DecTab t{kDecP10Lo, kDecP10Hi, kDecRcpHi, kDecRcpLo};
  static char line[1 << 20];
  while (std::fgets(line, sizeof line, stdin)) {
    const char kind = line[0];
    if (kind == 'I' || kind == 'C') {
      const Exact v(unhex(line + 2));
      dq::CastHostBytes rd{v.p};
      if (kind == 'C') {
        std::printf("V %" PRId64 "\n", dq::schema_char_count(rd, v.n));
        continue;
      }
      int32_t x = 0;
      if (dq::schema_to_int(rd, v.n, x)) std::printf("V %d\n", x);
      else std::printf("N\n");
    } else if (kind == 'D') {
      int p = 0, s = 0, used = 0;
      if (std::sscanf(line + 2, "%d %d %n", &p, &s, &used) < 2) return 2;
      const Exact v(unhex(line + 2 + used));
      dq::CastHostBytes rd{v.p};
      uint64_t lo = 0, hi = 0;
      if (dq::schema_to_decimal(rd, v.n, p, s, t, lo, hi)) std::printf("V %016" PRIx64 " %016" PRIx64 "\n", hi, lo);
      else std::printf("N\n");
    } else if (kind == 'T') {
      const std::vector<uint8_t> mb = unhex(line + 2);
      const std::string mask(mb.begin(), mb.end());
      const char* rest = std::strchr(line + 2, ' ');
      const Exact v(unhex(rest ? rest + 1 : "-"));
      dq::SchemaMaskEl els[dq::kSchemaMaxMask];
      const char* why = nullptr;
      const int n = dq::schema_compile_mask(mask.c_str(), els, &why);
      if (n < 0) {
        std::printf("U\n");
        continue;
      }
      dq::CastHostBytes rd{v.p};
      int64_t us = 0;
      if (dq::schema_parse_timestamp(rd, v.n, els, n, us)) std::printf("V %" PRId64 "\n", us);
      else std::printf("N\n");
    } else if (kind == 'R') {
      unsigned long long seed = 1;
      long count = 0;
      if (std::sscanf(line + 2, "%llu %ld", &seed, &count) < 2) return 2;
      rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
      const char* masks[] = {"yyyy-MM-dd HH:mm:ss", "yyyy.MM.dd 'at' HH'h'mm''ss", "d/M/yyyy", "HH:mm", "'x'yyyy"};
      const char alphabet[] = "0123456789+-..eE \t:/'xat";
      uint64_t sum = 0;
      for (long k = 0; k < count; ++k) {
        std::vector<uint8_t> b(rnd() % 48);
        for (auto& c : b) c = rnd() % 8 == 0 ? (uint8_t)rnd() : (uint8_t)alphabet[rnd() % (sizeof alphabet - 1)];
        const Exact v(b);
        dq::CastHostBytes rd{v.p};
        int32_t x = 0;
        uint64_t lo = 0, hi = 0;
        int64_t us = 0;
        sum = sum * 31 + (dq::schema_to_int(rd, v.n, x) ? (uint32_t)x : 7u);
        const int p = 1 + (int)(rnd() % 38), s = (int)(rnd() % (unsigned)(p + 1));
        sum = sum * 31 + (dq::schema_to_decimal(rd, v.n, p, s, t, lo, hi) ? lo ^ hi : 11u);
        sum = sum * 31 + (uint64_t)dq::schema_char_count(rd, v.n);
        for (const char* m : masks) {
          dq::SchemaMaskEl els[dq::kSchemaMaxMask];
          const char* why = nullptr;
          const int n = dq::schema_compile_mask(m, els, &why);
          if (n < 0) return 3;
          sum = sum * 31 + (dq::schema_parse_timestamp(rd, v.n, els, n, us) ? (uint64_t)us : 13u);
        }
        // a random mask through the compiler alone
        std::string rm(rnd() % 12, ' ');
        for (auto& c : rm) c = "yMdHmsS'-: a1"[rnd() % 13];
        dq::SchemaMaskEl els[dq::kSchemaMaxMask];
        const char* why = nullptr;
        sum = sum * 31 + (uint64_t)(dq::schema_compile_mask(rm.c_str(), els, &why) + 1);
      }
      std::printf("R %016" PRIx64 "\n", sum);
    } else {
      return 2;
    }
  }
  return 0;
}
