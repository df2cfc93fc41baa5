// cast_check.cpp -- host harness for tests/test_cast_host.py: runs dq_cast.h (the parse the kernels run) on the
// host.  stdin: lines "<L|D> <hex bytes, or - for the empty string>"; stdout per line: "N" (NULL), "V <bits hex>"
// (the long / the double's bits) or "H <b> <e>" (a hard row of the double cast and the text the host tier reads).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dq_cast.h"

#define DQ_DEC_TABLE static const
#include "dq_dec_tables.inc"

int main() {
  const dq::DecTab t{kDecP10Lo, kDecP10Hi, kDecRcpHi, kDecRcpLo};
  static char line[1 << 20];
  while (std::fgets(line, sizeof line, stdin)) {
    const char kind = line[0];
    std::vector<uint8_t> bytes;
    for (const char* p = line + 2; p[0] && p[1] && p[0] != '-' && p[0] != '\n'; p += 2) {
      const auto nib = [](char c) { return (unsigned)(c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10); };
      bytes.push_back((uint8_t)(nib(p[0]) << 4 | nib(p[1])));
    }
    dq::CastHostBytes rd{bytes.data()};
    const int64_t n = (int64_t)bytes.size();
    if (kind == 'L') {
      int64_t v = 0;
      if (dq::cast_to_long(rd, n, v)) std::printf("V %016" PRIx64 "\n", (uint64_t)v);
      else std::printf("N\n");
    } else {
      uint64_t bits = 0;
      int64_t b = 0, e = 0;
      const int k = dq::cast_to_double(rd, n, t, bits, b, e);
      if (k == dq::CAST_VALUE) std::printf("V %016" PRIx64 "\n", bits);
      else if (k == dq::CAST_HARD) std::printf("H %" PRId64 " %" PRId64 "\n", b, e);
      else std::printf("N\n");
    }
  }
  return 0;
}
