// dq_cast.h -- Cast(StringType -> LongType | DoubleType) of one value as Spark 2.2 evaluates it, host + device
// (the ColumnProfiler's castNumericStringColumns: profiles/ColumnProfiler.scala:330-339, 399-417):
//   * to long: org.apache.spark.unsafe.types.UTF8String.toLong(LongWrapper), which Cast.castToLong calls on the
//     raw bytes (no trimming): optional sign, digits accumulated as a negative number under Java's overflow
//     checks, the first '.' ends the integer part and every byte after it must be a digit (the fraction is
//     dropped: truncation toward zero), anything else is NULL;
//   * to double: Cast.castToDouble = `s.toString.toDouble` with NumberFormatException -> NULL, i.e.
//     java.lang.Double.parseDouble (sun.misc.FloatingDecimal.readJavaFormatString): String.trim (chars <= U+0020),
//     optional sign, then NaN | Infinity | a decimal (digits[.digits] | .digits | digits. with an optional
//     e|E[sign]digits) | a hex float (0x.. with a mandatory p exponent), the last two with an optional fFdD
//     suffix; the result is the correctly rounded (nearest, ties to even) double.
// The grammar is decided here for every value.  The conversion itself has two tiers: a decimal whose significand
// (leading zeros stripped) has at most 38 digits, whose written exponent is below 100000 in magnitude and whose net
// exponent (written exponent - fraction digits, both counted exactly) is in [-38, 0] -- or positive with the
// integer still within 38 digits -- is unscaled / 10^s of dq_decimal.h (correctly rounded, exact midpoint settle
// included); every other valid value (more digits, larger exponents, hex floats) is reported CAST_HARD and is
// converted on the host by an exact routine (dq_cast.hip), never approximated.
// Checked on the host against a Python restatement (tests/test_cast_host.py) and on the GPU (tests/test_cast_gpu.py).
#pragma once

#include <cstdint>

#include "dq_decimal.h"

namespace dq {

enum CastKind { CAST_NULL = 0, CAST_VALUE = 1, CAST_HARD = 2 };

constexpr int32_t kCastExpSat = 100000;  // written exponents of this magnitude or more are hard rows
constexpr uint64_t kJavaNaNBits = 0x7FF8000000000000ull;  // Double.NaN (what parseDouble returns for [+-]NaN)

// the bytes of one value on the host; the kernels read theirs through aligned dwords (dq_cast.hip)
struct CastHostBytes {
  using idx = int64_t;
  const uint8_t* p;
  uint32_t at(idx i) const { return p[i]; }
};

DQ_HD bool cast_is_digit(uint32_t c) { return c - '0' <= 9u; }
DQ_HD bool cast_is_hex(uint32_t c) { return c - '0' <= 9u || (c | 0x20u) - 'a' <= 5u; }

// UTF8String.toLong: false = NULL
template <typename Rd>
DQ_HD bool cast_to_long(Rd& rd, typename Rd::idx n, int64_t& out) {
  using I = typename Rd::idx;
  if (n <= 0) return false;
  uint32_t b = rd.at(0);
  const bool negative = b == '-';
  I offset = 0;
  if (negative || b == '+') {
    offset = 1;
    if (n == 1) return false;
  }
  const int64_t stop_value = INT64_MIN / 10;
  int64_t result = 0;
  while (offset < n) {
    b = rd.at(offset);
    ++offset;
    if (b == '.') break;  // the separator: the rest is the fraction
    if (!cast_is_digit(b)) return false;
    if (result < stop_value) return false;  // result * 10 would overflow
    result = (int64_t)((uint64_t)result * 10u - (uint64_t)(b - '0'));  // (wraps as Java's long does)
    if (result > 0) return false;           // ... or the subtraction did
  }
  while (offset < n) {  // the fraction is only checked to be well formed
    if (!cast_is_digit(rd.at(offset))) return false;
    ++offset;
  }
  if (!negative) {
    if (result == INT64_MIN) return false;  // -result < 0 in Java: 9223372036854775808
    result = -result;
  }
  out = result;
  return true;
}

// Double.parseDouble.  CAST_VALUE: `bits` holds the double.  CAST_HARD: a valid value outside the fast tier; its
// text without the blanks and the type suffix is [core_b, core_e) -- a form C's strtod reads the same way.
template <typename Rd>
DQ_HD int cast_to_double(Rd& rd, typename Rd::idx n, const DecTab& t, uint64_t& bits, typename Rd::idx& core_b,
                         typename Rd::idx& core_e) {
  using I = typename Rd::idx;
  I b = 0, e = n;
  while (b < e && rd.at(b) <= 0x20u) ++b;
  while (e > b && rd.at(e - 1) <= 0x20u) --e;
  if (b >= e) return CAST_NULL;
  I i = b;
  uint32_t c = rd.at(i);
  const bool neg = c == '-';
  if (neg || c == '+') {
    if (++i == e) return CAST_NULL;
    c = rd.at(i);
  }
  const uint64_t sign = neg ? 1ull << 63 : 0;
  if (c == 'N') {
    if (e - i != 3 || rd.at(i + 1) != 'a' || rd.at(i + 2) != 'N') return CAST_NULL;
    bits = kJavaNaNBits;
    return CAST_VALUE;
  }
  if (c == 'I') {
    const char* inf = "Infinity";
    if (e - i != 8) return CAST_NULL;
    for (int k = 1; k < 8; ++k)
      if (rd.at(i + k) != (uint32_t)inf[k]) return CAST_NULL;
    bits = sign | 0x7FF0000000000000ull;
    return CAST_VALUE;
  }
  core_b = b;
  I j = i;
  if (c == '0' && i + 1 < e && (rd.at(i + 1) | 0x20u) == 'x') {
    // HexFloatingPointLiteral: 0x HexDigits [.] | 0x [HexDigits] . HexDigits, then p [sign] Digits
    j = i + 2;
    bool any = false;
    while (j < e && cast_is_hex(rd.at(j))) ++j, any = true;
    if (j < e && rd.at(j) == '.') {
      ++j;
      while (j < e && cast_is_hex(rd.at(j))) ++j, any = true;
    }
    if (!any || j >= e || (rd.at(j) | 0x20u) != 'p') return CAST_NULL;
    ++j;
    if (j < e && (rd.at(j) == '+' || rd.at(j) == '-')) ++j;
    bool exp_digit = false;
    while (j < e && cast_is_digit(rd.at(j))) ++j, exp_digit = true;
    if (!exp_digit) return CAST_NULL;
    core_e = j;
    if (j < e && ((c = rd.at(j) | 0x20u) == 'f' || c == 'd')) ++j;
    return j == e ? CAST_HARD : CAST_NULL;
  }
  // decimal: the significand's first 19 significant digits in `a`, the next (up to 19) in `lo19`
  uint64_t a = 0, lo19 = 0;
  int nd = 0;           // significant digits (from the first non-zero one), saturating at 39
  I nfrac = 0;          // digits after the point, counted exactly (a value's bytes fit its index type)
  bool any = false;
  bool frac = false;
  for (; j < e; ++j) {
    c = rd.at(j);
    if (c == '.' && !frac) {
      frac = true;
      continue;
    }
    if (!cast_is_digit(c)) break;
    any = true;
    if (frac) ++nfrac;
    const uint32_t d = c - '0';
    if (nd == 0 && d == 0) continue;  // a leading zero
    if (nd < 19) a = a * 10u + d;
    else if (nd < 38) lo19 = lo19 * 10u + d;
    if (nd < 39) ++nd;
  }
  if (!any) return CAST_NULL;  // "", ".", "e5", "+"
  int32_t exp10 = 0;
  if (j < e && (rd.at(j) | 0x20u) == 'e') {
    ++j;
    bool eneg = false;
    if (j < e && ((c = rd.at(j)) == '+' || c == '-')) eneg = c == '-', ++j;
    bool exp_digit = false;
    for (; j < e && cast_is_digit(c = rd.at(j)); ++j) {
      exp_digit = true;
      if (exp10 < kCastExpSat) exp10 = exp10 * 10 + (int32_t)(c - '0');  // (saturates: a hard row below)
    }
    if (!exp_digit) return CAST_NULL;
    if (eneg) exp10 = -exp10;
  }
  core_e = j;
  if (j < e && ((c = rd.at(j) | 0x20u) == 'f' || c == 'd')) ++j;
  if (j != e) return CAST_NULL;
  if (nd == 0) {  // every digit a zero: +-0.0 whatever the exponent
    bits = sign;
    return CAST_VALUE;
  }
  // a saturated exponent never enters the arithmetic: the host tier reads the text itself
  if (nd > 38 || exp10 >= kCastExpSat || exp10 <= -kCastExpSat) return CAST_HARD;
  const int64_t ex = (int64_t)exp10 - (int64_t)nfrac;  // value = significand * 10^ex, exactly
  u128 sig = nd <= 19 ? (u128)a : (u128)a * t.p10lo[nd - 19] + lo19;
  int s;
  if (ex <= 0 && ex >= -kDecMaxPrecision) {
    s = (int)-ex;
  } else if (ex > 0 && nd + ex <= kDecMaxPrecision) {
    sig *= dec_p10(t, (int)ex);  // still an integer of at most 38 digits
    s = 0;
  } else {
    return CAST_HARD;
  }
  const uint64_t slo = (uint64_t)sig, shi = (uint64_t)(sig >> 64);
  bits = sign | dec_bits(dec_to_double(slo, shi, s, t, shi == 0 && (int64_t)slo >= 0));
  return CAST_VALUE;
}

}  // namespace dq
