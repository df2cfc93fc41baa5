// dq_schema.h -- the per-value rules of RowLevelSchemaValidator (schema/RowLevelSchemaValidator.scala:25-282) as
// Spark 2.2 evaluates them, host + device, templated on the byte reader like dq_cast.h:
//   * schema_to_int: Cast(c, IntegerType) (:240) = UTF8String.toInt: cast_to_long's algorithm (dq_cast.h) with
//     Int.MinValue limits -- raw bytes, [+-]digits[.digits], the fraction checked and dropped; -2147483648 is a
//     value, 2147483648 NULL;
//   * schema_to_decimal: Cast(c, DecimalType(p, s)) (:255-256) = new java.math.BigDecimal(text), then
//     Decimal.changePrecision(p, s) with ROUND_HALF_UP, NumberFormatException -> NULL, no trimming.  Grammar
//     [+-] (digits [. digits*] | . digits) [(e|E) [+-] digits]; an exponent of more than 10 digits after its leading
//     zeros, or a scale (fraction digits - exponent) outside int32, is an error.  The result is the unscaled 128-bit
//     integer at scale s: digits past the scale are dropped and the magnitude goes up by one iff the first dropped
//     digit is >= 5; NULL iff the rounded magnitude reaches 10^p.  Integer-only, so exact for every input length: a
//     grammar-and-counts walk finds where the kept digits end, an accumulate walk reads only those;
//   * schema_parse_timestamp: unix_timestamp(c, mask) (:275) = SimpleDateFormat(mask, Locale.US).parse (lenient)
//     against a mask compiled on the host (schema_compile_mask) into (kind, literal) elements: fields y (count >= 3),
//     M (count <= 2), d, H, m, s each followed by a literal or the end; a literal must equal the next character;
//     blanks and tabs are skipped before a field; a field is DecimalFormat's integer parse ([-] digits [E [-] digits],
//     the exponent taken only when exponent digits follow); text after the last element is ignored; a lenient
//     calendar takes any field value, so validity is this grammar alone.  The value: seconds since the epoch in UTC
//     of the proleptic Gregorian date (the month rolls years; day, hour, minute, second add linearly), times 10^6;
//   * schema_char_count: length(c) (:261, :265) = UTF-8 characters, i.e. bytes that are not 10xxxxxx;
//   * schema_regex_nonempty: regexp_extract(c, p, 0) != "" (:270), the DQ_REGEX_EXTRACT_NONEMPTY walk of the
//     serialized DFA (dq_regex.h regex_serialize);
// and schema_eval: one column definition's clauses of toCNF (:225-281) for one row.
// Non-ASCII Unicode digits, which BigDecimal and DecimalFormat accept, are malformed here (parity unpinned).
// Checked on the host against tests/schema_ref.py (tests/test_schema_host.py) and on the GPU (tests/test_schema_gpu.py).
#pragma once

#include <cstdint>

#include "dq_cast.h"

namespace dq {

enum SchemaKind { SCHEMA_STRING = 1, SCHEMA_INT = 2, SCHEMA_DECIMAL = 3, SCHEMA_TIMESTAMP = 4 };
enum SchemaFlag { SCHEMA_NOT_NULLABLE = 1, SCHEMA_HAS_MIN = 2, SCHEMA_HAS_MAX = 4, SCHEMA_HAS_REGEX = 8 };
enum SchemaMaskKind { MASK_LITERAL = 0, MASK_YEAR = 1, MASK_MONTH = 2, MASK_DAY = 3, MASK_HOUR = 4, MASK_MINUTE = 5, MASK_SECOND = 6 };

// one element of a compiled timestamp mask: a field, or one literal character
struct SchemaMaskEl {
  uint8_t kind;  // SchemaMaskKind
  uint8_t lit;
};

// one column definition as the rules read it (host and device copies are the same bytes)
struct SchemaDef {
  int32_t kind;   // SchemaKind
  int32_t flags;  // SchemaFlag bits
  int32_t minv, maxv;  // INT: minValue / maxValue; STRING: minLength / maxLength
  int32_t p, s;        // DECIMAL
  int32_t aux;         // STRING: the DFA's first word in the regex blob; TIMESTAMP: the mask's first element
  int32_t aux_n;       // TIMESTAMP: mask elements
};

// the cast of one value: INT in lo (sign-extended), DECIMAL in (lo, hi), TIMESTAMP microseconds in lo
struct SchemaCast {
  uint64_t lo, hi;
  bool ok;  // the cast is not NULL
};

constexpr int64_t kSchemaFieldCap = 1000000000000000ll;  // 10^15: a timestamp field's magnitude saturates here
constexpr int kSchemaMaxMask = 64;                       // elements of one compiled mask

// SimpleDateFormat's pattern -> elements (host).  Returns the element count, or -1 with *why set for a mask outside
// the subset: a letter other than y M d H m s, y with a count below 3 (a two-digit year is adjusted to a century),
// M with a count above 2 (a text month), a field that abuts the previous one (its width would bound the parse), an
// unquoted digit or a non-ASCII character, an unterminated quote, no field at all, or more than kSchemaMaxMask elements.
inline int schema_compile_mask(const char* mask, SchemaMaskEl* out, const char** why) {
  int n = 0, fields = 0;
  bool prev_field = false;
  const auto emit = [&](uint8_t kind, uint8_t lit) {
    if (n < kSchemaMaxMask) out[n] = SchemaMaskEl{kind, lit};
    ++n;
    prev_field = kind != MASK_LITERAL;
  };
  const auto ascii = [](unsigned char c) { return c >= 0x20 && c < 0x7F; };
  for (const char* p = mask; *p;) {
    const unsigned char c = (unsigned char)*p;
    if (c == '\'') {
      if (p[1] == '\'') {  // '' is one quote character
        emit(MASK_LITERAL, '\'');
        p += 2;
        continue;
      }
      ++p;
      bool closed = false;
      while (*p) {
        if (*p == '\'') {
          if (p[1] == '\'') {
            emit(MASK_LITERAL, '\'');
            p += 2;
            continue;
          }
          closed = true;
          ++p;
          break;
        }
        if (!ascii((unsigned char)*p)) return *why = "a non-ASCII literal", -1;
        emit(MASK_LITERAL, (uint8_t)*p++);
      }
      if (!closed) return *why = "unterminated quote", -1;
      continue;
    }
    if ((c | 0x20u) - 'a' < 26u) {
      int count = 0;
      while ((unsigned char)*p == c) ++p, ++count;
      uint8_t kind;
      switch (c) {
        case 'y': kind = MASK_YEAR; break;
        case 'M': kind = MASK_MONTH; break;
        case 'd': kind = MASK_DAY; break;
        case 'H': kind = MASK_HOUR; break;
        case 'm': kind = MASK_MINUTE; break;
        case 's': kind = MASK_SECOND; break;
        default: return *why = "a pattern letter other than y M d H m s", -1;
      }
      if (kind == MASK_YEAR && count < 3) return *why = "a year field of fewer than 3 letters", -1;
      if (kind == MASK_MONTH && count > 2) return *why = "a text month", -1;
      if (prev_field) return *why = "abutting fields", -1;
      emit(kind, 0);
      ++fields;
      continue;
    }
    if (!ascii(c) || c - '0' <= 9u) return *why = "an unquoted digit or a non-ASCII character", -1;
    emit(MASK_LITERAL, c);
    ++p;
  }
  if (fields == 0) return *why = "no field", -1;
  if (n > kSchemaMaxMask) return *why = "too many elements", -1;
  return n;
}

// UTF8String.toInt: false = NULL
template <typename Rd>
DQ_HD bool schema_to_int(Rd& rd, typename Rd::idx n, int32_t& out) {
  using I = typename Rd::idx;
  if (n <= 0) return false;
  uint32_t b = rd.at(0);
  const bool negative = b == '-';
  I offset = 0;
  if (negative || b == '+') {
    offset = 1;
    if (n == 1) return false;
  }
  const int64_t stop_value = INT32_MIN / 10;
  int64_t result = 0;  // Java's int accumulator, kept wide: it wraps exactly when this leaves the int range
  while (offset < n) {
    b = rd.at(offset);
    ++offset;
    if (b == '.') break;
    if (!cast_is_digit(b)) return false;
    if (result < stop_value) return false;
    result = result * 10 - (int64_t)(b - '0');
    if (result < INT32_MIN) return false;  // (Java: the int wrapped to a positive value)
  }
  while (offset < n) {
    if (!cast_is_digit(rd.at(offset))) return false;
    ++offset;
  }
  if (!negative) {
    if (result == INT32_MIN) return false;  // 2147483648
    result = -result;
  }
  out = (int32_t)result;
  return true;
}

// Cast(StringType -> DecimalType(p, s)): false = NULL; (lo, hi) = the two's-complement unscaled value
template <typename Rd>
DQ_HD bool schema_to_decimal(Rd& rd, typename Rd::idx n, int p, int s, const DecTab& t, uint64_t& lo, uint64_t& hi) {
  using I = typename Rd::idx;
  // walk 1: the grammar, the digit counts and the exponent
  I i = 0;
  if (n <= 0) return false;
  uint32_t c = rd.at(0);
  const bool neg = c == '-';
  if (neg || c == '+') i = 1;
  const I d0 = i;      // the first digit (or the point)
  int64_t nint = 0, nfrac = 0;
  int64_t lz = -1;     // leading zero digits of the digit string (-1: no non-zero digit yet)
  int64_t seen = 0;
  bool point = false;
  for (; i < n; ++i) {
    c = rd.at(i);
    if (c == '.' && !point) {
      point = true;
      continue;
    }
    if (!cast_is_digit(c)) break;
    if (point) ++nfrac;
    else ++nint;
    if (lz < 0 && c != '0') lz = seen;
    ++seen;
  }
  if (seen == 0) return false;  // "", ".", "+", "e5"
  int64_t exp10 = 0;
  if (i < n) {
    if ((c | 0x20u) != 'e') return false;
    ++i;
    bool eneg = false;
    if (i < n && ((c = rd.at(i)) == '+' || c == '-')) eneg = c == '-', ++i;
    if (i >= n) return false;  // "1e", "1e+"
    int edig = 0;              // exponent digits from the first non-zero one
    for (; i < n; ++i) {
      c = rd.at(i);
      if (!cast_is_digit(c)) return false;
      if (edig == 0 && c == '0') continue;
      if (++edig > 10) return false;  // BigDecimal: too many nonzero exponent digits
      exp10 = exp10 * 10 + (int64_t)(c - '0');
    }
    if (eneg) exp10 = -exp10;
  }
  const int64_t scale = nfrac - exp10;  // BigDecimal's scale
  if (scale > INT32_MAX || scale < INT32_MIN) return false;  // "Scale out of range"
  lo = hi = 0;
  if (lz < 0) return true;  // a zero of any exponent
  // the value is digits * 10^-scale; at scale s the unscaled integer is digits * 10^k
  const int64_t nd = nint + nfrac;
  const int64_t k = (int64_t)s - scale;
  const int64_t kept = k < 0 ? nd + k : nd;  // digits of the string that stay (may be <= 0)
  if (kept < lz) return true;                // every kept digit and the first dropped one are zeros: rounds to 0
  const int64_t sig = kept - lz;             // kept digits from the first non-zero one
  if (sig + (k > 0 ? k : 0) > kDecMaxPrecision) return false;  // >= 10^38 >= 10^p
  // walk 2: digit j of the string is byte d0 + j (+ 1 past the point)
  uint64_t a = 0, b19 = 0;
  for (int64_t j = lz; j < kept; ++j) {
    const uint32_t d = rd.at((I)(d0 + j + (j >= nint ? 1 : 0))) - '0';
    if (j - lz < 19) a = a * 10u + d;
    else b19 = b19 * 10u + d;
  }
  u128 mag = sig <= 19 ? (u128)a : (u128)a * t.p10lo[sig - 19] + b19;
  if (k < 0 && kept < nd) {  // ROUND_HALF_UP on the first dropped digit alone
    const uint32_t d = rd.at((I)(d0 + kept + (kept >= nint ? 1 : 0))) - '0';
    if (d >= 5) mag += 1;
  }
  if (k > 0) mag *= dec_p10(t, (int)k);
  if (mag >= dec_p10(t, p)) return false;  // changePrecision: more than p digits
  if (neg) mag = (u128)0 - mag;
  lo = (uint64_t)mag;
  hi = (uint64_t)(mag >> 64);
  return true;
}

// days from 1970-01-01 to year-month-1 in the proleptic Gregorian calendar (month 1..12)
DQ_HD int64_t schema_days_from_civil(int64_t y, int64_t m) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

// SimpleDateFormat.parse against a compiled mask: false = ParseException; micros = the TimestampType value
template <typename Rd>
DQ_HD bool schema_parse_timestamp(Rd& rd, typename Rd::idx n, const SchemaMaskEl* mask, int n_mask, int64_t& micros) {
  using I = typename Rd::idx;
  int64_t fy = 1970, fmo = 1, fd = 1, fh = 0, fmi = 0, fs = 0;  // (no runtime-indexed array: registers)
  I i = 0;
  for (int e = 0; e < n_mask; ++e) {
    const int kind = mask[e].kind;
    if (kind == MASK_LITERAL) {
      if (i >= n || rd.at(i) != mask[e].lit) return false;
      ++i;
      continue;
    }
    uint32_t c = 0;
    for (;; ++i) {  // SimpleDateFormat.subParse skips blanks and tabs before a field
      if (i >= n) return false;
      c = rd.at(i);
      if (c != ' ' && c != '\t') break;
    }
    const bool neg = c == '-';
    if (neg) {
      if (++i >= n) return false;
      c = rd.at(i);
    }
    if (!cast_is_digit(c)) return false;
    int64_t v = 0;
    for (; i < n && cast_is_digit(c = rd.at(i)); ++i) {
      v = v * 10 + (int64_t)(c - '0');
      if (v > kSchemaFieldCap) v = kSchemaFieldCap;
    }
    if (i < n && rd.at(i) == 'E') {  // an exponent counts only when its digits follow
      I j = i + 1;
      bool eneg = false;
      if (j < n && rd.at(j) == '-') eneg = true, ++j;
      if (j < n && cast_is_digit(rd.at(j))) {
        int ex = 0;
        for (; j < n && cast_is_digit(c = rd.at(j)); ++j) {
          ex = ex * 10 + (int)(c - '0');
          if (ex > 32) ex = 32;
        }
        i = j;
        for (; ex > 0; --ex) {
          if (eneg) v /= 10;
          else if ((v *= 10) > kSchemaFieldCap) v = kSchemaFieldCap;
        }
      }
    }
    v = neg ? -v : v;
    fy = kind == MASK_YEAR ? v : fy;
    fmo = kind == MASK_MONTH ? v : fmo;
    fd = kind == MASK_DAY ? v : fd;
    fh = kind == MASK_HOUR ? v : fh;
    fmi = kind == MASK_MINUTE ? v : fmi;
    fs = kind == MASK_SECOND ? v : fs;
  }
  // lenient calendar: the month rolls years, the rest add linearly (every field is at most 10^15 in magnitude)
  const int64_t months = fy * 12 + (fmo - 1);
  const int64_t y = (months >= 0 ? months : months - 11) / 12;
  const int64_t m = months - y * 12 + 1;
  const uint64_t days = (uint64_t)(schema_days_from_civil(y, m) + (fd - 1));
  // (from here wrapping arithmetic, as Java's long does)
  const uint64_t secs = days * 86400u + (uint64_t)fh * 3600u + (uint64_t)fmi * 60u + (uint64_t)fs;
  micros = (int64_t)(secs * 1000000u);
  return true;
}

// length(c): UTF-8 characters of valid UTF-8
template <typename Rd>
DQ_HD int64_t schema_char_count(Rd& rd, typename Rd::idx n) {
  int64_t cnt = 0;
  for (typename Rd::idx i = 0; i < n; ++i) cnt += (rd.at(i) & 0xC0u) != 0x80u;
  return cnt;
}

// the search DFA of one pattern (regex_serialize's words) over a value: true iff the extract is non-empty
template <typename Rd>
DQ_HD bool schema_regex_nonempty(const uint16_t* dfa, Rd& rd, typename Rd::idx n) {
  const uint32_t ns = dfa[0], nc = dfa[1];
  uint32_t st = dfa[2];
  const uint16_t* cls = dfa + 4;
  const uint16_t* acc = cls + 256;
  const uint16_t* tr = acc + ns;
  for (typename Rd::idx i = 0; i < n && st >= 2u; ++i) st = tr[st * nc + cls[rd.at(i)]];
  return acc[st] != 0;
}

enum SchemaOutcome { SCHEMA_CLAUSE_FALSE = 1, SCHEMA_CLAUSE_NULL = 2 };

// One definition's clauses of toCNF (:230-277) for one row: SCHEMA_CLAUSE_FALSE when a clause is FALSE,
// SCHEMA_CLAUSE_NULL when one is NULL (only `colIsNull.isNull.or(v >= min)` of :246 on a NULL source, which is
// FALSE OR NULL), both bits possible.  `cast` receives the definition's cast of the value (ok = false: NULL).
template <typename Rd>
DQ_HD int schema_eval(const SchemaDef& d, const SchemaMaskEl* masks, const uint16_t* regex, const DecTab& t, Rd& rd,
                      typename Rd::idx n, bool is_null, SchemaCast& cast) {
  cast.lo = cast.hi = 0;
  cast.ok = false;
  int out = 0;
  if (is_null) {
    if (d.flags & SCHEMA_NOT_NULLABLE) out |= SCHEMA_CLAUSE_FALSE;                         // :230-232
    if (d.kind == SCHEMA_INT && (d.flags & SCHEMA_HAS_MIN)) out |= SCHEMA_CLAUSE_NULL;     // :246
    return out;  // every other clause is `colIsNull.or(...)`: TRUE
  }
  switch (d.kind) {
    case SCHEMA_INT: {
      int32_t v = 0;
      if (!schema_to_int(rd, n, v)) return SCHEMA_CLAUSE_FALSE;                            // :243
      cast.lo = (uint64_t)(int64_t)v;
      cast.ok = true;
      if ((d.flags & SCHEMA_HAS_MIN) && !(v >= d.minv)) out |= SCHEMA_CLAUSE_FALSE;        // :246
      if ((d.flags & SCHEMA_HAS_MAX) && !(v <= d.maxv)) out |= SCHEMA_CLAUSE_FALSE;        // :250
      return out;
    }
    case SCHEMA_DECIMAL:
      cast.ok = schema_to_decimal(rd, n, d.p, d.s, t, cast.lo, cast.hi);                   // :255-256
      return cast.ok ? 0 : SCHEMA_CLAUSE_FALSE;
    case SCHEMA_TIMESTAMP: {
      int64_t us = 0;
      cast.ok = schema_parse_timestamp(rd, n, masks + d.aux, d.aux_n, us);                 // :275-276
      cast.lo = cast.ok ? (uint64_t)us : 0;
      return cast.ok ? 0 : SCHEMA_CLAUSE_FALSE;
    }
    default: {  // SCHEMA_STRING
      cast.ok = true;
      if (d.flags & (SCHEMA_HAS_MIN | SCHEMA_HAS_MAX)) {
        const int64_t len = schema_char_count(rd, n);
        if ((d.flags & SCHEMA_HAS_MIN) && !(len >= d.minv)) out |= SCHEMA_CLAUSE_FALSE;    // :261
        if ((d.flags & SCHEMA_HAS_MAX) && !(len <= d.maxv)) out |= SCHEMA_CLAUSE_FALSE;    // :265
      }
      if (out == 0 && (d.flags & SCHEMA_HAS_REGEX) && !schema_regex_nonempty(regex + d.aux, rd, n))
        out |= SCHEMA_CLAUSE_FALSE;                                                        // :270
      return out;
    }
  }
}

}  // namespace dq
