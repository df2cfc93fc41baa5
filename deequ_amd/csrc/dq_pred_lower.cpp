// dq_pred_lower.cpp -- predicate lowering (IR tree -> postfix program over three-valued atoms, with Spark 2.2's
// coercions) and PredBuilder, the one assembler of PredPrograms (dq_pred_lower.h).  It parses caller-supplied IR and
// calls nothing of the HIP runtime.
#include "dq_pred_lower.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "dq_plan_host.h"
#include "dq_regex.h"

namespace dq {

// (double)(float)v as Java's long -> float conversion rounds it (to nearest, ties to even)
static double int_as_float(int64_t v) { return (double)(float)v; }

struct Lit {  // exact literal: int / decimal (unscaled, scale) / double / null / bool
  enum K { INT, DEC, DBL, NUL, BOOL } k;
  int64_t i = 0;
  int32_t scale = 0;
  double d = 0.0;
};

static double lit_to_double(const Lit& l) {
  if (l.k == Lit::DBL) return l.d;
  if (l.k == Lit::INT || l.k == Lit::BOOL) return (double)l.i;
  // decimal -> correctly rounded double via its decimal text (Decimal.toDouble)
  char buf[64];
  long long u = (long long)l.i;
  bool neg = u < 0;
  unsigned long long a = neg ? (unsigned long long)(-(u + 1)) + 1ull : (unsigned long long)u;
  std::string digits = std::to_string(a);
  while ((int)digits.size() <= l.scale) digits = "0" + digits;
  std::string txt = (neg ? "-" : "") + digits.substr(0, digits.size() - l.scale) +
                    (l.scale ? "." + digits.substr(digits.size() - l.scale) : "");
  std::snprintf(buf, sizeof(buf), "%s", txt.c_str());
  return std::strtod(buf, nullptr);
}

static bool pow10_i64(int s, int64_t& out) {
  if (s < 0 || s > 18) return false;
  int64_t p = 1;
  for (int i = 0; i < s; ++i) p *= 10;
  out = p;
  return true;
}

// floor(u / p) for p > 0, without the overflow of -u + p - 1 near INT64_MIN
static int64_t floor_div(int64_t u, int64_t p) {
  const int64_t q = u / p;
  return (u % p != 0 && u < 0) ? q - 1 : q;
}

// exact compare of two non-double literals: returns -1/0/1
static int exact_cmp(const Lit& a, const Lit& b) {
  int64_t pa = 1, pb = 1;
  pow10_i64(a.k == Lit::DEC ? a.scale : 0, pa);
  pow10_i64(b.k == Lit::DEC ? b.scale : 0, pb);
  __int128 x = (__int128)a.i * pb, y = (__int128)b.i * pa;
  return (x > y) - (x < y);
}

static int flip_cmp(int c) {
  switch (c) {
    case DQ_CMP_LT: return DQ_CMP_GT;
    case DQ_CMP_LE: return DQ_CMP_GE;
    case DQ_CMP_GT: return DQ_CMP_LT;
    case DQ_CMP_GE: return DQ_CMP_LE;
    default: return c;
  }
}

static bool cmp_holds(int c, int r) {
  switch (c) {
    case DQ_CMP_LT: return r < 0;
    case DQ_CMP_LE: return r <= 0;
    case DQ_CMP_GT: return r > 0;
    case DQ_CMP_GE: return r >= 0;
    case DQ_CMP_EQ: return r == 0;
    default: return r != 0;
  }
}

static int dbl_cmp(double a, double b) {  // Spark nanSafeCompare
  bool an = a != a, bn = b != b;
  if (an || bn) return (an && bn) ? 0 : (an ? 1 : -1);
  return (a > b) - (a < b);
}

// literal-vs-literal comparison under Spark coercion: any double -> double, else exact decimal
static int lit_cmp_result(int cmp, const Lit& a, const Lit& b) {  // returns NR_*
  if (a.k == Lit::NUL || b.k == Lit::NUL) return NR_NULL;
  int r = (a.k == Lit::DBL || b.k == Lit::DBL) ? dbl_cmp(lit_to_double(a), lit_to_double(b)) : exact_cmp(a, b);
  return cmp_holds(cmp, r) ? NR_TRUE : NR_FALSE;
}

static int to_cmpop(int c) {
  switch (c) {
    case DQ_CMP_LT: return C_LT;
    case DQ_CMP_LE: return C_LE;
    case DQ_CMP_GT: return C_GT;
    case DQ_CMP_GE: return C_GE;
    case DQ_CMP_EQ: return C_EQ;
    default: return C_NE;
  }
}

struct Lowering {
  const dq_pred_node* pool;
  int32_t n_pred;
  const std::vector<dq_column_desc>* schema;
  std::vector<PredInstr> out;
  const std::vector<std::string>* patterns = nullptr;
  std::vector<uint16_t>* regex_blob = nullptr;              // concatenated DFAs (dq_regex.h layout)
  std::map<std::pair<int64_t, int32_t>, int64_t> regex_at;  // (pattern, mode) -> blob word offset

  dq_status lit_of(int32_t idx, Lit& l) {
    const dq_pred_node& n = pool[idx];
    switch (n.kind) {
      case DQ_PRED_LIT_INT: l.k = Lit::INT; l.i = n.i64; return DQ_OK;
      case DQ_PRED_LIT_DECIMAL:
        if (n.cmp < 0 || n.cmp > 18) return set_error(DQ_E_UNSUPPORTED, "decimal literal scale %d unsupported", n.cmp);
        l.k = Lit::DEC; l.i = n.i64; l.scale = n.cmp; return DQ_OK;
      case DQ_PRED_LIT_DOUBLE: l.k = Lit::DBL; l.d = n.f64; return DQ_OK;
      case DQ_PRED_LIT_NULL: l.k = Lit::NUL; return DQ_OK;
      case DQ_PRED_LIT_BOOL: l.k = Lit::BOOL; l.i = n.i64 ? 1 : 0; return DQ_OK;
      default: return set_error(DQ_E_UNSUPPORTED, "node %d is not a literal", idx);
    }
  }
  bool is_lit(int32_t idx) const {
    int k = pool[idx].kind;
    return k >= DQ_PRED_LIT_INT && k <= DQ_PRED_LIT_BOOL;
  }
  dq_status check_idx(int32_t idx) {
    if (idx < 0 || idx >= n_pred) return set_error(DQ_E_INVALID, "predicate node index %d out of range", idx);
    return DQ_OK;
  }
  dq_status check_col(int32_t c) {
    if (c < 0 || c >= (int32_t)schema->size()) return set_error(DQ_E_INVALID, "predicate column %d out of range", c);
    if (is_dict((*schema)[c].type))  // (every atom's column passes here)
      return set_error(DQ_E_UNSUPPORTED, "predicate over dictionary-encoded column %d: decode it (dq_dict_decode)", c);
    return DQ_OK;
  }
  void push_const(int nr) {
    PredInstr p{};
    p.op = PO_CONST; p.null_res = nr; p.col_a = -1; p.col_b = -1;
    out.push_back(p);
  }

  // operand = column, or COALESCE(column, literal)
  struct Operand { int32_t col = -1; bool has_fallback = false; Lit fallback{}; };

  dq_status operand_of(int32_t idx, Operand& o) {
    const dq_pred_node& n = pool[idx];
    if (n.kind == DQ_PRED_COLUMN) {
      if (dq_status s = check_col(n.a)) return s;
      o.col = n.a;
      return DQ_OK;
    }
    if (n.kind == DQ_PRED_COALESCE) {
      if (dq_status s = check_idx(n.a)) return s;
      if (dq_status s = check_idx(n.b)) return s;
      if (pool[n.a].kind != DQ_PRED_COLUMN || !is_lit(n.b))
        return set_error(DQ_E_UNSUPPORTED, "COALESCE supported only as COALESCE(column, literal)");
      if (dq_status s = check_col(pool[n.a].a)) return s;
      o.col = pool[n.a].a;
      o.has_fallback = true;
      return lit_of(n.b, o.fallback);
    }
    return set_error(DQ_E_UNSUPPORTED, "unsupported comparison operand (node kind %d)", n.kind);
  }

  // DecimalType(p, s) column CMP an integer / decimal literal.  Spark 2.2 (DecimalPrecision) casts an integer
  // literal to DecimalType(10, 0) (an int) or (20, 0) (a long) and both sides to the wider decimal type
  // (max of the integer digits + max of the scales); while that fits 38 digits every cast is exact, so the
  // comparison is the exact rational one, rewritten here into a bound B on the unscaled value u: u CMP B.  Wider
  // types (Spark bounds them to 38 digits and can turn values NULL), double literals (the decimal is cast to
  // double) and boolean literals stay on the fallback.  Precision <= 18: one atom on the low word (the whole value,
  // |u| < 10^18); wider: the 128-bit comparison as atoms on the high word H and the low word L (compared unsigned),
  // e.g. u < B  <=>  H < Bh OR (H = Bh AND L <u Bl).
  dq_status emit_dec_lit(const Operand& o, int cmp, const Lit& lit, int32_t type) {
    const int prec = DQ_DECIMAL_PRECISION(type), sc = DQ_DECIMAL_SCALE(type);
    auto fits = [&](const Lit& l) {  // the wider decimal type of the column and the literal fits 38 digits
      if (l.k == Lit::NUL) return true;
      if (l.k != Lit::INT && l.k != Lit::DEC) return false;
      const int ls = l.k == Lit::DEC ? l.scale : 0;
      int lp;
      if (l.k == Lit::INT) lp = (l.i >= INT32_MIN && l.i <= INT32_MAX) ? 10 : 20;
      else {
        const uint64_t a = l.i < 0 ? (uint64_t)0 - (uint64_t)l.i : (uint64_t)l.i;
        lp = std::max((int)std::to_string(a).size(), ls);
      }
      return std::max(prec - sc, lp - ls) + std::max(sc, ls) <= kDecMaxPrecision;
    };
    if (!fits(lit) || (o.has_fallback && !fits(o.fallback)))
      return set_error(DQ_E_UNSUPPORTED, "decimal column %d compared with a %s literal", o.col,
                       lit.k == Lit::DBL || o.fallback.k == Lit::DBL ? "double" : "wider or boolean");
    const int nr = o.has_fallback ? lit_cmp_result(cmp, o.fallback, lit) : NR_NULL;
    if (lit.k == Lit::NUL) { push_const(NR_NULL); return DQ_OK; }
    // u / 10^sc CMP L / 10^t  ->  u CMP' B
    const int t = lit.k == Lit::DEC ? lit.scale : 0;
    int c2;
    i128 B;
    if (t <= sc) {
      i128 m = 1;
      for (int k = 0; k < sc - t; ++k) m *= 10;
      B = (i128)lit.i * m;  // (fits: the wider type has at most 38 digits)
      c2 = to_cmpop(cmp);
    } else {
      int64_t p10;
      pow10_i64(t - sc, p10);
      const int64_t u = lit.i;
      const int64_t fl = floor_div(u, p10);
      const bool exact = (u % p10) == 0;
      const int64_t ce = exact ? fl : fl + 1;
      switch (cmp) {
        case DQ_CMP_LT: c2 = C_LT; B = ce; break;
        case DQ_CMP_LE: c2 = C_LE; B = fl; break;
        case DQ_CMP_GT: c2 = C_GT; B = fl; break;
        case DQ_CMP_GE: c2 = C_GE; B = ce; break;
        case DQ_CMP_EQ: c2 = exact ? C_EQ : C_FALSE; B = fl; break;
        default: c2 = exact ? C_NE : C_TRUE; B = fl; break;
      }
    }
    auto atom = [&](int kind, int c, int64_t v) {
      PredInstr p{};
      p.op = PO_ATOM_CMP; p.col_a = o.col; p.col_b = -1; p.kind_a = kind; p.kind_b = 0;
      p.ctype = CT_INT; p.cmp = c; p.lit_i = v; p.null_res = nr;
      out.push_back(p);
    };
    auto logic = [&](int op) {
      PredInstr p{};
      p.op = op; p.col_a = p.col_b = -1;
      out.push_back(p);
    };
    if (c2 == C_TRUE || c2 == C_FALSE) { atom(CK_D128_LO, c2, 0); return DQ_OK; }
    if (prec <= 18) {
      if (B > (i128)INT64_MAX || B < (i128)INT64_MIN) {  // every |u| < 10^18 lies on one side of B
        const bool below = B > 0;  // u < B for every u
        const bool holds = c2 == C_LT || c2 == C_LE || c2 == C_NE ? below : (c2 == C_EQ ? false : !below);
        atom(CK_D128_LO, holds ? C_TRUE : C_FALSE, 0);
      } else {
        atom(CK_D128_LO, c2, (int64_t)B);
      }
      return DQ_OK;
    }
    const int64_t bh = (int64_t)(B >> 64);
    const int64_t bl = (int64_t)((uint64_t)B ^ (1ull << 63));  // (CK_D128_LOU flips the loaded low word the same way)
    if (c2 == C_EQ || c2 == C_NE) {
      atom(CK_D128_HI, c2, bh);
      atom(CK_D128_LOU, c2, bl);
      logic(c2 == C_EQ ? PO_AND : PO_OR);
      return DQ_OK;
    }
    const bool lt = c2 == C_LT || c2 == C_LE;
    atom(CK_D128_HI, lt ? C_LT : C_GT, bh);
    atom(CK_D128_HI, C_EQ, bh);
    atom(CK_D128_LOU, c2, bl);
    logic(PO_AND);
    logic(PO_OR);
    return DQ_OK;
  }

  // column CMP literal, or COALESCE(column, fallback) CMP literal, with Spark 2.2's coercions.  The operand's type
  // comes first: the column's, widened by the fallback (COALESCE takes the common type of its arguments); then
  // the comparison's type from the operand and the literal:
  //   integral operand (integral column, fallback NULL / integer / decimal): vs an integer or decimal literal
  //     exact, vs a double literal in double;
  //   an integral column with a double fallback is a DoubleType operand: every literal is cast to double and the
  //     column compares as (double)value, also against an integer or decimal literal;
  //   FloatType operand (float column, fallback NULL / integer, the integer cast to float): vs an integer literal
  //     in float (the literal rounded to float: findTightestCommonType), vs a decimal literal of any scale or a
  //     double literal in double (DecimalPrecision: the decimal cast to double);
  //   a float column with a decimal or double fallback is a DoubleType operand: every literal is cast to double, an
  //     integer one too (not rounded to float);
  //   DoubleType column: the fallback and the literal cast to double.
  // A float widens to double exactly, so every float case is a double compare with the literal rounded as above.
  // null_res is the comparison of the fallback, widened the same way, with the literal.
  dq_status emit_col_lit(const Operand& o, int cmp, Lit lit) {
    const dq_column_desc& cd = (*schema)[o.col];
    if (is_decimal(cd.type)) return emit_dec_lit(o, cmp, lit, cd.type);
    const bool boolean = cd.type == DQ_TYPE_BOOL;
    if (!is_numeric(cd.type) && !boolean)
      return set_error(DQ_E_UNSUPPORTED, "comparison on a non-numeric column (%d)", o.col);
    PredInstr p{};
    p.op = PO_ATOM_CMP; p.col_a = o.col; p.col_b = -1; p.kind_a = kind_of(cd.type); p.kind_b = 0;
    Lit fb = o.fallback;
    if (boolean) {
      // BooleanType vs a boolean literal (Spark orders false < true); against a number Spark 2.2 rewrites
      // (BooleanEquality) or casts -- not restated here: the fallback
      if ((lit.k != Lit::BOOL && lit.k != Lit::NUL) || (o.has_fallback && fb.k != Lit::BOOL && fb.k != Lit::NUL))
        return set_error(DQ_E_UNSUPPORTED, "boolean column compared with a non-boolean literal");
      if (lit.k == Lit::BOOL) lit.k = Lit::INT;
      if (fb.k == Lit::BOOL) fb.k = Lit::INT;
    } else {
      const bool fb_wide = o.has_fallback && (fb.k == Lit::DBL || (fb.k == Lit::DEC && cd.type == DQ_TYPE_F32));
      const bool dbl_operand = cd.type == DQ_TYPE_F64 || fb_wide;
      auto widen = [](Lit& l, bool in_float) {  // an integer or decimal literal as the double it compares as
        if (l.k != Lit::INT && l.k != Lit::DEC) return;
        l.d = in_float && l.k == Lit::INT ? int_as_float(l.i) : lit_to_double(l);
        l.k = Lit::DBL;
      };
      if (is_floating(cd.type) || dbl_operand) {
        if (o.has_fallback) widen(fb, cd.type == DQ_TYPE_F32);
        widen(lit, cd.type == DQ_TYPE_F32 && !dbl_operand);
      }
    }
    p.null_res = o.has_fallback ? lit_cmp_result(cmp, fb, lit) : NR_NULL;
    if (lit.k == Lit::NUL) { push_const(NR_NULL); return DQ_OK; }
    if (lit.k == Lit::BOOL) return set_error(DQ_E_UNSUPPORTED, "boolean literal compared with a number");
    if (is_floating(cd.type) || lit.k == Lit::DBL) {
      p.ctype = CT_DBL; p.cmp = to_cmpop(cmp); p.lit_d = lit_to_double(lit);
    } else if (lit.k == Lit::INT || (lit.k == Lit::DEC && lit.scale == 0)) {
      p.ctype = CT_INT; p.cmp = to_cmpop(cmp); p.lit_i = lit.i;
    } else {
      // integral column vs decimal literal v = u / 10^s: exact rewrite to integer bounds
      int64_t p10;
      pow10_i64(lit.scale, p10);
      int64_t u = lit.i;
      int64_t fl = floor_div(u, p10);
      bool integral = (u % p10) == 0;
      int64_t ce = integral ? fl : fl + 1;                      // ceil
      p.ctype = CT_INT;
      switch (cmp) {
        case DQ_CMP_LT: p.cmp = C_LT; p.lit_i = ce; break;      // x < v  <=> x < ceil(v)
        case DQ_CMP_LE: p.cmp = C_LE; p.lit_i = fl; break;      // x <= v <=> x <= floor(v)
        case DQ_CMP_GT: p.cmp = C_GT; p.lit_i = fl; break;      // x > v  <=> x > floor(v)
        case DQ_CMP_GE: p.cmp = C_GE; p.lit_i = ce; break;      // x >= v <=> x >= ceil(v)
        case DQ_CMP_EQ: p.cmp = integral ? C_EQ : C_FALSE; p.lit_i = fl; break;
        default: p.cmp = integral ? C_NE : C_TRUE; p.lit_i = fl; break;
      }
    }
    out.push_back(p);
    return DQ_OK;
  }

  dq_status lower(int32_t idx, int depth) {
    if (dq_status s = check_idx(idx)) return s;
    if (depth > 30) return set_error(DQ_E_UNSUPPORTED, "predicate nesting too deep");
    const dq_pred_node& n = pool[idx];
    switch (n.kind) {
      case DQ_PRED_AND:
      case DQ_PRED_OR: {
        if (dq_status s = lower(n.a, depth + 1)) return s;
        if (dq_status s = lower(n.b, depth + 1)) return s;
        PredInstr p{};
        p.op = n.kind == DQ_PRED_AND ? PO_AND : PO_OR; p.col_a = p.col_b = -1;
        out.push_back(p);
        return DQ_OK;
      }
      case DQ_PRED_NOT: {
        if (dq_status s = lower(n.a, depth + 1)) return s;
        PredInstr p{};
        p.op = PO_NOT; p.col_a = p.col_b = -1;
        out.push_back(p);
        return DQ_OK;
      }
      case DQ_PRED_REGEX: {  // PatternMatch.scala:48-49 / RLIKE on a string column
        if (dq_status s = check_idx(n.a)) return s;
        const dq_pred_node& c = pool[n.a];
        if (c.kind != DQ_PRED_COLUMN) return set_error(DQ_E_UNSUPPORTED, "regex on a non-column expression");
        if (dq_status s = check_col(c.a)) return s;
        const int32_t t = (*schema)[c.a].type;
        if (t != DQ_TYPE_UTF8 && t != DQ_TYPE_LARGE_UTF8)
          return set_error(DQ_E_UNSUPPORTED, "regex on a non-string column (%d)", c.a);
        if (n.cmp != DQ_REGEX_RLIKE && n.cmp != DQ_REGEX_EXTRACT_NONEMPTY && n.cmp != DQ_REGEX_FULL)
          return set_error(DQ_E_INVALID, "regex mode %d", n.cmp);
        if (!patterns || n.i64 < 0 || n.i64 >= (int64_t)patterns->size())
          return set_error(DQ_E_INVALID, "regex pattern index %lld out of range", (long long)n.i64);
        auto key = std::make_pair(n.i64, n.cmp);
        auto it = regex_at.find(key);
        int64_t off;
        if (it != regex_at.end()) {
          off = it->second;
        } else {
          RegexDfa d;
          if (dq_status s = regex_compile((*patterns)[n.i64].c_str(), n.cmp, d)) return s;
          off = (int64_t)regex_blob->size();
          regex_serialize(d, *regex_blob);
          regex_at[key] = off;
        }
        PredInstr p{};
        p.op = PO_ATOM_REGEX; p.col_a = c.a; p.col_b = -1; p.kind_a = kind_of(t);
        p.lit_i = off;
        p.null_res = n.cmp == DQ_REGEX_EXTRACT_NONEMPTY ? NR_FALSE : NR_NULL;
        out.push_back(p);
        return DQ_OK;
      }
      case DQ_PRED_IS_NULL:
      case DQ_PRED_IS_NOT_NULL: {
        if (dq_status s = check_idx(n.a)) return s;
        const dq_pred_node& c = pool[n.a];
        bool isnull = n.kind == DQ_PRED_IS_NULL;
        if (c.kind == DQ_PRED_COLUMN) {
          if (dq_status s = check_col(c.a)) return s;
          PredInstr p{};
          p.op = isnull ? PO_ATOM_ISNULL : PO_ATOM_NOTNULL; p.col_a = c.a; p.col_b = -1;
          out.push_back(p);
          return DQ_OK;
        }
        if (is_lit(n.a)) {
          bool lit_null = c.kind == DQ_PRED_LIT_NULL;
          push_const((lit_null == isnull) ? NR_TRUE : NR_FALSE);
          return DQ_OK;
        }
        if (c.kind == DQ_PRED_COALESCE && is_lit(c.b) && pool[c.b].kind != DQ_PRED_LIT_NULL) {
          push_const(isnull ? NR_FALSE : NR_TRUE);  // COALESCE(col, non-null literal) is never NULL
          return DQ_OK;
        }
        return set_error(DQ_E_UNSUPPORTED, "IS NULL over an unsupported expression");
      }
      case DQ_PRED_LIT_BOOL: push_const(n.i64 ? NR_TRUE : NR_FALSE); return DQ_OK;
      case DQ_PRED_LIT_NULL: push_const(NR_NULL); return DQ_OK;
      case DQ_PRED_COLUMN: {  // a BooleanType column as a predicate: its value (NULL stays NULL), i.e. col = TRUE
        if (dq_status s = check_col(n.a)) return s;
        if ((*schema)[n.a].type != DQ_TYPE_BOOL)
          return set_error(DQ_E_UNSUPPORTED, "column %d is not a boolean expression", n.a);
        PredInstr p{};
        p.op = PO_ATOM_CMP; p.col_a = n.a; p.col_b = -1; p.kind_a = CK_BOOL; p.kind_b = 0;
        p.null_res = NR_NULL; p.ctype = CT_INT; p.cmp = C_EQ; p.lit_i = 1;
        out.push_back(p);
        return DQ_OK;
      }
      case DQ_PRED_CMP: {
        if (dq_status s = check_idx(n.a)) return s;
        if (dq_status s = check_idx(n.b)) return s;
        int cmp = n.cmp;
        if (cmp < DQ_CMP_LT || cmp > DQ_CMP_NE) return set_error(DQ_E_INVALID, "bad comparison op %d", cmp);
        bool la = is_lit(n.a), lb = is_lit(n.b);
        if (la && lb) {
          Lit a, b;
          if (dq_status s = lit_of(n.a, a)) return s;
          if (dq_status s = lit_of(n.b, b)) return s;
          push_const(lit_cmp_result(cmp, a, b));
          return DQ_OK;
        }
        if (la || lb) {
          int32_t oi = la ? n.b : n.a, li = la ? n.a : n.b;
          if (la) cmp = flip_cmp(cmp);
          Operand o;
          Lit l;
          if (dq_status s = operand_of(oi, o)) return s;
          if (dq_status s = lit_of(li, l)) return s;
          return emit_col_lit(o, cmp, l);
        }
        // column vs column
        if (pool[n.a].kind != DQ_PRED_COLUMN || pool[n.b].kind != DQ_PRED_COLUMN)
          return set_error(DQ_E_UNSUPPORTED, "comparison of two non-column expressions");
        int32_t ca = pool[n.a].a, cb = pool[n.b].a;
        if (dq_status s = check_col(ca)) return s;
        if (dq_status s = check_col(cb)) return s;
        int32_t ta = (*schema)[ca].type, tb = (*schema)[cb].type;
        const bool bools = ta == DQ_TYPE_BOOL && tb == DQ_TYPE_BOOL;
        if (!bools && (!is_numeric(ta) || !is_numeric(tb)))
          return set_error(DQ_E_UNSUPPORTED, "comparison of non-numeric columns");
        if (is_decimal(ta) || is_decimal(tb))
          return set_error(DQ_E_UNSUPPORTED, "comparison of a decimal column with a column");
        // FloatType vs Int / LongType compares in FloatType (the integer rounded to float), which a double
        // compare does not restate for integers beyond 2^24: the fallback (ShortType / ByteType are exact)
        auto wide_int = [](int32_t t) { return t == DQ_TYPE_I32 || t == DQ_TYPE_I64; };
        if ((ta == DQ_TYPE_F32 && wide_int(tb)) || (tb == DQ_TYPE_F32 && wide_int(ta)))
          return set_error(DQ_E_UNSUPPORTED, "float column compared with an int / long column");
        PredInstr p{};
        p.op = PO_ATOM_CMP; p.col_a = ca; p.col_b = cb; p.kind_a = kind_of(ta); p.kind_b = kind_of(tb);
        p.null_res = NR_NULL; p.cmp = to_cmpop(cmp);
        p.ctype = bools || (is_integral(ta) && is_integral(tb)) ? CT_INT : CT_DBL;
        out.push_back(p);
        return DQ_OK;
      }
      default:
        return set_error(DQ_E_UNSUPPORTED, "predicate node kind %d is not a boolean expression", n.kind);
    }
  }
};

// canonical text of a predicate subtree (dedup of roots)
static std::string canon(const dq_pred_node* pool, int32_t n_pred, int32_t idx, int depth = 0) {
  if (idx < 0 || idx >= n_pred || depth > 64) return "?";
  const dq_pred_node& n = pool[idx];
  char buf[128];
  std::snprintf(buf, sizeof(buf), "(%d:%d:%lld:%a", n.kind, n.cmp, (long long)n.i64, n.f64);
  std::string s = buf;
  if (n.kind == DQ_PRED_COLUMN) s += ":c" + std::to_string(n.a);
  else {
    if (n.kind == DQ_PRED_CMP || n.kind == DQ_PRED_AND || n.kind == DQ_PRED_OR || n.kind == DQ_PRED_NOT ||
        n.kind == DQ_PRED_IS_NULL || n.kind == DQ_PRED_IS_NOT_NULL || n.kind == DQ_PRED_COALESCE ||
        n.kind == DQ_PRED_REGEX)
      s += canon(pool, n_pred, n.a, depth + 1);
    if (n.kind == DQ_PRED_CMP || n.kind == DQ_PRED_AND || n.kind == DQ_PRED_OR || n.kind == DQ_PRED_COALESCE)
      s += canon(pool, n_pred, n.b, depth + 1);
  }
  return s + ")";
}

// ------------------------------------------------------------------------------------------
// PredBuilder
// ------------------------------------------------------------------------------------------
PredBuilder::PredBuilder(const dq_pred_node* pool, int32_t n_pred, const std::vector<dq_column_desc>* schema,
                         const std::vector<std::string>* patterns, std::vector<uint16_t>* regex_blob)
    : low_(new Lowering{pool, n_pred, schema, {}}) {
  low_->patterns = patterns;
  low_->regex_blob = regex_blob;
}
PredBuilder::~PredBuilder() = default;

dq_status PredBuilder::over(PredLimit l, size_t value) {
  limit = l;
  limit_value = value;
  return DQ_E_UNSUPPORTED;
}

// the slot of root `key`: the one it has, or the next one, its code (`atom`, or else node's lowering) and STORE appended
dq_status PredBuilder::add(const std::string& key, int32_t node, const PredInstr* atom, int32_t& slot) {
  auto it = root_slot_.find(key);
  if (it != root_slot_.end()) { slot = it->second; return DQ_OK; }
  if (n_roots() >= kMaxRoots) return over(PL_ROOTS, kMaxRoots);
  low_->out.clear();
  if (atom) low_->out.push_back(*atom);
  else if (dq_status s = low_->lower(node, 0)) return s;
  slot = n_roots();
  root_slot_[key] = slot;
  code_.insert(code_.end(), low_->out.begin(), low_->out.end());
  PredInstr st{};
  st.op = PO_STORE; st.slot = slot; st.col_a = st.col_b = -1;
  code_.push_back(st);
  return DQ_OK;
}

dq_status PredBuilder::root(int32_t node, int32_t& slot) {
  if (node < 0 || node >= low_->n_pred) return set_error(DQ_E_INVALID, "predicate root %d out of range", node);
  return add(canon(low_->pool, low_->n_pred, node), node, nullptr, slot);
}

dq_status PredBuilder::notnull_root(int32_t col, int32_t& slot) {
  PredInstr ins{};
  ins.op = PO_ATOM_NOTNULL; ins.col_a = col; ins.col_b = -1;
  return add("notnull:" + std::to_string(col), -1, &ins, slot);
}

dq_status PredBuilder::assemble(PredProgram& prog) {
  if ((int32_t)code_.size() > kMaxInstr) return over(PL_INSTR, code_.size());
  int depth = 0, max_depth = 0;
  for (const PredInstr& ins : code_) {
    depth += (ins.op == PO_AND || ins.op == PO_OR || ins.op == PO_STORE) ? -1 : (ins.op == PO_NOT ? 0 : 1);
    max_depth = std::max(max_depth, depth);
  }
  if (max_depth > kPredStack) return over(PL_STACK, (size_t)max_depth);
  if (low_->regex_blob->size() > (size_t)kMaxRegexWords) return over(PL_REGEX, low_->regex_blob->size());
  prog.regex_words = (int32_t)low_->regex_blob->size();
  prog.stack_depth = std::max(1, max_depth);
  prog.n_roots = n_roots();
  prog.n_instr = (int32_t)code_.size();
  std::copy(code_.begin(), code_.end(), prog.instr);
  prog.n_loads = 0;
  for (int32_t i = 0; i < prog.n_instr; ++i)
    if (prog.instr[i].op == PO_ATOM_CMP || prog.instr[i].op == PO_ATOM_ISNULL || prog.instr[i].op == PO_ATOM_NOTNULL ||
        prog.instr[i].op == PO_ATOM_REGEX)
      prog.load_instr[prog.n_loads++] = (int16_t)i;
  return DQ_OK;
}

}  // namespace dq
