// dq_pred_compile.cpp -- Spark SQL predicate text -> the dq_pred_node IR (include/dqscan.h), on the host.
//
// Stands in for Spark's expr(...) parser at the C boundary: the predicate strings deequ builds
// (analyzers/Analyzer.scala:385-408 `where` filters; checks/Check.scala:538-548, 670-871 satisfies /
// isNonNegative / isContainedIn / isLessThan ...) are parsed here, so a JVM / JNI shim hands over the
// text and gets exactly the lowering the tests pin.  Grammar (the numeric subset the GPU evaluates with
// SQL three-valued logic, plus string equality / IN lists on string columns):
//
//     expr     := or
//     or       := and ( OR and )*
//     and      := not ( AND not )*
//     not      := NOT not | cmp
//     cmp      := operand ( (< | <= | > | >= | = | == | != | <>) operand | IS [NOT] NULL
//                           | [NOT] IN ('s', ...) )?
//     operand  := sum
//     sum      := term ( (+ | -) term )*
//     term     := unary ( (* | / | %) unary )*
//     unary    := - unary | primary
//     primary  := column | `column` | number | - number | NULL | TRUE | FALSE | 'string'
//               | COALESCE(primary, primary) | ( expr )      (COALESCE also takes `- number`)
//
// A sum that is one primary lowers as it always did.  One with an operator and a column becomes a DQ_PRED_EXPR node
// over a postfix dq_expr_program (include/dqscan.h states the Spark 2.2 typing and the refusals): the caller
// materialises it as a derived column, so the plan and its kernels never see arithmetic.
// Literal typing follows Spark 2.2: `3` integer, `3.0` exact decimal (unscaled int64 + scale), `3e0`
// double.  String (in)equality and IN lists compare the UTF-8 bytes of a string column with the literals:
// they lower to a whole-value DFA (DQ_PRED_REGEX, mode DQ_REGEX_FULL) over the escaped literals.  Anything
// else -- string ordering, numeric comparison of a string column, LIKE / RLIKE / BETWEEN, function calls,
// typed literal suffixes, backslash escapes in literals -- is DQ_E_UNSUPPORTED: the analyzer is routed to
// the fallback set, as a column type the plan does not cover.
#include <cerrno>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dqscan.h"
#include "dq_internal.h"

struct dq_pred_pool {
  std::vector<std::string> names;
  std::vector<int32_t> types;
  std::unordered_map<std::string, int32_t> index;
  std::vector<dq_pred_node> nodes;
  std::vector<std::string> patterns;
  std::vector<const char*> pattern_ptrs;
  struct Expr {
    std::string text;  // canonical
    dq_expr_program prog;
  };
  std::vector<std::unique_ptr<Expr>> exprs;
};

namespace {

struct PredError {
  dq_status status;
  std::string msg;
};

[[noreturn]] void unsupported(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw PredError{DQ_E_UNSUPPORTED, buf};
}

enum TokKind { T_ID, T_STR, T_NUM, T_KW, T_OP, T_END };
struct Tok {
  TokKind kind;
  std::string text;
  bool operator==(const Tok& o) const { return kind == o.kind && text == o.text; }
};

const char* const kKeywords[] = {"AND", "OR", "NOT", "IS", "NULL", "COALESCE", "TRUE", "FALSE", "IN", "LIKE", "RLIKE",
                                 "BETWEEN"};

bool is_digit(char c) { return c >= '0' && c <= '9'; }
bool is_alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (unsigned char)c >= 0x80; }
bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

std::string upper(const std::string& s) {
  std::string u = s;
  for (char& c : u)
    if (c >= 'a' && c <= 'z') c = (char)(c - 'a' + 'A');
  return u;
}

std::vector<Tok> tokenize(const std::string& s) {
  std::vector<Tok> toks;
  size_t i = 0;
  const char* q = s.c_str();
  while (i < s.size()) {
    const char c = s[i];
    if (is_space(c)) {
      ++i;
    } else if (c == '`') {
      const size_t j = s.find('`', i + 1);
      if (j == std::string::npos) unsupported("unterminated identifier in '%s'", q);
      toks.push_back({T_ID, s.substr(i + 1, j - i - 1)});
      i = j + 1;
    } else if (c == '\'' || c == '"') {
      const size_t j = s.find(c, i + 1);
      if (j == std::string::npos) unsupported("unterminated string literal in '%s'", q);
      const std::string body = s.substr(i + 1, j - i - 1);
      if (body.find('\\') != std::string::npos)  // Spark unescapes backslash sequences: not restated here
        unsupported("string literal with a backslash escape in '%s'", q);
      toks.push_back({T_STR, body});
      i = j + 1;
    } else if (is_digit(c) || (c == '.' && i + 1 < s.size() && is_digit(s[i + 1]))) {
      size_t j = i;
      while (j < s.size() && (is_digit(s[j]) || s[j] == '.')) ++j;
      if (j < s.size() && (s[j] == 'e' || s[j] == 'E')) {
        ++j;
        if (j < s.size() && (s[j] == '+' || s[j] == '-')) ++j;
        while (j < s.size() && is_digit(s[j])) ++j;
      }
      if (j < s.size() && std::strchr("dDlLsSyY", s[j]) && s[j] != '\0')  // typed literal suffixes (1.0D, 10L)
        unsupported("typed literal suffix in '%s'", q);
      toks.push_back({T_NUM, s.substr(i, j - i)});
      i = j;
    } else if (is_alpha(c) || c == '_') {
      size_t j = i;
      while (j < s.size() && (is_alpha(s[j]) || is_digit(s[j]) || s[j] == '_')) ++j;
      const std::string w = s.substr(i, j - i), u = upper(w);
      bool kw = false;
      for (const char* k : kKeywords) kw = kw || u == k;
      toks.push_back(kw ? Tok{T_KW, u} : Tok{T_ID, w});
      i = j;
    } else if (s.compare(i, 2, "<=") == 0 || s.compare(i, 2, ">=") == 0 || s.compare(i, 2, "!=") == 0 ||
               s.compare(i, 2, "<>") == 0 || s.compare(i, 2, "==") == 0) {
      toks.push_back({T_OP, s.substr(i, 2)});
      i += 2;
    } else if (std::strchr("<>=(),-+*/%", c) && c != '\0') {
      toks.push_back({T_OP, std::string(1, c)});
      ++i;
    } else {
      unsupported("unexpected character '%c' in '%s'", c, q);
    }
  }
  return toks;
}

int32_t cmp_of(const std::string& op) {
  if (op == "<") return DQ_CMP_LT;
  if (op == "<=") return DQ_CMP_LE;
  if (op == ">") return DQ_CMP_GT;
  if (op == ">=") return DQ_CMP_GE;
  if (op == "=" || op == "==") return DQ_CMP_EQ;
  if (op == "!=" || op == "<>") return DQ_CMP_NE;
  return 0;
}

// An arithmetic operand before it is lowered: leaves are columns and literals, inner nodes dq_expr_op operators.
struct Ast {
  int32_t op = 0;         // DQ_EXPR_COL / DQ_EXPR_LIT leaf, DQ_EXPR_NEG (l), DQ_EXPR_ADD .. DQ_EXPR_MOD (l, r)
  int32_t col = -1;       // COL: position in the pool's column list
  int32_t lit_kind = 0;   // LIT: DQ_PRED_LIT_INT / _DECIMAL / _DOUBLE
  int32_t scale = 0;      // LIT decimal
  int64_t i64 = 0;
  double f64 = 0.0;
  int32_t type = 0;       // enum dq_type, set by Parser::type_of (0 for a decimal literal not yet placed)
  std::shared_ptr<Ast> l, r;
};
using AstP = std::shared_ptr<Ast>;

// An operand: a node index, or (string literals) the literal text, valid only beside a string column, or an
// arithmetic expression that its consumer (a comparison, IS [NOT] NULL) lowers to a DQ_PRED_EXPR node.
struct Operand {
  int32_t node = -1;
  bool is_str = false;
  std::string str;
  AstP ast;
};

int type_rank(int32_t t) {  // Byte < Short < Int < Long < Float < Double; 0: not a type arithmetic takes
  switch (t) {
    case DQ_TYPE_I8: return 1;
    case DQ_TYPE_I16: return 2;
    case DQ_TYPE_I32: return 3;
    case DQ_TYPE_I64: return 4;
    case DQ_TYPE_F32: return 5;
    case DQ_TYPE_F64: return 6;
    default: return 0;
  }
}

class Parser {
 public:
  Parser(dq_pred_pool& pool, const std::string& text) : P(pool), text(text), toks(tokenize(text)) {}

  int32_t parse() {
    const Operand r = parse_or();
    if (pos != toks.size()) unsupported("unsupported syntax near '%s' in '%s'", toks[pos].text.c_str(), text.c_str());
    return need_node(r);
  }

 private:
  dq_pred_pool& P;
  const std::string& text;
  std::vector<Tok> toks;
  size_t pos = 0;

  Tok peek() const { return pos < toks.size() ? toks[pos] : Tok{T_END, ""}; }
  Tok take() {
    Tok t = peek();
    ++pos;
    return t;
  }
  void expect(TokKind k, const char* v) {
    const Tok t = take();
    if (!(t.kind == k && t.text == v)) unsupported("expected '%s', got '%s' in '%s'", v, t.text.c_str(), text.c_str());
  }
  bool at(TokKind k, const char* v) const {
    const Tok t = peek();
    return t.kind == k && t.text == v;
  }
  int32_t add(int32_t kind, int32_t a = -1, int32_t b = -1, int32_t cmp = 0, int64_t i64 = 0, double f64 = 0.0) {
    P.nodes.push_back(dq_pred_node{kind, a, b, cmp, i64, f64});
    return (int32_t)P.nodes.size() - 1;
  }
  Operand node(int32_t n) {
    Operand o;
    o.node = n;
    return o;
  }
  int32_t need_node(const Operand& o) {
    if (o.is_str) unsupported("bare string literal in '%s'", text.c_str());
    if (o.ast) unsupported("arithmetic expression used as a boolean or as an argument in '%s'", text.c_str());
    return o.node;
  }

  Operand parse_or() {
    Operand a = parse_and();
    while (at(T_KW, "OR")) {
      take();
      const int32_t l = need_node(a);
      const int32_t r = need_node(parse_and());
      a = node(add(DQ_PRED_OR, l, r));
    }
    return a;
  }
  Operand parse_and() {
    Operand a = parse_not();
    while (at(T_KW, "AND")) {
      take();
      const int32_t l = need_node(a);
      const int32_t r = need_node(parse_not());
      a = node(add(DQ_PRED_AND, l, r));
    }
    return a;
  }
  Operand parse_not() {
    if (at(T_KW, "NOT")) {
      take();
      return node(add(DQ_PRED_NOT, need_node(parse_not())));
    }
    return parse_cmp();
  }

  // plan column of a COLUMN node or of COALESCE(column, ...); -1 otherwise
  int32_t column_of(int32_t n) const {
    const dq_pred_node& x = P.nodes[(size_t)n];
    if (x.kind == DQ_PRED_COLUMN) return x.a;
    if (x.kind == DQ_PRED_COALESCE && P.nodes[(size_t)x.a].kind == DQ_PRED_COLUMN) return P.nodes[(size_t)x.a].a;
    return -1;
  }
  bool is_string_col(int32_t col) const {
    return col >= 0 && (P.types[(size_t)col] == DQ_TYPE_UTF8 || P.types[(size_t)col] == DQ_TYPE_LARGE_UTF8);
  }

  Operand parse_cmp() {
    Operand a = parse_sum();
    const Tok t = peek();
    if (t.kind == T_OP && cmp_of(t.text)) {
      take();
      Operand b = parse_sum();
      if ((a.is_str || b.is_str) && (a.ast || b.ast))
        unsupported("string literal compared with an arithmetic expression in '%s'", text.c_str());
      if (a.ast) a = node(lower(a.ast));
      if (b.ast) b = node(lower(b.ast));
      if (a.is_str || b.is_str) {  // string (in)equality
        if (t.text != "=" && t.text != "==" && t.text != "!=" && t.text != "<>")
          unsupported("string ordering comparison in '%s'", text.c_str());
        const Operand& col = a.is_str ? b : a;
        const Operand& lit = a.is_str ? a : b;
        if (col.is_str) unsupported("comparison of two string literals in '%s'", text.c_str());
        const int32_t e = string_in(col.node, {lit.str});
        return node(t.text == "!=" || t.text == "<>" ? add(DQ_PRED_NOT, e) : e);
      }
      // numeric comparison: a string column operand is outside the grammar (Spark would cast it)
      for (int32_t side : {a.node, b.node}) {
        const int32_t c = column_of(side);
        if (is_string_col(c))
          unsupported("predicate compares string column '%s' in '%s'", P.names[(size_t)c].c_str(), text.c_str());
      }
      return node(add(DQ_PRED_CMP, a.node, b.node, cmp_of(t.text)));
    }
    if (!a.is_str && (at(T_KW, "IN") || at(T_KW, "NOT"))) {
      const size_t save = pos;
      const bool neg = at(T_KW, "NOT");
      take();
      if (neg && !at(T_KW, "IN")) {
        pos = save;
        return a;
      }
      if (neg) take();
      if (a.ast) unsupported("IN over an arithmetic expression in '%s'", text.c_str());
      expect(T_OP, "(");
      std::vector<Tok> items{take()};
      while (at(T_OP, ",")) {
        take();
        items.push_back(take());
      }
      expect(T_OP, ")");
      std::vector<std::string> lits;
      for (const Tok& it : items) {
        if (it.kind != T_STR) unsupported("IN list of non-string literals in '%s'", text.c_str());
        lits.push_back(it.text);
      }
      const int32_t e = string_in(a.node, lits);
      return node(neg ? add(DQ_PRED_NOT, e) : e);
    }
    if (at(T_KW, "IS")) {
      take();
      bool neg = false;
      if (at(T_KW, "NOT")) {
        take();
        neg = true;
      }
      expect(T_KW, "NULL");
      if (a.ast) a = node(lower(a.ast));
      return node(add(neg ? DQ_PRED_IS_NOT_NULL : DQ_PRED_IS_NULL, need_node(a)));
    }
    if (t.kind == T_KW && (t.text == "LIKE" || t.text == "RLIKE" || t.text == "BETWEEN"))
      unsupported("%s is not in the GPU predicate grammar: '%s'", t.text.c_str(), text.c_str());
    if (a.is_str) unsupported("bare string literal in '%s'", text.c_str());
    return a;
  }

  // col IN (literals) as one whole-value DFA (?:l1|l2|...) with every non-alphanumeric ASCII character
  // escaped (the DFA compiler reads `\` + such a character as the literal character)
  int32_t string_in(int32_t col_node, const std::vector<std::string>& lits) {
    const dq_pred_node cn = P.nodes[(size_t)col_node];
    if (cn.kind != DQ_PRED_COLUMN) unsupported("string comparison on a non-column expression in '%s'", text.c_str());
    if (!is_string_col(cn.a)) unsupported("string literal compared with a non-string column in '%s'", text.c_str());
    std::string pat = "(?:";
    for (size_t i = 0; i < lits.size(); ++i) {
      if (i) pat += '|';
      for (char ch : lits[i]) {
        const unsigned char u = (unsigned char)ch;
        if (!((u < 128 && (is_digit(ch) || (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z'))) || u >= 128))
          pat += '\\';
        pat += ch;
      }
    }
    pat += ')';
    if (col_node == (int32_t)P.nodes.size() - 1) P.nodes.pop_back();  // re-added by add_regex
    int32_t root = -1;
    const dq_status s = dq_pred_pool_add_regex(&P, cn.a, pat.c_str(), DQ_REGEX_FULL, &root);
    if (s != DQ_OK) throw PredError{s, dq_last_error()};
    return root;
  }

  // ---- arithmetic operands -------------------------------------------------------------------------------------
  // The leaf nodes of a sum with an operator were appended to the pool while its primaries were parsed; the sum
  // takes them back (the pool holds only the DQ_PRED_EXPR node its consumer appends).
  Operand parse_sum() {
    const size_t n0 = P.nodes.size();
    Operand a = parse_term();
    while (at(T_OP, "+") || at(T_OP, "-")) {
      const int32_t op = take().text == "+" ? DQ_EXPR_ADD : DQ_EXPR_SUB;
      const AstP l = as_ast(a);
      a = binary(op, l, as_ast(parse_term()));
    }
    if (a.ast) P.nodes.resize(n0);
    return a;
  }
  Operand parse_term() {
    Operand a = parse_unary();
    while (at(T_OP, "*") || at(T_OP, "/") || at(T_OP, "%")) {
      const std::string o = take().text;
      const AstP l = as_ast(a);
      a = binary(o == "*" ? DQ_EXPR_MUL : o == "/" ? DQ_EXPR_DIV : DQ_EXPR_MOD, l, as_ast(parse_unary()));
    }
    return a;
  }
  Operand parse_unary() {
    if (!at(T_OP, "-")) return parse_operand();
    take();
    if (peek().kind == T_NUM) return node(number("-" + take().text));  // `- number` is a literal
    if (++minus_depth > 64) unsupported("unary minus nested too deeply in '%s'", text.c_str());
    const AstP x = as_ast(parse_unary());
    --minus_depth;
    Operand o;
    o.ast = std::make_shared<Ast>();
    o.ast->op = DQ_EXPR_NEG;
    o.ast->l = x;
    return o;
  }
  int minus_depth = 0;

  Operand binary(int32_t op, const AstP& l, const AstP& r) {
    Operand o;
    o.ast = std::make_shared<Ast>();
    o.ast->op = op;
    o.ast->l = l;
    o.ast->r = r;
    return o;
  }

  // an operand of an arithmetic operator: an expression as it is, a column or numeric literal node as a leaf
  AstP as_ast(const Operand& o) {
    if (o.ast) return o.ast;
    if (o.is_str) unsupported("string operand of an arithmetic operator in '%s'", text.c_str());
    const dq_pred_node& x = P.nodes[(size_t)o.node];
    AstP a = std::make_shared<Ast>();
    switch (x.kind) {
      case DQ_PRED_COLUMN: {
        const int32_t t = P.types[(size_t)x.a];
        const char* name = P.names[(size_t)x.a].c_str();
        if (DQ_TYPE_BASE(t) == DQ_TYPE_DECIMAL128)
          unsupported("decimal column '%s' inside arithmetic in '%s'", name, text.c_str());
        if (!type_rank(t)) unsupported("non-numeric column '%s' inside arithmetic in '%s'", name, text.c_str());
        a->op = DQ_EXPR_COL;
        a->col = x.a;
        a->type = t;
        return a;
      }
      case DQ_PRED_LIT_INT:
      case DQ_PRED_LIT_DECIMAL:
      case DQ_PRED_LIT_DOUBLE:
        a->op = DQ_EXPR_LIT;
        a->lit_kind = x.kind;
        a->i64 = x.i64;
        a->f64 = x.f64;
        a->scale = x.cmp;
        return a;
      case DQ_PRED_LIT_NULL: unsupported("NULL inside arithmetic in '%s'", text.c_str());
      case DQ_PRED_LIT_BOOL: unsupported("boolean operand of an arithmetic operator in '%s'", text.c_str());
      case DQ_PRED_COALESCE: unsupported("COALESCE inside arithmetic in '%s'", text.c_str());
      default: unsupported("boolean operand of an arithmetic operator in '%s'", text.c_str());
    }
  }

  // The Spark type of every node.  A decimal literal has a type only beside a Float / Double operand (it is cast
  // to Double); anywhere else the operation would be decimal arithmetic.
  bool is_decimal_lit(const AstP& a) const { return a->op == DQ_EXPR_LIT && a->lit_kind == DQ_PRED_LIT_DECIMAL; }
  int32_t type_of(const AstP& a) {
    switch (a->op) {
      case DQ_EXPR_COL: return a->type;
      case DQ_EXPR_LIT:
        if (a->lit_kind == DQ_PRED_LIT_DOUBLE) a->type = DQ_TYPE_F64;
        else if (a->lit_kind == DQ_PRED_LIT_INT) a->type = a->i64 >= INT32_MIN && a->i64 <= INT32_MAX ? DQ_TYPE_I32 : DQ_TYPE_I64;
        else unsupported("decimal literal outside a Float / Double operation (decimal arithmetic) in '%s'", text.c_str());
        return a->type;
      case DQ_EXPR_NEG: return a->type = type_of(a->l);
      default: break;
    }
    int32_t tl, tr;
    if (is_decimal_lit(a->l) && is_decimal_lit(a->r))
      unsupported("arithmetic on two decimal literals (decimal arithmetic) in '%s'", text.c_str());
    if (is_decimal_lit(a->l) || is_decimal_lit(a->r)) {
      const AstP& lit = is_decimal_lit(a->l) ? a->l : a->r;
      const int32_t other = type_of(is_decimal_lit(a->l) ? a->r : a->l);
      if (other != DQ_TYPE_F32 && other != DQ_TYPE_F64)
        unsupported("decimal literal combined with an integral operand (decimal arithmetic) in '%s'", text.c_str());
      // the literal's double: its digits read as a double are the correctly rounded value of unscaled / 10^scale
      char buf[64];
      std::snprintf(buf, sizeof(buf), "%lldE-%d", (long long)lit->i64, (int)lit->scale);
      lit->f64 = std::strtod(buf, nullptr);
      lit->lit_kind = DQ_PRED_LIT_DOUBLE;
      lit->type = DQ_TYPE_F64;
      tl = a->l == lit ? DQ_TYPE_F64 : other;
      tr = a->r == lit ? DQ_TYPE_F64 : other;
    } else {
      tl = type_of(a->l);
      tr = type_of(a->r);
    }
    a->type = a->op == DQ_EXPR_DIV ? DQ_TYPE_F64 : (type_rank(tl) >= type_rank(tr) ? tl : tr);
    return a->type;
  }

  struct Emit {
    dq_expr_program p{};
    int depth = 0;
    std::string why;
  };
  void push_instr(Emit& e, int32_t op, int32_t arg, int32_t type, int delta) {
    if (e.p.n_instrs >= DQ_EXPR_MAX_INSTRS)
      unsupported("arithmetic expression longer than %d instructions in '%s'", DQ_EXPR_MAX_INSTRS, text.c_str());
    e.p.instrs[e.p.n_instrs++] = dq_expr_instr{op, arg, type, 0};
    e.depth += delta;
    if (e.depth > DQ_EXPR_MAX_STACK)
      unsupported("arithmetic expression nested deeper than a %d-entry value stack in '%s'", DQ_EXPR_MAX_STACK, text.c_str());
    if (e.depth > e.p.stack_depth) e.p.stack_depth = e.depth;
  }
  void emit(Emit& e, const AstP& a, int32_t want) {
    switch (a->op) {
      case DQ_EXPR_COL: {
        int32_t k = 0;
        while (k < e.p.n_columns && e.p.columns[k] != a->col) ++k;
        if (k == e.p.n_columns) {
          if (k >= DQ_EXPR_MAX_COLUMNS)
            unsupported("arithmetic expression over more than %d columns in '%s'", DQ_EXPR_MAX_COLUMNS, text.c_str());
          e.p.columns[k] = a->col;
          e.p.column_types[k] = a->type;
          ++e.p.n_columns;
        }
        push_instr(e, DQ_EXPR_COL, k, a->type, 1);
        break;
      }
      case DQ_EXPR_LIT: {
        if (e.p.n_literals >= DQ_EXPR_MAX_LITERALS)
          unsupported("arithmetic expression with more than %d literals in '%s'", DQ_EXPR_MAX_LITERALS, text.c_str());
        const bool dbl = a->type == DQ_TYPE_F64;
        e.p.literals[e.p.n_literals] = dq_expr_literal{a->type, 0, dbl ? 0 : a->i64, dbl ? a->f64 : 0.0};
        push_instr(e, DQ_EXPR_LIT, e.p.n_literals++, a->type, 1);
        break;
      }
      case DQ_EXPR_NEG:
        emit(e, a->l, a->type);
        push_instr(e, DQ_EXPR_NEG, 0, a->type, 0);
        break;
      default: {
        emit(e, a->l, a->type);
        emit(e, a->r, a->type);
        push_instr(e, a->op, 0, a->type, -1);
        if (a->op == DQ_EXPR_DIV || a->op == DQ_EXPR_MOD) e.p.divides = 1;
      }
    }
    if (want != a->type) push_instr(e, DQ_EXPR_CAST, 0, want, 0);
  }

  bool has_column(const AstP& a) const {
    return a->op == DQ_EXPR_COL || (a->l && has_column(a->l)) || (a->r && has_column(a->r));
  }
  std::string canonical(const AstP& a) const {
    char buf[64];
    switch (a->op) {
      case DQ_EXPR_COL: return "`" + P.names[(size_t)a->col] + "`";
      case DQ_EXPR_LIT:
        if (a->type != DQ_TYPE_F64) {
          std::snprintf(buf, sizeof(buf), "%lld", (long long)a->i64);
          return buf;
        }
        std::snprintf(buf, sizeof(buf), "%.17g", a->f64);
        return std::strpbrk(buf, "en") ? std::string(buf) : std::string(buf) + "e0";  // (e: exponent, n: inf / nan)
      case DQ_EXPR_NEG: return "(-" + canonical(a->l) + ")";
      default: {
        static const char* const sym[] = {"+", "-", "*", "/", "%"};
        return "(" + canonical(a->l) + " " + sym[a->op - DQ_EXPR_ADD] + " " + canonical(a->r) + ")";
      }
    }
  }

  // the DQ_PRED_EXPR node of an arithmetic operand; equal canonical texts share one entry of the pool
  int32_t lower(const AstP& a) {
    if (!has_column(a)) unsupported("arithmetic on literals alone (no column) in '%s'", text.c_str());
    const int32_t type = type_of(a);
    Emit e;
    emit(e, a, type);
    e.p.result_type = type;
    const std::string canon = canonical(a);
    size_t idx = 0;
    while (idx < P.exprs.size() && P.exprs[idx]->text != canon) ++idx;
    if (idx == P.exprs.size()) {
      P.exprs.push_back(std::make_unique<dq_pred_pool::Expr>());
      P.exprs.back()->text = canon;
      P.exprs.back()->prog = e.p;
      P.exprs.back()->prog.text = P.exprs.back()->text.c_str();
    }
    return add(DQ_PRED_EXPR, (int32_t)idx, -1, type);
  }

  Operand parse_operand() {
    const Tok t = take();
    if (t.kind == T_OP && t.text == "(") {
      Operand e = parse_or();
      expect(T_OP, ")");
      return e;
    }
    if (t.kind == T_NUM) return node(number(t.text));
    if (t.kind == T_STR) {
      Operand o;
      o.is_str = true;
      o.str = t.text;
      return o;
    }
    if (t.kind == T_KW && t.text == "NULL") return node(add(DQ_PRED_LIT_NULL));
    if (t.kind == T_KW && (t.text == "TRUE" || t.text == "FALSE"))
      return node(add(DQ_PRED_LIT_BOOL, -1, -1, 0, t.text == "TRUE" ? 1 : 0));
    if (t.kind == T_KW && t.text == "COALESCE") {
      expect(T_OP, "(");
      const int32_t a = need_node(parse_unary());  // (a primary or `- number`: arithmetic is refused here)
      expect(T_OP, ",");
      const int32_t b = need_node(parse_unary());
      if (at(T_OP, ",")) unsupported("COALESCE with more than two arguments in '%s'", text.c_str());
      expect(T_OP, ")");
      return node(add(DQ_PRED_COALESCE, a, b));
    }
    if (t.kind == T_ID) {
      if (at(T_OP, "(")) unsupported("function call %s(...) in '%s'", t.text.c_str(), text.c_str());
      const auto it = P.index.find(t.text);
      if (it == P.index.end()) throw PredError{DQ_E_INVALID, "no such column: " + t.text};
      return node(add(DQ_PRED_COLUMN, it->second));
    }
    unsupported("unexpected token '%s' in '%s'", t.text.c_str(), text.c_str());
  }

  // Spark 2.2 literal typing: exponent -> double, '.' -> exact decimal (int64 unscaled, scale <= 18),
  // else a 64-bit integer
  int32_t number(const std::string& s) {
    const bool neg = !s.empty() && s[0] == '-';
    const std::string body = neg ? s.substr(1) : s;
    if (body.find_first_of("eE") != std::string::npos) {
      const size_t e = body.find_first_of("eE");
      const std::string mant = body.substr(0, e), ex = body.substr(e + 1);
      const size_t dot = mant.find('.');
      const bool mant_ok = !mant.empty() && mant.find('.', dot == std::string::npos ? 0 : dot + 1) == std::string::npos &&
                           mant != ".";
      const size_t ed = ex.find_first_not_of("+-") == std::string::npos ? ex.size() : ex.find_first_not_of("+-");
      if (!mant_ok || ed > 1 || ed >= ex.size()) unsupported("malformed number %s in '%s'", s.c_str(), text.c_str());
      errno = 0;
      char* end = nullptr;
      const double v = std::strtod(s.c_str(), &end);
      if (end != s.c_str() + s.size()) unsupported("malformed number %s in '%s'", s.c_str(), text.c_str());
      return add(DQ_PRED_LIT_DOUBLE, -1, -1, 0, 0, v);  // an overflow is +-inf, as float() / Double.parseDouble
    }
    const size_t dot = body.find('.');
    if (dot != std::string::npos) {
      const std::string ip = body.substr(0, dot), fp = body.substr(dot + 1);
      if (fp.find('.') != std::string::npos) unsupported("malformed number %s in '%s'", s.c_str(), text.c_str());
      uint64_t u = 0;
      for (char ch : ip + fp) {
        if (u > (UINT64_C(1) << 63) / 10) unsupported("decimal literal %s exceeds 64-bit precision", s.c_str());
        u = u * 10 + (uint64_t)(ch - '0');
      }
      if (u >= (UINT64_C(1) << 63) || fp.size() > 18)
        unsupported("decimal literal %s exceeds 64-bit precision", s.c_str());
      return add(DQ_PRED_LIT_DECIMAL, -1, -1, (int32_t)fp.size(), neg ? -(int64_t)u : (int64_t)u);
    }
    uint64_t u = 0;
    for (char ch : body) {
      if (u > UINT64_MAX / 10 || u * 10 > UINT64_MAX - (uint64_t)(ch - '0'))
        unsupported("integer literal %s out of range", s.c_str());
      u = u * 10 + (uint64_t)(ch - '0');
    }
    if (neg ? u > (UINT64_C(1) << 63) : u >= (UINT64_C(1) << 63)) unsupported("integer literal %s out of range", s.c_str());
    return add(DQ_PRED_LIT_INT, -1, -1, 0, neg ? (int64_t)(0 - u) : (int64_t)u);
  }
};

}  // namespace

extern "C" {

dq_status dq_pred_pool_create(const char* const* names, const int32_t* types, int32_t n_cols, dq_pred_pool** out) {
  if (!out || n_cols < 0 || (n_cols > 0 && (!names || !types)))
    return dq::set_error(DQ_E_INVALID, "dq_pred_pool_create: bad argument");
  dq_pred_pool* p = new dq_pred_pool();
  for (int32_t c = 0; c < n_cols; ++c) {
    if (!names[c]) {
      delete p;
      return dq::set_error(DQ_E_INVALID, "dq_pred_pool_create: NULL column name");
    }
    p->names.push_back(names[c]);
    p->types.push_back(types[c]);
    p->index.emplace(names[c], c);  // the first of duplicate names wins, as a resolver would fail later
  }
  *out = p;
  return DQ_OK;
}

dq_status dq_pred_pool_add(dq_pred_pool* pool, const char* sql, int32_t* root) {
  if (!pool || !sql || !root) return dq::set_error(DQ_E_INVALID, "dq_pred_pool_add: bad argument");
  const size_t n0 = pool->nodes.size(), np0 = pool->patterns.size(), ne0 = pool->exprs.size();
  try {
    const std::string text(sql);
    Parser ps(*pool, text);
    *root = ps.parse();
    return DQ_OK;
  } catch (const PredError& e) {
    pool->nodes.resize(n0);  // the pool is unchanged by a failed add
    pool->patterns.resize(np0);
    pool->pattern_ptrs.resize(np0);
    pool->exprs.resize(ne0);
    return dq::set_error(e.status, "%s", e.msg.c_str());
  }
}

dq_status dq_pred_pool_add_regex(dq_pred_pool* pool, int32_t column, const char* pattern, int32_t mode, int32_t* root) {
  if (!pool || !pattern || !root || column < 0 || column >= (int32_t)pool->names.size())
    return dq::set_error(DQ_E_INVALID, "dq_pred_pool_add_regex: bad argument");
  if (dq_status s = dq_regex_info(pattern, mode, nullptr, nullptr)) return s;  // outside the DFA subset
  int32_t idx = -1;
  for (size_t i = 0; i < pool->patterns.size(); ++i)
    if (pool->patterns[i] == pattern) idx = (int32_t)i;
  if (idx < 0) {
    pool->patterns.push_back(pattern);
    pool->pattern_ptrs.clear();
    for (const std::string& q : pool->patterns) pool->pattern_ptrs.push_back(q.c_str());
    idx = (int32_t)pool->patterns.size() - 1;
  }
  pool->nodes.push_back(dq_pred_node{DQ_PRED_COLUMN, column, -1, 0, 0, 0.0});
  const int32_t col = (int32_t)pool->nodes.size() - 1;
  pool->nodes.push_back(dq_pred_node{DQ_PRED_REGEX, col, -1, mode, idx, 0.0});
  *root = (int32_t)pool->nodes.size() - 1;
  return DQ_OK;
}

int32_t dq_pred_pool_size(const dq_pred_pool* pool) { return pool ? (int32_t)pool->nodes.size() : 0; }
const dq_pred_node* dq_pred_pool_nodes(const dq_pred_pool* pool) {
  return pool && !pool->nodes.empty() ? pool->nodes.data() : nullptr;
}
int32_t dq_pred_pool_num_patterns(const dq_pred_pool* pool) { return pool ? (int32_t)pool->patterns.size() : 0; }
const char* const* dq_pred_pool_patterns(const dq_pred_pool* pool) {
  return pool && !pool->pattern_ptrs.empty() ? pool->pattern_ptrs.data() : nullptr;
}
int32_t dq_pred_pool_num_exprs(const dq_pred_pool* pool) { return pool ? (int32_t)pool->exprs.size() : 0; }
const dq_expr_program* dq_pred_pool_expr(const dq_pred_pool* pool, int32_t index) {
  return pool && index >= 0 && (size_t)index < pool->exprs.size() ? &pool->exprs[(size_t)index]->prog : nullptr;
}
void dq_pred_pool_destroy(dq_pred_pool* pool) { delete pool; }

}  // extern "C"
