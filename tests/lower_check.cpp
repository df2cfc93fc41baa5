// lower_check.cpp -- the predicate lowering and the program builder (deequ_amd/csrc/dq_pred_lower.cpp) under host
// ASan + UBSan: a stand-alone program (its own main, the library's set_error restated here), built and run by
// tests/test_lower_host.py.  It compiles a fixed corpus of predicate texts (and hand-made IR nodes for what the SQL
// grammar cannot say) over a fixed schema, builds every case twice through PredBuilder -- in the order the planner
// asks for roots (a spec's `where` first, then its predicate or its synthetic NOT NULL root) and in the row
// program's (an output's predicate first, then its `where`) -- and prints a deterministic dump of each program.
// tests/lower_check_expected.txt is that dump as the code before the split (two assembly loops in dq_plan.cpp)
// produced it.  No device is touched.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../deequ_amd/csrc/dq_pred_compile.cpp"
#include "../deequ_amd/csrc/dq_regex.cpp"
#include "../deequ_amd/csrc/dq_pred_lower.cpp"

namespace dq {
static char g_msg[1024];
dq_status set_error(dq_status code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace dq
extern "C" const char* dq_last_error(void) { return dq::g_msg; }

using namespace dq;

// ---- corpus --------------------------------------------------------------------------------------------------------
struct Item {  // one analyzer / output: a predicate root (or the NOT NULL root of a column) and an optional `where`
  int32_t pred = -1, where = -1, notnull_col = -1;
};
struct Case {
  std::string name;
  std::vector<Item> items;
};

static const char* kNames[] = {"y", "h", "i", "b", "f", "a", "flag", "day", "t", "d18", "d38", "s", "ls", "dc", "b2", "a2"};
static const int32_t kTypes[] = {DQ_TYPE_I8, DQ_TYPE_I16, DQ_TYPE_I32, DQ_TYPE_I64, DQ_TYPE_F32, DQ_TYPE_F64,
                                 DQ_TYPE_BOOL, DQ_TYPE_DATE32, DQ_TYPE_TIMESTAMP, DQ_DECIMAL128(18, 2),
                                 DQ_DECIMAL128(38, 4), DQ_TYPE_UTF8, DQ_TYPE_LARGE_UTF8, DQ_TYPE_DICT_UTF8,
                                 DQ_TYPE_I64, DQ_TYPE_F64};
constexpr int kCols = 16;

static dq_pred_pool* g_pool = nullptr;
static std::vector<dq_pred_node> g_nodes;  // the pool's nodes, then the hand-made ones
static std::vector<std::string> g_patterns;
static std::vector<dq_column_desc> g_schema;
static std::vector<Case> g_cases;
static int g_fail = 0;

static int32_t sql(const std::string& text) {  // root of a text the SQL compiler must accept
  int32_t root = -1;
  if (dq_pred_pool_add(g_pool, text.c_str(), &root) != DQ_OK) {
    std::printf("FAILED: the SQL compiler refused `%s`: %s\n", text.c_str(), g_msg);
    ++g_fail;
  }
  return root;
}
static void one(const std::string& text) { g_cases.push_back({text, {Item{sql(text), -1, -1}}}); }
static void several(const std::string& name, const std::vector<std::string>& texts) {
  Case c{name, {}};
  for (const std::string& t : texts) c.items.push_back(Item{sql(t), -1, -1});
  g_cases.push_back(c);
}

static void sql_corpus() {
  const std::vector<std::string> ops = {"<", "<=", ">", ">=", "=", "!="};
  // column versus int, decimal and double literal
  for (const char* c : {"y", "h", "i", "b", "f", "a"})
    several(std::string(c) + " vs int / decimal / double",
            {std::string(c) + " > 3", std::string(c) + " <= 2.5", std::string(c) + " = 1e0"});
  for (const char* c : {"flag", "day", "t"})
    for (const char* l : {" > 3", " <= 2.5", " = 1e0"}) one(std::string(c) + l);
  several("flag vs boolean", {"flag = TRUE", "FALSE != flag", "flag", "NOT flag", "COALESCE(flag, TRUE) = TRUE"});
  one("flag = NULL");
  one("i = TRUE");
  one("i");
  // an integral column versus a decimal literal: the integer bounds of every operator, and the literal first
  {
    std::vector<std::string> t;
    for (const std::string& o : ops) t.push_back("i " + o + " 2.5");
    t.insert(t.end(), {"i = 2.0", "i != 2.00", "i >= -2.5", "b > -9223372036854775808", "-3 < a", "2.5 >= h"});
    several("integral vs decimal literal", t);
  }
  // decimal columns: the one-atom path (precision <= 18) and the high / low word path
  for (const char* c : {"d18", "d38"}) {
    std::vector<std::string> vi, vd, vw;
    for (const std::string& o : ops) {
      vi.push_back(std::string(c) + " " + o + " 3");
      vd.push_back(std::string(c) + " " + o + " -2.50505");  // more digits than the column's scale
      vw.push_back(std::string(c) + " " + o + " 2.5");
    }
    several(std::string(c) + " vs int", vi);
    several(std::string(c) + " vs decimal (finer)", vd);
    several(std::string(c) + " vs decimal (coarser)", vw);
  }
  several("decimal edges", {"d18 < 9223372036854775807", "d18 >= -9223372036854775808", "d18 = 9223372036854775807",
                            "d38 = NULL", "COALESCE(d18, 1.5) > 1", "COALESCE(d38, NULL) <= 7", "d38 != 12345678901234.5678"});
  one("d18 > 1e0");
  one("d38 = TRUE");
  one("COALESCE(d18, 1e0) > 1");
  // COALESCE, column versus column, IS [NOT] NULL
  several("COALESCE", {"COALESCE(b, 1.0) > 0", "COALESCE(f, 2.5) >= 1", "COALESCE(f, 2) > 16777217", "COALESCE(i, 1e0) < 3",
                       "COALESCE(a, NULL) > 1", "COALESCE(i, -3.00) < -3", "COALESCE(h, 7) = NULL", "COALESCE(f, 2) > 0.5"});
  several("column vs column", {"i = b", "y < a", "flag = flag", "f < h", "a2 >= f", "b != b2"});
  one("f < i");
  one("b > f");
  one("d18 < i");
  one("day < i");
  one("flag = i");
  several("IS NULL", {"t IS NOT NULL", "a IS NULL", "NULL IS NULL", "3 IS NOT NULL", "COALESCE(b, 3) IS NULL", "s IS NULL",
                      "COALESCE(b, 3) IS NOT NULL", "2.5 IS NULL"});
  one("COALESCE(b, NULL) IS NULL");
  // literal versus literal
  several("literal folding", {"1 < 2", "1.5 >= 1.50", "2 = 2e0", "NULL = 1", "1 != NULL", "TRUE", "NULL", "1 < 2.5", "3 > 2e0",
                              "1.10 = 1.1", "FALSE"});
  // strings
  several("strings", {"s = 'x'", "s != 'x'", "s IN ('a.b', 'c')", "ls = 'x'", "ls <> 'q'", "ls IN ('e', 'f')", "'x' = s",
                      "s NOT IN ('e')"});
  one("dc IS NULL");
  // nesting: a stack of exactly kPredStack, and one more
  {
    std::string deep = "i > " + std::to_string(kPredStack), over = "i > " + std::to_string(kPredStack + 1);
    for (int k = kPredStack - 1; k >= 1; --k)
      deep = "i > " + std::to_string(k) + (k % 2 ? " AND " : " OR ") + (k % 3 == 0 ? "NOT (" : "(") + deep + ")";
    for (int k = kPredStack; k >= 1; --k) over = "i > " + std::to_string(k) + (k % 2 ? " AND (" : " OR (") + over + ")";
    one(deep);
    one(over);
  }
  // kMaxRoots + 1 distinct roots; the same root under several spellings
  {
    std::vector<std::string> t;
    for (int k = 0; k <= kMaxRoots; ++k) t.push_back("b > " + std::to_string(k));
    several("one root too many", t);
    several("deduplicated roots", {"i > 1", "(i > 1)", "a < 2 AND i > 1", "`i` > 1", "i  >  1", "a < 2 AND (i > 1)", "i > 1.0"});
  }
  // kMaxInstr instructions, and one more (a NOT)
  {
    std::vector<std::string> full, over;
    for (int r = 0; r < kMaxInstr / 16; ++r) {
      std::string t;
      for (int j = 0; j < 8; ++j) t += (j ? " AND b > " : "b > ") + std::to_string(100 * r + j);
      full.push_back(t);
      over.push_back(r == 0 ? "NOT (" + t + ")" : t);
    }
    several("a full program", full);
    several("one instruction too many", over);
  }
  // patterns under and over the DFA budget (kMaxRegexWords): whole-value DFAs of ~300 states x 27 byte classes,
  // ~8.7 K words each
  {
    std::vector<std::string> t;
    for (int k = 0; k < 4; ++k) {
      std::string v;
      for (int j = 0; j < 300; ++j) v += (char)('a' + (j + k) % 26);
      t.push_back("s = '" + v + "'");
    }
    several("three long patterns", {t[0], t[1], t[2]});
    several("four long patterns", t);
  }
  // roots with `where`, and the planner's NOT NULL roots (Completeness with a `where`)
  {
    const int32_t w1 = sql("b > 0"), w2 = sql("i > 1 OR s = 'x'"), p1 = sql("a > 1"), p2 = sql("s IN ('x', 'y')");
    g_cases.push_back({"where and NOT NULL roots",
                       {Item{-1, w1, 5}, Item{p1, w1, -1}, Item{-1, w2, 5}, Item{p2, -1, -1}, Item{w1, w2, -1},
                        Item{-1, w1, 11}, Item{p1, p2, -1}}});
  }
}

static int32_t node(int32_t kind, int32_t a, int32_t b, int32_t cmp, int64_t i64, double f64) {
  g_nodes.push_back(dq_pred_node{kind, a, b, cmp, i64, f64});
  return (int32_t)g_nodes.size() - 1;
}
static void made(const std::string& name, int32_t root) { g_cases.push_back({name, {Item{root, -1, -1}}}); }

// what the SQL compiler does not emit: one case per refusal of the lowering it cannot reach
static void made_corpus() {
  const int32_t ci = node(DQ_PRED_COLUMN, 2, -1, 0, 0, 0.0), cs = node(DQ_PRED_COLUMN, 11, -1, 0, 0, 0.0);
  const int32_t l3 = node(DQ_PRED_LIT_INT, -1, -1, 0, 3, 0.0), lnull = node(DQ_PRED_LIT_NULL, -1, -1, 0, 0, 0.0);
  const int32_t isnull = node(DQ_PRED_IS_NULL, ci, -1, 0, 0, 0.0);
  made("decimal literal of scale 19", node(DQ_PRED_CMP, ci, node(DQ_PRED_LIT_DECIMAL, -1, -1, 19, 1, 0.0), DQ_CMP_LT, 0, 0.0));
  made("decimal literal of scale -1", node(DQ_PRED_CMP, node(DQ_PRED_LIT_DECIMAL, -1, -1, -1, 1, 0.0), l3, DQ_CMP_LT, 0, 0.0));
  made("child index out of range", node(DQ_PRED_NOT, 1 << 30, -1, 0, 0, 0.0));
  made("negative child index", node(DQ_PRED_AND, isnull, -2, 0, 0, 0.0));
  made("column out of range", node(DQ_PRED_IS_NULL, node(DQ_PRED_COLUMN, kCols, -1, 0, 0, 0.0), -1, 0, 0, 0.0));
  made("COALESCE of a non-column", node(DQ_PRED_CMP, node(DQ_PRED_COALESCE, l3, l3, 0, 0, 0.0), l3, DQ_CMP_GT, 0, 0.0));
  made("COALESCE with a column fallback", node(DQ_PRED_CMP, node(DQ_PRED_COALESCE, ci, ci, 0, 0, 0.0), l3, DQ_CMP_GT, 0, 0.0));
  made("COALESCE child out of range", node(DQ_PRED_CMP, node(DQ_PRED_COALESCE, ci, -1, 0, 0, 0.0), l3, DQ_CMP_GT, 0, 0.0));
  made("comparison operand that is a predicate", node(DQ_PRED_CMP, isnull, l3, DQ_CMP_EQ, 0, 0.0));
  made("comparison of two non-columns", node(DQ_PRED_CMP, isnull, isnull, DQ_CMP_EQ, 0, 0.0));
  made("comparison operator 0", node(DQ_PRED_CMP, ci, l3, 0, 0, 0.0));
  made("comparison operator 7", node(DQ_PRED_CMP, ci, l3, DQ_CMP_NE + 1, 0, 0.0));
  made("string column vs number", node(DQ_PRED_CMP, cs, l3, DQ_CMP_EQ, 0, 0.0));
  made("string columns compared", node(DQ_PRED_CMP, cs, cs, DQ_CMP_EQ, 0, 0.0));
  made("dictionary column vs number", node(DQ_PRED_CMP, node(DQ_PRED_COLUMN, 13, -1, 0, 0, 0.0), l3, DQ_CMP_EQ, 0, 0.0));
  made("IS NULL over a predicate", node(DQ_PRED_IS_NULL, isnull, -1, 0, 0, 0.0));
  made("IS NOT NULL over COALESCE(column, NULL)",
       node(DQ_PRED_IS_NOT_NULL, node(DQ_PRED_COALESCE, ci, lnull, 0, 0, 0.0), -1, 0, 0, 0.0));
  made("an arithmetic operand as a predicate", node(DQ_PRED_EXPR, 0, -1, DQ_TYPE_I32, 0, 0.0));
  made("a literal as a predicate", l3);
  made("node kind 99", node(99, 0, 0, 0, 0, 0.0));
  {
    int32_t n = isnull;
    for (int k = 0; k < 31; ++k) n = node(DQ_PRED_NOT, n, -1, 0, 0, 0.0);
    made("31 NOTs", n);
    made("32 NOTs", node(DQ_PRED_NOT, n, -1, 0, 0, 0.0));
  }
  g_patterns.push_back("[a-c]+x");
  const int64_t pat = (int64_t)g_patterns.size() - 1;
  g_patterns.push_back("(ab");
  g_cases.push_back({"regex modes", {Item{node(DQ_PRED_REGEX, cs, -1, DQ_REGEX_RLIKE, pat, 0.0), -1, -1},
                                     Item{node(DQ_PRED_REGEX, cs, -1, DQ_REGEX_EXTRACT_NONEMPTY, pat, 0.0), -1, -1},
                                     Item{node(DQ_PRED_REGEX, cs, -1, DQ_REGEX_FULL, pat, 0.0), -1, -1},
                                     Item{node(DQ_PRED_REGEX, node(DQ_PRED_COLUMN, 12, -1, 0, 0, 0.0), -1, DQ_REGEX_RLIKE, pat, 0.0), -1, -1}}});
  made("regex over a non-column", node(DQ_PRED_REGEX, l3, -1, DQ_REGEX_RLIKE, pat, 0.0));
  made("regex over an int column", node(DQ_PRED_REGEX, ci, -1, DQ_REGEX_RLIKE, pat, 0.0));
  made("regex over a dictionary column", node(DQ_PRED_REGEX, node(DQ_PRED_COLUMN, 13, -1, 0, 0, 0.0), -1, DQ_REGEX_RLIKE, pat, 0.0));
  made("regex mode 3", node(DQ_PRED_REGEX, cs, -1, 3, pat, 0.0));
  made("regex pattern out of range", node(DQ_PRED_REGEX, cs, -1, DQ_REGEX_RLIKE, 9999, 0.0));
  made("regex pattern -1", node(DQ_PRED_REGEX, cs, -1, DQ_REGEX_RLIKE, -1, 0.0));
  made("regex that does not compile", node(DQ_PRED_REGEX, cs, -1, DQ_REGEX_RLIKE, pat + 1, 0.0));
  made("regex child out of range", node(DQ_PRED_REGEX, -1, -1, DQ_REGEX_RLIKE, pat, 0.0));
}

// ---- the two ways through the builder ------------------------------------------------------------------------------
struct Built {
  dq_status status = DQ_OK;
  PredLimit limit = PL_NONE;
  PredProgram prog;
  std::vector<uint16_t> blob;
};

static void build(const Case& c, bool plan_style, Built& o) {
  std::memset(&o.prog, 0, sizeof o.prog);
  g_msg[0] = '\0';
  PredBuilder pb(g_nodes.data(), (int32_t)g_nodes.size(), &g_schema, &g_patterns, &o.blob);
  for (const Item& it : c.items) {
    int32_t slot = -1;
    if (plan_style) {  // build_plan: the spec's `where`, then its predicate / NOT NULL root
      if (it.where >= 0 && o.status == DQ_OK) o.status = pb.root(it.where, slot);
      if (o.status == DQ_OK) o.status = it.notnull_col >= 0 ? pb.notnull_root(it.notnull_col, slot) : pb.root(it.pred, slot);
    } else if (it.notnull_col < 0) {  // row_program_build: the output's predicate, then its `where`
      if (o.status == DQ_OK) o.status = pb.root(it.pred, slot);
      if (it.where >= 0 && o.status == DQ_OK) o.status = pb.root(it.where, slot);
    }
    if (o.status == DQ_OK && (plan_style || it.notnull_col < 0) && (slot < 0 || slot >= pb.n_roots())) {
      std::printf("FAILED: %s: slot %d of %d roots\n", c.name.c_str(), slot, pb.n_roots());
      ++g_fail;
    }
  }
  if (o.status == DQ_OK) o.status = pb.assemble(o.prog);
  o.limit = pb.limit;
  if ((o.limit != PL_NONE) != (o.status == DQ_E_UNSUPPORTED && g_msg[0] == '\0')) {
    std::printf("FAILED: %s: limit %d with status %d and message `%s`\n", c.name.c_str(), (int)o.limit, (int)o.status, g_msg);
    ++g_fail;
  }
}

// ---- dump ----------------------------------------------------------------------------------------------------------
static void dump(const char* style, const Built& o) {
  static const char* kLimit[] = {"none", "roots", "instructions", "stack", "regex"};
  std::printf("-- %s\n", style);
  if (o.status != DQ_OK) {
    std::printf("status=%d limit=%s%s%s\n", (int)o.status, kLimit[o.limit], o.limit == PL_NONE ? " error=" : "",
                o.limit == PL_NONE ? g_msg : "");
    return;
  }
  const PredProgram& p = o.prog;
  uint64_t h = 1469598103934665603ull;  // FNV-1a over the DFA words' bytes (little-endian)
  for (uint16_t w : o.blob)
    for (int k = 0; k < 2; ++k) h = (h ^ ((w >> (8 * k)) & 0xFF)) * 1099511628211ull;
  std::printf("status=0 n_instr=%d n_roots=%d stack_depth=%d n_loads=%d regex_words=%d regex_fnv=%016llx\n", p.n_instr,
              p.n_roots, p.stack_depth, p.n_loads, p.regex_words, (unsigned long long)h);
  std::printf("load_instr:");
  for (int i = 0; i < p.n_loads; ++i) std::printf(" %d", (int)p.load_instr[i]);
  std::printf("\n");
  for (int i = 0; i < p.n_instr; ++i) {
    const PredInstr& x = p.instr[i];
    std::printf("%3d: op=%d cmp=%d ctype=%d null_res=%d col_a=%d col_b=%d kind_a=%d kind_b=%d lit_i=%lld lit_d=%a slot=%d pad=%d\n",
                i, x.op, x.cmp, x.ctype, x.null_res, x.col_a, x.col_b, x.kind_a, x.kind_b, (long long)x.lit_i, x.lit_d,
                x.slot, x.pad);
  }
}

int main() {
  if (dq_pred_pool_create(kNames, kTypes, kCols, &g_pool) != DQ_OK) return 2;
  for (int c = 0; c < kCols; ++c) g_schema.push_back(dq_column_desc{kTypes[c], c == kCols - 1 ? 0 : 1});
  sql_corpus();
  const int32_t n_sql = dq_pred_pool_size(g_pool);
  g_nodes.assign(dq_pred_pool_nodes(g_pool), dq_pred_pool_nodes(g_pool) + n_sql);
  for (int32_t k = 0; k < dq_pred_pool_num_patterns(g_pool); ++k) g_patterns.emplace_back(dq_pred_pool_patterns(g_pool)[k]);
  made_corpus();
  for (size_t k = 0; k < g_cases.size(); ++k) {
    const Case& c = g_cases[k];
    bool same_order = true;  // the planner and the row program meet this case's roots in the same order
    for (const Item& it : c.items) same_order = same_order && it.where < 0 && it.notnull_col < 0;
    std::printf("== case %zu (%zu roots asked, %s order): %s\n", k, c.items.size(), same_order ? "same" : "own",
                c.name.size() > 100 ? (c.name.substr(0, 100) + "...").c_str() : c.name.c_str());
    Built plan, row;
    build(c, true, plan);
    dump("plan", plan);
    build(c, false, row);
    dump("row", row);
    if (same_order && (plan.status != row.status || std::memcmp(&plan.prog, &row.prog, sizeof(PredProgram)) != 0 ||
                       plan.blob != row.blob)) {
      std::printf("FAILED: %s: the two orders built different programs\n", c.name.c_str());
      ++g_fail;
    }
  }
  dq_pred_pool_destroy(g_pool);
  if (g_fail) return 1;
  std::printf("ok %zu cases\n", g_cases.size());
  return 0;
}
