// expr_check.cpp -- the predicate compiler's arithmetic operands (deequ_amd/csrc/dq_pred_compile.cpp) under host
// ASan + UBSan: a stand-alone program (its own main, the library's set_error / dq_last_error restated here), built
// by tests/test_expr_host.py.  It drives dq_pred_pool_add over a fixed list of accepted and malformed texts and
// checks what the header promises: a refusal leaves the pool unchanged, an accepted text leaves children that point
// at earlier nodes, and every program obeys the stack discipline and the limits.  No device is touched.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../deequ_amd/csrc/dq_pred_compile.cpp"
#include "../deequ_amd/csrc/dq_regex.cpp"

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

static int g_fail = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, dq::g_msg); \
      ++g_fail;                                                                   \
    }                                                                             \
  } while (0)

static void check_program(const dq_expr_program* p) {
  CHECK(p && p->n_instrs >= 1 && p->n_instrs <= DQ_EXPR_MAX_INSTRS);
  CHECK(p->n_columns >= 1 && p->n_columns <= DQ_EXPR_MAX_COLUMNS);
  CHECK(p->n_literals >= 0 && p->n_literals <= DQ_EXPR_MAX_LITERALS);
  CHECK(p->text && std::strlen(p->text) > 0);
  int depth = 0, deepest = 0;
  for (int i = 0; i < p->n_instrs; ++i) {
    const dq_expr_instr& x = p->instrs[i];
    if (x.op == DQ_EXPR_COL) CHECK(x.arg >= 0 && x.arg < p->n_columns && x.type == p->column_types[x.arg]);
    if (x.op == DQ_EXPR_LIT) CHECK(x.arg >= 0 && x.arg < p->n_literals && x.type == p->literals[x.arg].type);
    if (x.op == DQ_EXPR_COL || x.op == DQ_EXPR_LIT) {
      ++depth;
    } else if (x.op >= DQ_EXPR_ADD && x.op <= DQ_EXPR_MOD) {
      CHECK(depth >= 2);
      --depth;
    } else {
      CHECK((x.op == DQ_EXPR_CAST || x.op == DQ_EXPR_NEG) && depth >= 1);
    }
    if (depth > deepest) deepest = depth;
  }
  CHECK(depth == 1 && deepest == p->stack_depth && deepest <= DQ_EXPR_MAX_STACK);
  CHECK(p->instrs[p->n_instrs - 1].type == p->result_type);
}

int main() {
  const char* names[] = {"a", "b", "i", "h", "y", "f", "s", "t", "d", "flag"};
  const int32_t types[] = {DQ_TYPE_F64, DQ_TYPE_I64, DQ_TYPE_I32, DQ_TYPE_I16, DQ_TYPE_I8, DQ_TYPE_F32, DQ_TYPE_UTF8,
                           DQ_TYPE_TIMESTAMP, DQ_DECIMAL128(10, 2), DQ_TYPE_BOOL};
  dq_pred_pool* pool = nullptr;
  CHECK(dq_pred_pool_create(names, types, 10, &pool) == DQ_OK);

  std::string deep = "i", wide = "i", many = "i";
  for (int k = 0; k < 12; ++k) deep = "(i + " + deep + ")";
  for (int k = 0; k < 40; ++k) wide += " + i";
  for (int k = 0; k < 20; ++k) many += " + " + std::to_string(k);
  std::string minus(200, '-');
  const std::vector<std::string> texts = {
      // accepted
      "a + b > 3", "a+b>3", "i % 2 = 0", "b * i <= a", "a / b IS NULL", "a / b IS NOT NULL", "-i - -3 > f * 2.5",
      "(a + b) * (i - h) / y % 7 >= -(f)", "a + b > 4 AND NOT (a + b < 9 OR `i` * 2 = h)", "a * b + i <= a - 1e3",
      "y + 1 = 128", "b + 9223372036854775807 > 0", "i - -2147483648 < 0", "f % 2.5 > 0.5", "- - i > 0", "a > -3",
      "COALESCE(b, -3) > i + 1", "s = 'x' AND i + 1 > 2", "1 < 2",
      // refused
      "i + 2.5 > 1", "2.5 * 3.5 > a", "1 + 2 > a", "s + 1 > 2", "t - 1 > 0", "d * 2 > 1", "flag + 1 > 0", "abs(a) > 1",
      "a BETWEEN 1 AND 2", "a + 1 BETWEEN 1 AND 2", "a IN (1, 2)", "a - 1 IN (1, 2)", "COALESCE(a, 0) + 1 > 2",
      "NULL + 1 > a", "a + NULL > 1", "a + b", "NOT a + b", "a + > 1", "a + b >", "(a + b > 1", "a + 'x' > 1",
      "a + b = 'x'", "a * * b > 1", "a % > 1", "/ a > 1", "a + (b > 1) > 2", "COALESCE(a + 1, 0) > 2", "a + TRUE > 1",
      "length(s) + 1 > 3", "a + zz > 1", "-(2.5) + a > 1", deep + " > 0", wide + " > 0", many + " > 0",
      minus + "i > 0", "a +", "+", "a % b %", "((((a", "a + 1e > 2", "a + 1.2.3 > 2", "a + 10L > 2"};
  int accepted = 0, refused = 0;
  for (const std::string& text : texts) {
    const int32_t n0 = dq_pred_pool_size(pool), e0 = dq_pred_pool_num_exprs(pool), p0 = dq_pred_pool_num_patterns(pool);
    int32_t root = -7;
    const dq_status s = dq_pred_pool_add(pool, text.c_str(), &root);
    CHECK(s == DQ_OK || s == DQ_E_UNSUPPORTED || s == DQ_E_INVALID);
    if (s != DQ_OK) {
      ++refused;
      CHECK(dq_pred_pool_size(pool) == n0 && dq_pred_pool_num_exprs(pool) == e0 && dq_pred_pool_num_patterns(pool) == p0);
      CHECK(std::strlen(dq_last_error()) > 0);
      continue;
    }
    ++accepted;
    const int32_t n = dq_pred_pool_size(pool);
    const dq_pred_node* nodes = dq_pred_pool_nodes(pool);
    CHECK(root >= 0 && root < n);
    for (int32_t i = n0; i < n; ++i) {
      const int32_t k = nodes[i].kind;
      if (k == DQ_PRED_CMP || k == DQ_PRED_AND || k == DQ_PRED_OR || k == DQ_PRED_COALESCE)
        CHECK(nodes[i].a >= 0 && nodes[i].a < i && nodes[i].b >= 0 && nodes[i].b < i);
      if (k == DQ_PRED_NOT || k == DQ_PRED_IS_NULL || k == DQ_PRED_IS_NOT_NULL) CHECK(nodes[i].a >= 0 && nodes[i].a < i);
      if (k == DQ_PRED_EXPR) {
        CHECK(nodes[i].a >= 0 && nodes[i].a < dq_pred_pool_num_exprs(pool));
        CHECK(nodes[i].cmp == dq_pred_pool_expr(pool, nodes[i].a)->result_type);
      }
    }
  }
  for (int32_t k = 0; k < dq_pred_pool_num_exprs(pool); ++k) check_program(dq_pred_pool_expr(pool, k));
  CHECK(dq_pred_pool_expr(pool, -1) == nullptr && dq_pred_pool_expr(pool, dq_pred_pool_num_exprs(pool)) == nullptr);
  CHECK(accepted == 19 && refused == (int)texts.size() - 19);
  dq_pred_pool_destroy(pool);
  if (g_fail) return 1;
  std::printf("ok %d accepted, %d refused\n", accepted, refused);
  return 0;
}
