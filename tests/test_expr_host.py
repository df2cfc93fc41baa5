"""Arithmetic operands of predicates without a GPU: the grammar and the postfix programs dq_pred_pool_add returns
(evaluated with tests/expr_ref.py, the independent restatement of the rules), the result-type table, the refusals, the
unchanged lowering of every text accepted before, the reference itself against hand-written Java values, the host-only
plan lowering, dq_expr_eval_host (the kernel's row function on the CPU) against the reference, and the compiler under
host ASan + UBSan as a stand-alone program (tests/expr_check.cpp).  tests/test_expr_gpu.py runs the same cases on the
device.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import expr_ref as R
from tests.conftest import ROOT

KINDS = ["i8", "i16", "i32", "i64", "f32", "f64"]
# two columns of every kind, and operands arithmetic refuses
SCHEMA = [(f"{k}_{j}", k, True) for k in KINDS for j in "ab"] + [
    ("s", "utf8", True), ("t", "timestamp", True), ("day", "date32", True), ("flag", "bool", True),
    ("dec", "decimal(10,2)", True)]
OPS = ["+", "-", "*", "/", "%"]


@pytest.fixture(scope="module")
def dq():
    import deequ_amd

    return deequ_amd


def compile_expr(text, schema=SCHEMA):
    """The one expression of predicate `text` (expressions.Expression), compiled on the host."""
    from deequ_amd.analyzers import PlanBuilder

    b = PlanBuilder(schema, collect_exprs=True)
    b.pool.add(text)
    assert len(b.exprs) == 1, (text, list(b.exprs))
    return next(iter(b.exprs.values()))


def edge_values(kind):
    """MIN / MAX and small values of both signs; for the floating kinds also +-0.0, NaN, +-inf and subnormals."""
    if kind in R.BITS:
        lo, hi = -(1 << (R.BITS[kind] - 1)), (1 << (R.BITS[kind] - 1)) - 1
        return np.array([lo, hi, lo + 1, hi - 1, -1, 0, 1, 2, -2, 3, 7, -7, 100, -100], dtype=R.NP[kind])
    f = np.finfo(R.NP[kind])
    return np.array([0.0, -0.0, np.nan, np.inf, -np.inf, f.smallest_subnormal, -f.smallest_subnormal, f.tiny / 2,
                     f.max, -f.max, 1.5, -2.5, 7.0, 3.0, 1.0 + f.eps], dtype=R.NP[kind])


def pair_columns(ka, kb, n, bitmaps):
    """Two columns of n rows in which every pair of edge values meets (the first len(a) * len(b) rows, then again);
    with bitmaps, NULLs with periods 11 and 13."""
    va, vb = edge_values(ka), edge_values(kb)
    r = np.arange(n)
    a, b = va[r % len(va)], vb[(r // len(va)) % len(vb)]
    return (ka, a, (r % 11 != 3) if bitmaps else None), (kb, b, (r % 13 != 5) if bitmaps else None)


def reference(expr, cols):
    """expr_ref over the rows: (dtype, values, valid, NULL count) of a compiled expression."""
    instrs, lits = expr.instructions(), expr.literals()
    t, vals, ok = R.rows(lambda *row: R.eval_postfix(instrs, lits, row), *cols)
    return t, vals, ok, int((~ok).sum())


def host_eval(expr, cols):
    """dq_expr_eval_host over numpy columns: (values, valid, NULL count)."""
    from deequ_amd import _lib as L
    from deequ_amd.table import pack_validity

    n = len(cols[0][1])
    keep, views = [], (L.ColumnView * len(cols))()
    for k, (t, a, valid) in enumerate(cols):
        a = np.ascontiguousarray(a, dtype=R.NP[t])
        bits = None if valid is None else pack_validity(valid)
        keep += [a, bits]
        views[k].values = a.ctypes.data
        views[k].validity = None if bits is None else bits.ctypes.data
    out = np.full(n + 1, 0x55, dtype=R.NP[expr.dtype])
    words = np.zeros((n + 63) // 64 + 1, dtype=np.uint64)
    nulls = ctypes.c_int64(-1)
    L.check(L.lib.dq_expr_eval_host(ctypes.byref(expr.program), views, n, out.ctypes.data, words.ctypes.data,
                                    ctypes.byref(nulls)))
    valid = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
    return out[:n], valid, nulls.value


def assert_matches(expr, cols, got_vals, got_valid, got_nulls, what=""):
    t, vals, ok, nulls = reference(expr, cols)
    assert expr.dtype == t, (what, expr.text, expr.dtype, t)
    assert np.array_equal(got_valid, ok), (what, expr.text, np.flatnonzero(got_valid != ok)[:5])
    bad = np.flatnonzero(ok & ~R.same(t, got_vals, vals))
    assert bad.size == 0, (what, expr.text, bad[:5], got_vals[bad[:5]], vals[bad[:5]])
    assert got_nulls == nulls, (what, expr.text)


def v(t, x):
    return (t, x if t in R.BITS or x is None else R.NP[t](x))


# ---- the reference against hand-written Java values ----------------------------------------------------------------
def test_reference_against_java_values():
    assert R.binary("+", v("i8", 127), v("i8", 1)) == ("i8", -128)  # (byte) (127 + 1)
    assert R.binary("%", v("i32", -2147483648), v("i32", -1)) == ("i32", 0)
    assert R.binary("%", v("i32", -7), v("i32", 3)) == ("i32", -1)
    assert R.binary("%", v("i32", 7), v("i32", -3)) == ("i32", 1)
    assert R.binary("/", v("i32", 7), v("i32", 2)) == ("f64", 3.5)
    assert R.binary("/", v("i32", 7), v("i32", 0)) == ("f64", None)
    assert R.binary("%", v("i64", 7), v("i8", 0)) == ("i64", None)
    assert R.binary("/", v("f64", 1.0), v("f64", -0.0)) == ("f64", None)
    assert R.binary("%", v("f32", 1.0), v("f32", 0.0)) == ("f32", None)
    assert R.binary("*", v("i32", 65536), v("i32", 65536)) == ("i32", 0)
    assert R.binary("-", v("i64", -(1 << 63)), v("i32", 1)) == ("i64", (1 << 63) - 1)
    assert R.neg(v("i16", -32768)) == ("i16", -32768)
    assert R.binary("+", v("i64", 1), v("f32", 0.5)) == ("f32", np.float32(1.5))
    assert R.binary("+", v("i32", 1), v("i32", None)) == ("i32", None)
    assert R.binary("%", v("f64", -7.5), v("f64", 2.0)) == ("f64", -1.5)  # Java: -7.5 % 2.0
    assert R.binary("*", R.literal("2.5"), v("f32", 2.0)) == ("f64", 5.0)
    assert R.literal("3") == ("i32", 3) and R.literal("2147483648") == ("i64", 2147483648)
    assert R.literal("3e0") == ("f64", 3.0)
    with pytest.raises(R.Unsupported):
        R.binary("+", R.literal("2.5"), v("i32", 1))
    # no contraction: a * b + c with a = b = 1 + 2^-27, c = -(1 + 2^-26) is 0; one rounding (an FMA) gives 2^-54
    a, c = 1.0 + 2.0 ** -27, -(1.0 + 2.0 ** -26)
    assert R.binary("+", R.binary("*", v("f64", a), v("f64", a)), v("f64", c)) == ("f64", 0.0)
    a, c = np.float32(1.0 + 2.0 ** -12), np.float32(-(1.0 + 2.0 ** -11))
    assert R.binary("+", R.binary("*", v("f32", a), v("f32", a)), v("f32", c)) == ("f32", np.float32(0.0))
    assert float(a) * float(a) + float(c) == 2.0 ** -24  # (what a single rounding would keep)


# ---- grammar ------------------------------------------------------------------------------------------------------
def _row(expr, values):
    """The program on one row given {column: (type, value)}."""
    return R.eval_postfix(expr.instructions(), expr.literals(), [values[c] for c in expr.columns])


def test_precedence_associativity_unary_and_parentheses(dq):
    x = {"i32_a": v("i32", 17), "i32_b": v("i32", 5), "i64_a": v("i64", 3), "f64_a": v("f64", 0.25)}
    a, b, c, d = x["i32_a"], x["i32_b"], x["i64_a"], x["f64_a"]
    B, N = R.binary, R.neg
    lit = R.literal
    cases = {
        "i32_a + i32_b * i64_a > 0": B("+", a, B("*", b, c)),
        "i32_a * i32_b + i64_a > 0": B("+", B("*", a, b), c),
        "(i32_a + i32_b) * i64_a > 0": B("*", B("+", a, b), c),
        "i32_a - i32_b - i64_a > 0": B("-", B("-", a, b), c),
        "i32_a - (i32_b - i64_a) > 0": B("-", a, B("-", b, c)),
        "i32_a / i32_b / i64_a > 0": B("/", B("/", a, b), c),
        "i32_a % i32_b % i64_a = 0": B("%", B("%", a, b), c),
        "i32_a / i32_b * i64_a > 0": B("*", B("/", a, b), c),
        "i32_a - i32_b % i64_a > 0": B("-", a, B("%", b, c)),
        "-i32_a + i32_b > 0": B("+", N(a), b),
        "- - i32_a > 0": N(N(a)),
        "-(i32_a + i32_b) * i64_a > 0": B("*", N(B("+", a, b)), c),
        "i32_a - -3 > 0": B("-", a, lit("-3")),
        "i32_a -3 > 0": B("-", a, lit("3")),
        "i32_a * -i32_b > 0": B("*", a, N(b)),
        "((i32_a)) + (((i32_b) * 2)) > 0": B("+", a, B("*", b, lit("2"))),
        "f64_a * 2.5 + i32_a > 0": B("+", B("*", d, lit("2.5")), a),
        "`i32_a`+`i32_b`*3e0 > 0": B("+", a, B("*", b, lit("3e0"))),
        "1 < i32_a % 4": B("%", a, lit("4")),
        "i32_a + 3000000000 IS NOT NULL": B("+", a, lit("3000000000")),
    }
    for text, want in cases.items():
        e = compile_expr(text)
        got = _row(e, x)
        assert got[0] == want[0] == e.dtype and got[1] == want[1], (text, e.text, got, want)
        assert e.program.stack_depth <= 8 and e.program.n_instrs <= 32


def test_result_type_table(dq):
    from deequ_amd import _lib as L

    for ka, kb, op in itertools.product(KINDS, KINDS, OPS):
        e = compile_expr(f"{ka}_a {op} {kb}_b > 0")
        want = "f64" if op == "/" else KINDS[max(KINDS.index(ka), KINDS.index(kb))]
        assert e.dtype == want and e.divides == (op in "/%"), (ka, kb, op, e.dtype)
        assert e.columns == (f"{ka}_a", f"{kb}_b")
    for k in KINDS:
        wide = lambda t: KINDS[max(KINDS.index(k), KINDS.index(t))]  # noqa: E731
        assert compile_expr(f"{k}_a + 1 > 0").dtype == wide("i32")  # an integer literal that fits: IntegerType
        assert compile_expr(f"{k}_a + 2147483648 > 0").dtype == wide("i64")
        assert compile_expr(f"{k}_a + -2147483648 > 0").dtype == wide("i32")
        assert compile_expr(f"{k}_a * 3e0 > 0").dtype == "f64"
        assert compile_expr(f"-{k}_a > 0").dtype == k
        assert compile_expr(f"{k}_a / 2 > 0").dtype == "f64"
        if k in ("f32", "f64"):  # a decimal literal next to Float / Double: cast to Double
            e = compile_expr(f"{k}_a - 2.5 > 0")
            assert e.dtype == "f64" and e.literals() == [(L.TYPE_F64, 2.5)]
    e = compile_expr("i8_a + 1 > 0")  # nullable: an input is, or the program divides
    assert e.nullable([("i8_a", "i8", False)]) is False and e.nullable([("i8_a", "i8", True)]) is True
    assert compile_expr("i8_a % 2 = 0").nullable([("i8_a", "i8", False)]) is True


def test_canonical_text_dedup(dq):
    from deequ_amd import _lib as L
    from deequ_amd.analyzers import PlanBuilder

    b = PlanBuilder(SCHEMA, collect_exprs=True)
    for text in ("i32_a+i32_b > 1", "(`i32_a`) + ((i32_b)) < 9 AND i32_a  +  i32_b <> 4", "i32_b + i32_a > 1",
                 "i32_a + i32_b + 1 > 1", "i32_a + (i32_b + 1) > 1", "i32_a + 1e0 > 0", "i32_a + 1 > 0"):
        b.pool.add(text)
    assert list(b.exprs) == ["(`i32_a` + `i32_b`)", "(`i32_b` + `i32_a`)", "((`i32_a` + `i32_b`) + 1)",
                             "(`i32_a` + (`i32_b` + 1))", "(`i32_a` + 1e0)", "(`i32_a` + 1)"]
    assert L.lib.dq_pred_pool_num_exprs(b.pool._h) == 6
    kinds = [n[0] for n in b.pool.nodes]
    assert kinds.count(L.PRED_EXPR) == 8 and [n[1] for n in b.pool.nodes if n[0] == L.PRED_EXPR][:3] == [0, 0, 0]


REFUSED = {
    "flag + 1 > 0": "non-numeric", "day - 1 > 0": "non-numeric", "t % 2 = 0": "non-numeric", "s + 1 > 2": "non-numeric",
    "i32_a + 'x' > 1": "string", "dec * 2 > 1": "decimal column", "i32_a + 2.5 > 1": "decimal literal",
    "2.5 * 3.5 + f64_a > 1": "decimal", "-(2.5) + f64_a > 1": "decimal", "2.5 * 3.5 > f64_a": "no column", "COALESCE(i32_a, 0) + 1 > 2": "COALESCE",
    "i32_a + NULL > 1": "NULL", "NULL * i32_a > 1": "NULL", "1 + 2 > i32_a": "no column", "-(3) < i32_a": "no column",
    "i32_a + TRUE > 0": "boolean", "i32_a + (i32_b > 1) > 0": "boolean", "abs(i32_a) + 1 > 1": "function call",
    "length(s) > 3": "function call", "i32_a + 1 BETWEEN 1 AND 2": "BETWEEN", "i32_a BETWEEN 1 AND 2": "BETWEEN",
    "i32_a IN (1, 2)": "IN list", "i32_a + 1 IN (1, 2)": "IN over", "i32_a + i32_b": "boolean", "NOT i32_a + 1": "boolean",
    "i32_a + i32_b = 'x'": "string", "COALESCE(i32_a + 1, 0) > 2": None, "COALESCE((i32_a + 1), 0) > 2": "argument", "i32_a LIKE 'x%'": "LIKE",
    " > 0".join(["(i32_a + " * 9 + "i32_b" + ")" * 9, ""]): "value stack",
    " + ".join(["i32_a"] * 20) + " > 0": "instructions",
    " + ".join(f"{k}_{j}" for k in KINDS for j in "ab")[:-8] + " > 0": "columns",
    "i32_a + " + " + ".join(str(k) for k in range(16)) + " > 0": "instructions",
    "i32_a * * 2 > 0": None, "i32_a + > 0": None, "i32_a % > 1": None, "(i32_a + 1 > 0": None, "i32_a + 10L > 1": None,
}


def test_refusals_leave_the_pool_unchanged(dq):
    from deequ_amd import _lib as L
    from deequ_amd.analyzers import PlanBuilder
    from deequ_amd.predicates import UnsupportedPredicate

    b = PlanBuilder(SCHEMA, collect_exprs=True)
    b.pool.add("i32_a + 1 > 0 AND s = 'x'")
    size = (L.lib.dq_pred_pool_size(b.pool._h), L.lib.dq_pred_pool_num_exprs(b.pool._h),
            L.lib.dq_pred_pool_num_patterns(b.pool._h))
    for text, reason in REFUSED.items():
        with pytest.raises(UnsupportedPredicate) as ei:
            b.pool.add(text)
        if reason:
            assert reason in str(ei.value), (text, str(ei.value))
        assert (L.lib.dq_pred_pool_size(b.pool._h), L.lib.dq_pred_pool_num_exprs(b.pool._h),
                L.lib.dq_pred_pool_num_patterns(b.pool._h)) == size, text
    with pytest.raises(KeyError):
        b.pool.add("i32_a + zz > 1")
    assert L.lib.dq_pred_pool_size(b.pool._h) == size[0]


ACCEPTED_BEFORE = [
    "`f64_a` IS NULL OR (`f64_a` >= 0.0 AND `f64_a` <= 7.5)", "COALESCE(i64_a, 1.0) > 0 AND f64_a > -1.5e2 AND NOT i64_a <> 3",
    "i64_a > -9223372036854775808", "s IN ('a.b', 'c') OR s = 'd' OR s NOT IN ('e')", "f64_a > - 3", "-3 < f64_a",
    "COALESCE(i64_a, -3.00) < -3", "1 < 2", "TRUE", "flag = TRUE", "(i32_a > 1) AND ((i32_b) <= (2))", "t IS NOT NULL",
    "i32_a = i32_b", "NOT (i8_a != 3 OR i16_a == 4)", "'x' = s", "f32_a >= .5", "i32_a", "NULL",
]


def test_texts_accepted_before_lower_as_before(dq):
    """The node arrays of texts without arithmetic, pinned as the parent commit produced them for a sample, and for
    all of them equal whether or not the pool has seen expressions in between."""
    from deequ_amd import _lib as L
    from deequ_amd.analyzers import PlanBuilder

    plain = PlanBuilder(SCHEMA, collect_exprs=True)
    mixed = PlanBuilder(SCHEMA, collect_exprs=True)
    for i, text in enumerate(ACCEPTED_BEFORE):
        n0, m0 = len(plain.pool.nodes), len(mixed.pool.nodes)
        plain.pool.add(text)
        mixed.pool.add(text)
        rel = lambda nodes, base: [(k, a - base if k >= L.PRED_CMP else a, b - base if b >= 0 else b, c, i64, f)  # noqa: E731
                                   for k, a, b, c, i64, f in nodes[base:]]
        assert rel(plain.pool.nodes, n0) == rel(mixed.pool.nodes, m0), text
        mixed.pool.add(f"i32_a * {i + 2} + i64_a % 3 > f64_a / 2")
    assert plain.pool.patterns == mixed.pool.patterns and not plain.exprs
    assert all(n[0] != L.PRED_EXPR for n in plain.pool.nodes)
    b = PlanBuilder(SCHEMA)
    r = b.pool.add("COALESCE(i64_a, -3.00) < -3 AND f64_a > - 3")
    C = L
    assert b.pool.nodes == [(C.PRED_COLUMN, 0, -1, 0, 0, 0.0), (C.PRED_LIT_DECIMAL, -1, -1, 2, -300, 0.0),
                            (C.PRED_COALESCE, 0, 1, 0, 0, 0.0), (C.PRED_LIT_INT, -1, -1, 0, -3, 0.0),
                            (C.PRED_CMP, 2, 3, C.CMP_LT, 0, 0.0), (C.PRED_COLUMN, 1, -1, 0, 0, 0.0),
                            (C.PRED_LIT_INT, -1, -1, 0, -3, 0.0), (C.PRED_CMP, 5, 6, C.CMP_GT, 0, 0.0),
                            (C.PRED_AND, 4, 7, 0, 0, 0.0)] and r == 8


# ---- plan lowering on the host -------------------------------------------------------------------------------------
def test_host_only_plan_lowering(dq):
    from deequ_amd import _lib as L
    from deequ_amd import expressions as X
    from deequ_amd.analyzers import PlanBuilder
    from deequ_amd.metrics import UnsupportedOnGpuPathException
    from deequ_amd.runner import explain, gpu_eligible

    schema = [("a", "i32", False), ("b", "i64", True), ("x", "f64", True)]
    an = [dq.Compliance("sum", "a + b > 3"), dq.Compliance("div", "a / b IS NULL")]
    with_cols, names = X.lowering_schema(an, schema)
    assert names == {"(`a` + `b`)": "expr(`a` + `b`)", "(`a` / `b`)": "expr(`a` / `b`)"}
    assert with_cols[3:] == [("expr(`a` + `b`)", "i64", True), ("expr(`a` / `b`)", "f64", True)]
    b = PlanBuilder(with_cols, expr_columns=names)
    for a in an:
        a._lower(b)
    assert b.columns == ["expr(`a` + `b`)", "expr(`a` / `b`)"]  # nothing else reads a or b
    assert [n[0] for n in b.pool.nodes] == [L.PRED_LIT_INT, L.PRED_COLUMN, L.PRED_CMP, L.PRED_COLUMN, L.PRED_IS_NULL]
    text = explain(an + [dq.Mean("x", where="a % 2 = 0")], schema)
    assert text.startswith("plan: ")
    # a name a data column carries is avoided; a non-nullable input without / or % gives a non-nullable column
    taken, names = X.derived_schema({e.text: e for e in [compile_expr("a + 1 > 0", schema)]},
                                    schema + [("expr(`a` + 1)", "i32", True)])
    assert names == {"(`a` + 1)": "_expr(`a` + 1)"} and taken[-1] == ("_expr(`a` + 1)", "i32", False)
    # routing: arithmetic is eligible, with or without attached columns; what the grammar refuses is not
    assert gpu_eligible(an[0], schema) is None and gpu_eligible(an[1], with_cols, None, names) is None
    assert gpu_eligible(dq.Compliance("p", "abs(a) + 1 > 2"), schema) is not None
    assert gpu_eligible(dq.Compliance("p", "a + 2.5 > 2"), schema) is not None
    # the plan's comparison rules apply to the derived column's type: Float against an integer is refused as before
    f = [("f", "f32", True), ("i", "i32", True)]
    assert (gpu_eligible(dq.Compliance("p", "f * 2 > 16777217"), f) is None) == \
        (gpu_eligible(dq.Compliance("p", "f > 16777217"), f) is None)
    # a plan over data that carries no derived column is refused, not run without the expression
    with pytest.raises(UnsupportedOnGpuPathException):
        an[0]._lower(PlanBuilder(schema))
    # row-level planning on the host: nothing is skipped
    check = dq.Check(dq.CheckLevel.Error, "c").satisfies("a + b > 3", "sum").satisfies("a / b > 0.5", "div")
    plan = dq.plan_row_level([check], schema)
    assert plan.skipped == [] and sorted(plan.expr_columns) == ["(`a` + `b`)", "(`a` / `b`)"]
    assert sorted(plan.columns()) == sorted(plan.expr_columns.values())
    for p in plan.programs:
        p.close()


def test_program_checks_of_the_evaluator(dq):
    from deequ_amd import _lib as L

    e = compile_expr("i32_a + i64_a * 2 > 0")
    cols = [("i32", np.array([1, 2, 3], np.int32), None), ("i64", np.array([5, 6, 7], np.int64), None)]
    vals, valid, nulls = host_eval(e, cols)
    assert vals.tolist() == [11, 14, 17] and valid.all() and nulls == 0
    views = (L.ColumnView * 2)()
    out, words = np.zeros(4, np.int64), np.zeros(2, np.uint64)

    def run(p):
        return L.lib.dq_expr_eval_host(ctypes.byref(p), views, 0, out.ctypes.data, words.ctypes.data, None)

    def broken(change):
        p = L.ExprProgram.from_buffer_copy(e.program)
        change(p)
        return run(p)

    assert run(e.program) == L.DQ_OK  # n = 0 is valid
    assert broken(lambda p: setattr(p, "n_instrs", 33)) == L.DQ_E_INVALID
    assert broken(lambda p: setattr(p, "n_instrs", p.n_instrs - 1)) == L.DQ_E_INVALID  # two values left
    assert broken(lambda p: setattr(p, "n_columns", 9)) == L.DQ_E_INVALID
    assert broken(lambda p: setattr(p.instrs[0], "arg", 5)) == L.DQ_E_INVALID
    assert broken(lambda p: setattr(p.instrs[0], "type", L.TYPE_I64)) == L.DQ_E_INVALID
    assert broken(lambda p: setattr(p.instrs[p.n_instrs - 1], "op", 77)) == L.DQ_E_INVALID
    assert broken(lambda p: setattr(p, "result_type", L.TYPE_I32)) == L.DQ_E_INVALID
    assert broken(lambda p: p.column_types.__setitem__(0, L.TYPE_UTF8)) == L.DQ_E_UNSUPPORTED
    assert broken(lambda p: setattr(p, "result_type", L.TYPE_BOOL)) == L.DQ_E_UNSUPPORTED
    assert b"dq_expr_eval_host" in L.lib.dq_last_error()
    assert L.lib.dq_expr_eval_host(None, views, 0, None, None, None) == L.DQ_E_INVALID
    deep = L.ExprProgram.from_buffer_copy(e.program)  # nine pushes: over the stack
    for i in range(9):
        deep.instrs[i].op, deep.instrs[i].arg, deep.instrs[i].type = L.EXPR_COL, 0, L.TYPE_I32
    deep.n_instrs = 9
    assert run(deep) == L.DQ_E_INVALID


# ---- the row function on the CPU against the reference --------------------------------------------------------------
@pytest.mark.parametrize("bitmaps", [False, True])
def test_host_evaluator_every_operator_and_kind_pair(dq, bitmaps):
    n = 15 * 15 + 7
    for ka, kb in itertools.product(KINDS, KINDS):
        cols = pair_columns(ka, kb, n, bitmaps)
        for op in OPS:
            e = compile_expr(f"{ka}_a {op} {kb}_b IS NOT NULL")
            assert_matches(e, cols, *host_eval(e, cols), what=(ka, op, kb))
    for k in KINDS:
        col = (k, edge_values(k), None)
        for text in (f"-{k}_a > 0", f"{k}_a % 3 > 0", f"{k}_a * 2147483647 > 0", f"7 / {k}_a > 0", f"{k}_a - 3e0 > 0",
                     f"{k}_a + 9223372036854775807 > 0", f"-(-{k}_a - 1) * {k}_a % 7 / 2 > 0"):
            e = compile_expr(text)
            assert_matches(e, [col], *host_eval(e, [col]), what=text)


def contraction_case(kind):
    """(columns a, b, c of one kind, the expression): a * b + c is exactly 0 with two roundings, 2^-54 (f64) / 2^-24
    (f32) with one."""
    f = R.NP[kind]
    a = f(1.0 + 2.0 ** (-27 if kind == "f64" else -12))
    c = f(-(1.0 + 2.0 ** (-26 if kind == "f64" else -11)))
    cols = [(kind, np.full(70, a, f), None), (kind, np.full(70, c, f), None)]
    return cols, compile_expr(f"{kind}_a * {kind}_a + {kind}_b = 0")


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_host_evaluator_does_not_contract(dq, kind):
    cols, e = contraction_case(kind)
    vals, valid, nulls = host_eval(e, cols)
    assert valid.all() and nulls == 0 and (vals == 0.0).all() and e.dtype == kind
    assert_matches(e, cols, vals, valid, nulls)


def test_compiler_under_host_sanitizers(tmp_path):
    """tests/expr_check.cpp: a stand-alone program over dq_pred_compile.cpp with host ASan + UBSan (nothing is loaded
    into Python, no device is used)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "expr_check"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-fno-gpu-sanitize", "-fno-omit-frame-pointer", "-o", str(exe),
                    os.path.join(ROOT, "tests", "expr_check.cpp"), "-fsanitize=address,undefined"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
