"""Arithmetic operands of predicates on the device.

dq_expr_eval against tests/expr_ref.py bit for bit -- values where valid, validity, NULL count; the rules are exact, so
there is no tolerance (Java knows one NaN: every NaN equals every NaN, expr_ref.same) -- at the row counts that cover
the wave, validity-word and block tails, with and without input bitmaps, every operator over every kind pair at MIN /
MAX, +-0.0, NaN, +-inf and subnormals, and the a * b + c cases an FMA would get wrong.  Then end to end at 4097 rows,
as one table and as two chunks: analyzers, `where` filters, checks and row-level results whose predicates hold
arithmetic, against expr_ref for the derived values and the oracle (its comparison rules) for the rest.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

from oracle import dq_oracle as O
from tests import expr_ref as R
from tests.test_expr_host import (KINDS, OPS, SCHEMA, assert_matches, compile_expr, contraction_case, edge_values,
                                  pair_columns, reference)

pytestmark = pytest.mark.gpu

TILE = 1024  # rows of one workgroup of dq_expr_eval: kExprRowsPerBlock (deequ_amd/csrc/dq_expr.hip)
SIZES = [0, 1, 63, 64, 65, 511, 513, 4097]
N = 4097


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deequ_amd

    return deequ_amd


def gpu_eval(expr, cols):
    """dq_expr_eval over numpy columns, into buffers padded as the library pads them and filled with a canary: (values,
    valid, NULL count); nothing beyond the n values and the validity words of the n rows may be written."""
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.table import column_from_numpy

    n = len(cols[0][1])
    size = np.dtype(R.NP[expr.dtype]).itemsize
    words = (n + 63) // 64
    device = [column_from_numpy(f"c{k}", t, np.ascontiguousarray(a, R.NP[t]), valid) for k, (t, a, valid) in enumerate(cols)]
    views = (L.ColumnView * len(cols))(*[c.view() for c in device])
    values = torch.full((max(16, (size * n + 15) // 16 * 16 + 16),), 0xA5, dtype=torch.uint8, device="cuda")
    validity = torch.full(((words + 1) * 8,), 0xA5, dtype=torch.uint8, device="cuda")
    nulls = ctypes.c_int64(-1)
    L.check(L.lib.dq_expr_eval(ctypes.byref(expr.program), views, n, values.data_ptr(), validity.data_ptr(),
                               torch.cuda.current_device(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                               ctypes.byref(nulls)))
    hv, hb = values.cpu().numpy(), validity.cpu().numpy()
    assert (hv[size * n:] == 0xA5).all() and (hb[8 * words:] == 0xA5).all(), "wrote past the rows"
    bits = np.unpackbits(hb[:8 * words], bitorder="little")
    assert not bits[n:].any(), "validity bits past n_rows"
    return hv[:size * n].view(R.NP[expr.dtype]).copy(), bits[:n].astype(bool), nulls.value


# ---- row counts ----------------------------------------------------------------------------------------------------
MIXED = ["i8_a + i16_a * i32_a - i64_a > 0", "f32_a * f32_b + i32_a / i64_b > 0", "i64_a % i32_b = 0",
         "-f64_a % f32_a + 2.5 > 0"]


@functools.lru_cache(maxsize=None)
def mixed_case(bitmaps):
    """The twelve numeric columns of SCHEMA at N rows (edge values at coprime strides) and, per MIXED text, its
    expression, its columns and the reference over the N rows -- computed once; a shorter run is a prefix."""
    r = np.arange(N)
    table = {}
    for k, (name, kind, _) in enumerate(SCHEMA[:12]):
        vals = edge_values(kind)
        table[name] = (kind, vals[(r * (2 * k + 1) + k) % len(vals)], (r % (7 + k) != k % 5) if bitmaps else None)
    out = []
    for text in MIXED:
        e = compile_expr(text)
        cols = [table[c] for c in e.columns]
        out.append((e, cols, reference(e, cols)))
    return out


@pytest.mark.parametrize("bitmaps", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_row_counts(dq, n, bitmaps):
    assert N > 4 * TILE and any(s % 64 for s in SIZES)  # several workgroups; partial waves and words
    for e, cols, (t, vals, ok, _) in mixed_case(bitmaps):
        part = [(k, a[:n], None if valid is None else valid[:n]) for k, a, valid in cols]
        got_vals, got_valid, got_nulls = gpu_eval(e, part)
        assert e.dtype == t and np.array_equal(got_valid, ok[:n]), (e.text, n)
        assert R.same(t, got_vals, vals[:n])[ok[:n]].all(), (e.text, n)
        assert got_nulls == int((~ok[:n]).sum()), (e.text, n)


# ---- every operator over every kind pair --------------------------------------------------------------------------
@pytest.mark.parametrize("bitmaps", [False, True])
@pytest.mark.parametrize("ka", KINDS)
def test_every_operator_and_kind_pair(dq, ka, bitmaps):
    n = 15 * 15 + 7
    for kb in KINDS:
        cols = pair_columns(ka, kb, n, bitmaps)
        for op in OPS:
            e = compile_expr(f"{ka}_a {op} {kb}_b IS NOT NULL")
            assert_matches(e, cols, *gpu_eval(e, cols), what=(ka, op, kb))
    col = (ka, edge_values(ka), (np.arange(len(edge_values(ka))) % 4 != 1) if bitmaps else None)
    for text in (f"-{ka}_a > 0", f"{ka}_a % 3 > 0", f"{ka}_a * 2147483647 > 0", f"7 / {ka}_a > 0", f"{ka}_a - 3e0 > 0",
                 f"{ka}_a + 9223372036854775807 > 0", f"-(-{ka}_a - 1) * {ka}_a % 7 / 2 > 0"):
        e = compile_expr(text)
        assert_matches(e, [col], *gpu_eval(e, [col]), what=text)


def test_chunk_longer_than_the_grid(dq):
    """Past kExprMaxBlocks (2048) workgroups' rows a wave walks the chunk with the grid's stride: every row of
    2048 * 1024 + 65 against the rule restated on whole numpy arrays (Int product wrapped at 32 bits, widened, Long sum
    wrapped at 64), and the rows around the start, the stride boundary and the end against expr_ref."""
    n = 2048 * TILE + 65
    rng = np.random.default_rng(5)
    a = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    b = rng.integers(-70000, 70000, n).astype(np.int32)
    c = rng.integers(-2 ** 63, 2 ** 63 - 1, n).astype(np.int64)
    va, vb = rng.random(n) > 0.1, rng.random(n) > 0.1
    e = compile_expr("i32_a * i32_b + i64_a > 0")
    cols = [("i32", a, va), ("i32", b, vb), ("i64", c, None)]
    vals, valid, nulls = gpu_eval(e, cols)
    with np.errstate(over="ignore"):
        want = (a * b).astype(np.int64) + c
    assert e.dtype == "i64" and np.array_equal(valid, va & vb) and nulls == int((~(va & vb)).sum())
    assert np.array_equal(vals[valid], want[valid]) and not vals[~valid].any()
    for lo, hi in ((0, 70), (2048 * TILE - 70, 2048 * TILE + 65)):
        part = [(t, x[lo:hi], None if v is None else v[lo:hi]) for t, x, v in cols]
        assert_matches(e, part, vals[lo:hi], valid[lo:hi], int((~valid[lo:hi]).sum()))


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_no_contraction(dq, kind):
    """a = b = 1 + 2^-27 (f64) / 1 + 2^-12 (f32), c = -(1 + 2^-26) / -(1 + 2^-11): a * b + c is exactly 0.0 with two
    roundings; an FMA gives 2^-54 / 2^-24."""
    cols, e = contraction_case(kind)
    vals, valid, nulls = gpu_eval(e, cols)
    assert e.dtype == kind and valid.all() and nulls == 0
    assert (vals == 0.0).all(), vals[:4]
    assert_matches(e, cols, vals, valid, nulls)


def test_bad_arguments_launch_nothing(dq):
    import torch

    from deequ_amd import _lib as L

    e = compile_expr("i32_a + i64_a > 0")
    views = (L.ColumnView * 2)()
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    views[0].values = views[1].values = buf.data_ptr()
    args = (0, None, None)
    assert L.lib.dq_expr_eval(ctypes.byref(e.program), views, 0, None, None, *args) == L.DQ_OK  # n = 0
    assert L.lib.dq_expr_eval(ctypes.byref(e.program), views, -1, None, None, *args) == L.DQ_E_INVALID
    assert L.lib.dq_expr_eval(ctypes.byref(e.program), views, 3, None, None, *args) == L.DQ_E_INVALID
    assert L.lib.dq_expr_eval(ctypes.byref(e.program), views, 3, buf.data_ptr() + 4, buf.data_ptr(), *args) == L.DQ_E_INVALID
    assert b"dq_expr_eval" in L.lib.dq_last_error()
    bad = L.ExprProgram.from_buffer_copy(e.program)
    bad.column_types[0] = L.TYPE_UTF8
    assert L.lib.dq_expr_eval(ctypes.byref(bad), views, 3, buf.data_ptr(), buf.data_ptr() + 128, *args) == L.DQ_E_UNSUPPORTED
    bad = L.ExprProgram.from_buffer_copy(e.program)
    bad.n_instrs -= 1
    assert L.lib.dq_expr_eval(ctypes.byref(bad), views, 3, buf.data_ptr(), buf.data_ptr() + 128, *args) == L.DQ_E_INVALID
    views[0].reserved = 1
    assert L.lib.dq_expr_eval(ctypes.byref(e.program), views, 3, buf.data_ptr(), buf.data_ptr() + 128, *args) == L.DQ_E_INVALID
    assert (buf.cpu().numpy() == 0).all()


# ---- end to end ----------------------------------------------------------------------------------------------------
SPLIT = 1500  # the two chunks: rows [0, 1500) and [1500, 4097) -- neither a multiple of 64


@functools.lru_cache(maxsize=None)
def e2e():
    """Host columns a i32, b i32 (zeros and NULLs: divisors), c i64, d f64 (NULLs), and the derived columns of the
    expressions below by expr_ref, as oracle columns next to the source ones."""
    rng = np.random.default_rng(20240)
    a = rng.integers(-50000, 50000, N).astype(np.int32)
    a[::97] = np.iinfo(np.int32).max
    b = rng.integers(-4, 5, N).astype(np.int32)
    b[::89] = np.iinfo(np.int32).min
    c = rng.integers(-2 ** 40, 2 ** 40, N).astype(np.int64)
    d = (rng.standard_normal(N) * 2.0 ** 38).astype(np.float64)
    d[::53] = np.nan
    host = {"a": ("i32", a, None), "b": ("i32", b, rng.random(N) > 0.1), "c": ("i64", c, None),
            "d": ("f64", d, rng.random(N) > 0.05)}
    B = R.binary
    derived = {
        "abc": lambda a, b, c, d: B("+", B("*", a, b), c),   # a * b + c
        "bm2": lambda a, b, c, d: B("%", b, R.literal("2")),  # b % 2
        "q": lambda a, b, c, d: B("/", a, b),                 # a / b
        "apc": lambda a, b, c, d: B("+", a, c),               # a + c
        "b2": lambda a, b, c, d: B("*", b, R.literal("2")),   # b * 2
        "apb": lambda a, b, c, d: B("+", a, b),               # a + b
    }
    cols = {k: O.OColumn(t, v, np.ones(N, bool) if valid is None else valid) for k, (t, v, valid) in host.items()}
    for name, fn in derived.items():
        t, vals, ok = R.rows(fn, *host.values())
        cols[name] = O.OColumn(t, vals, ok)
    return host, cols


def tables(dq, chunked):
    from deequ_amd.table import column_from_numpy

    host, _ = e2e()

    def part(lo, hi):
        return dq.Table([column_from_numpy(k, t, v[lo:hi], None if valid is None else valid[lo:hi])
                         for k, (t, v, valid) in host.items()])

    return [part(0, SPLIT), part(SPLIT, N)] if chunked else part(0, N)


def analyzers(dq):
    """(analyzer, the oracle spec with the derived columns in place of the expressions)"""
    return [
        (dq.Compliance("x", "a * b + c <= d"), ("Compliance", "x", "abc <= d", None)),
        (dq.Mean("a", where="b % 2 = 0"), ("Mean", "a", "bm2 = 0")),
        (dq.Compliance("q", "a / b > 0.5"), ("Compliance", "q", "q > 0.5", None)),
        (dq.Compliance("ee", "a + c > b * 2"), ("Compliance", "ee", "apc > b2", None)),
        (dq.Compliance("null", "a + b IS NULL"), ("Compliance", "null", "apb IS NULL", None)),
        (dq.Completeness("d", where="a * b + c > 0 AND NOT (a / b <= -0.5)"), ("Completeness", "d", "abc > 0 AND NOT (q <= -0.5)")),
    ]


def oracle_value(spec):
    _, cols = e2e()
    return O.compute_state(spec, cols, N).metricValue()


@pytest.mark.parametrize("chunked", [False, True])
def test_analyzers_and_wheres(dq, chunked):
    from deequ_amd import expressions as X

    data = tables(dq, chunked)
    an = analyzers(dq)
    before = X.eval_calls
    ctx = dq.AnalysisRunner.onData(data).addAnalyzers([a for a, _ in an]).run()
    # six distinct expressions, each evaluated once per chunk, however many analyzers read it (a * b + c and a / b
    # are read by two each)
    assert X.eval_calls - before == 6 * (2 if chunked else 1)
    for a, spec in an:
        m = ctx.metric(a)
        assert m.value.isSuccess, (a, m.value)
        assert m.value.get() == oracle_value(spec), (a, m.value.get(), oracle_value(spec))
    first = data[0] if chunked else data
    assert list(first.columns) == ["a", "b", "c", "d"] and first.expr_columns == {}  # nothing outlives the run


def test_check_and_row_level_results(dq):
    _, cols = e2e()
    check = (dq.Check(dq.CheckLevel.Error, "arith")
             .satisfies("a / b > 0.5", "q", lambda v: v < 1.0)
             .satisfies("a * b + c <= d", "x", lambda v: v < 1.0)
             .satisfies("a + b IS NULL", "n", lambda v: v > 0.0).where("a % 3 = 1"))
    want = [O.OracleExpr(t).eval_bool(cols, N)[0] for t in ("q > 0.5", "abc <= d", "apb IS NULL")]
    am3 = R.rows(lambda a: R.binary("%", a, R.literal("3")), e2e()[0]["a"])
    filtered = ~((am3[1] == 1) & am3[2])
    want[2] = want[2] | filtered  # filteredRow = "TRUE": a filtered row passes
    for data in (tables(dq, False), tables(dq, True)):
        result = dq.VerificationSuite().onData(data).addCheck(check).run()
        assert result.status == dq.CheckStatus.Success, result.checkResults
        rows = result.rowLevelResults(data)
        assert rows.skipped == []
        for key, w in zip([str(c) for c in check.constraints], want):
            got = rows.as_bool(key)
            assert got.shape == (N,) and np.array_equal(got, w), (key, np.flatnonzero(got != w)[:5])
        assert np.array_equal(rows.as_bool("arith"), want[0] & want[1] & want[2])
        failing = rows.failing_rows("arith")
        n_fail = sum(t.num_rows for t in failing) if isinstance(failing, list) else failing.num_rows
        assert n_fail == int((~(want[0] & want[1] & want[2])).sum())


def test_states_merge_across_chunks(dq):
    """A state saved for the first chunk and aggregated with the second equals the one-table run; so do the states of
    the two chunks scanned as one dataset."""
    from deequ_amd.state_provider import InMemoryStateProvider

    an = [a for a, _ in analyzers(dq)]
    whole = dq.AnalysisRunner.onData(tables(dq, False)).addAnalyzers(an).run()
    first, second = tables(dq, True)
    states = InMemoryStateProvider()
    dq.AnalysisRunner.onData(first).addAnalyzers(an).saveStatesWith(states).run()
    merged = dq.AnalysisRunner.onData(second).addAnalyzers(an).aggregateWith(states).run()
    for a in an:
        assert merged.metric(a).value.get() == whole.metric(a).value.get(), a


def test_interpreter_and_compiled_agree(dq):
    from deequ_amd.runner import scan_states

    an = [a for a, _ in analyzers(dq)]
    data = tables(dq, True)
    interp = scan_states(data, an, pred_pass="interpreter")
    comp = scan_states(data, an, pred_pass="compiled")
    for a, spec in analyzers(dq):
        assert interp[a].metricValue() == comp[a].metricValue() == oracle_value(spec), a


def test_a_plan_without_the_derived_column_is_refused(dq):
    from deequ_amd.metrics import UnsupportedOnGpuPathException
    from deequ_amd.runner import ScanPlan

    t = tables(dq, False)
    with pytest.raises(UnsupportedOnGpuPathException):
        ScanPlan([dq.Compliance("x", "a * b + c <= d")], t.schema)
