"""Row-level results on the device (deequ_amd/rowlevel.py over dq_row_outcomes / dq_freq_unique_rows) against the
oracle's per-row evaluators: OracleExpr.eval_bool for predicates and `where`, regexp_extract_nonempty for patterns,
frequencies for group counts, numpy unpackbits (little) for the bitmap layout."""
import ctypes

import numpy as np
import pytest

from oracle import dq_oracle as O
from tests.helpers import host_column, oracle_columns

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd
    from deequ_amd import rowlevel  # noqa: F401

    return deequ_amd


def both(data):
    """{"name": (dtype, values)} -> (device Table, oracle columns, n)"""
    from deequ_amd.table import Table

    ocols, n = oracle_columns({"columns": {k: ("utf8" if t == "large_utf8" else t, v) for k, (t, v) in data.items()}})
    return Table.from_pydict(data), ocols, n


def bits_of(t, n):
    return np.unpackbits(t.cpu().numpy(), bitorder="little")[:n].astype(bool)


def oracle_pass(ocols, n, pred, where=None):
    """(pass, applies) of a row-level predicate form."""
    if pred[0] == "regex":
        c = ocols[pred[1]]
        t = np.array([bool(c.valid[i]) and O.regexp_extract_nonempty(c.values[i], pred[2]) for i in range(n)], dtype=bool)
    else:
        t, _ = O.OracleExpr(pred[1]).eval_bool(ocols, n)
    a = np.ones(n, dtype=bool) if where is None else O.OracleExpr(where).eval_bool(ocols, n)[0]
    return t & a, a


def nullable_f64(rng, n):
    vals = rng.normal(size=n).round(2).tolist()
    return [None if rng.random() < 0.2 else v for v in vals]


# ---- tail and layout ------------------------------------------------------------------------------------------------

# dq_row_outcomes launches dq_scan's predicate-pass ranges: max(1, n / DQ_MIN_RANGE_ROWS) of them (pred_ranges in
# dq_plan_host.h, DQ_MIN_RANGE_ROWS = 16384), so 2 * 16384 + 17 rows run as two workgroup ranges
TWO_RANGES = 2 * 16384 + 17
TAIL_SIZES = [1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 17, TWO_RANGES]


@pytest.mark.parametrize("n", TAIL_SIZES)
def test_tail_and_layout(dq, n):
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.rowlevel import RowForm, RowProgram

    rng = np.random.default_rng(n)
    table, ocols, _ = both({"x": ("f64", nullable_f64(rng, n))})
    forms = [RowForm("a", "predicate", ("sql", "x >= 0")), RowForm("b", "predicate", ("sql", "x IS NOT NULL")),
             RowForm("c", "predicate", ("sql", "x >= 0"), "x < 1")]
    prog = RowProgram(forms, table.schema)
    words = (n + 63) // 64
    bufs = [torch.full(((words + 1) * 8,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(6)]  # + a guard word
    pp = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in bufs[:3]])
    ap = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in bufs[3:]])
    npass, napp = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    views = (L.ColumnView * 1)(table.columns["x"].view())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib.dq_row_outcomes(prog.handle, views, n, pp, ap, torch.cuda.current_device(), stream, npass, napp))
    for i, f in enumerate(forms):
        want_p, want_a = oracle_pass(ocols, n, f.pred, f.where)
        for buf, want, count in ((bufs[i], want_p, npass[i]), (bufs[3 + i], want_a, napp[i])):
            raw = buf.cpu().numpy()
            assert (raw[words * 8:] == 0xFF).all(), "guard word touched"
            allbits = np.unpackbits(raw[:words * 8], bitorder="little")
            assert not allbits[n:].any(), "bits past n_rows"
            assert (allbits[:n].astype(bool) == want).all()
            assert count == int(allbits.sum()) == int(want.sum())
    prog.close()


def test_zero_rows_and_rejections(dq):
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.rowlevel import RowForm, RowProgram

    table, _, _ = both({"x": ("f64", [1.0, None, 3.0])})
    prog = RowProgram([RowForm("a", "predicate", ("sql", "x >= 0"))], table.schema)
    buf = torch.full((16,), 0xFF, dtype=torch.uint8, device="cuda")
    pp = (ctypes.c_void_p * 1)(buf.data_ptr())
    npass = (ctypes.c_int64 * 1)(7)
    views = (L.ColumnView * 1)(table.columns["x"].view())
    dev = torch.cuda.current_device()
    assert L.lib.dq_row_outcomes(prog.handle, views, 0, pp, None, dev, None, npass, None) == L.DQ_OK
    assert npass[0] == 0 and (buf.cpu().numpy() == 0xFF).all()
    # rejected on the host, before any launch: a misaligned bitmap, a missing one, a bad device, n_rows < 0
    bad = (ctypes.c_void_p * 1)(buf.data_ptr() + 4)
    assert L.lib.dq_row_outcomes(prog.handle, views, 3, bad, None, dev, None, npass, None) == L.DQ_E_INVALID
    none = (ctypes.c_void_p * 1)(None)
    assert L.lib.dq_row_outcomes(prog.handle, views, 3, none, None, dev, None, npass, None) == L.DQ_E_INVALID
    assert L.lib.dq_row_outcomes(prog.handle, views, 3, pp, None, 4096, None, npass, None) == L.DQ_E_INVALID
    assert L.lib.dq_row_outcomes(prog.handle, views, -1, pp, None, dev, None, npass, None) == L.DQ_E_INVALID
    empty = (L.ColumnView * 1)()
    assert L.lib.dq_row_outcomes(prog.handle, empty, 3, pp, None, dev, None, npass, None) == L.DQ_E_INVALID
    assert (buf.cpu().numpy() == 0xFF).all()
    prog.close()


# ---- three-valued logic ---------------------------------------------------------------------------------------------

def logic_data(n=700, seed=5):
    rng = np.random.default_rng(seed)

    def ints():
        return [None if rng.random() < 0.25 else int(v) for v in rng.integers(-2, 6, size=n)]

    return {"a": ("i64", ints()), "b": ("i32", ints()), "c": ("f64", nullable_f64(rng, n)),
            "s": ("utf8", [None if rng.random() < 0.2 else str(rng.choice(["x", "y", "z", ""])) for _ in range(n)]),
            "z": ("i64", [None] * n)}


PREDICATES = ["a > b OR c IS NULL", "NOT (a < 3)", "COALESCE(a, 0) = 0", "s IN ('x','y')", "z > 0", "z IS NULL"]


@pytest.mark.parametrize("mode", ["TRUE", "NULL"])
@pytest.mark.parametrize("where", [None, "b >= 1", "z = 1"])
def test_three_valued_logic(dq, mode, where):
    from deequ_amd.checks import Check, CheckLevel
    from deequ_amd.rowlevel import row_level_results

    table, ocols, n = both(logic_data())
    check = Check(CheckLevel.Error, "logic")
    for i, p in enumerate(PREDICATES):
        check = check.satisfies(p, f"p{i}")
        if where is not None:
            check = check.where(where)
    res = row_level_results([check], table, filteredRow=mode)
    assert res.skipped == [] and len(res.constraints) == len(PREDICATES)
    all_pass = np.ones(n, dtype=bool)
    for (key, out), p in zip(res.constraints.items(), PREDICATES):
        t, tn = O.OracleExpr(p).eval_bool(ocols, n)
        want_p, want_a = oracle_pass(ocols, n, ("sql", p), where)
        assert not want_p[~tn].any()  # a NULL predicate result is not a pass
        got = res.as_bool(key)
        if where is None:
            assert not np.ma.isMaskedArray(got) or not np.ma.getmaskarray(got).any()
            assert (np.asarray(got) == want_p).all()
            assert (out.num_pass, out.num_rows) == (int(want_p.sum()), n)
        elif mode == "TRUE":  # a filtered row (where FALSE or NULL) passes
            assert (got == (want_p | ~want_a)).all()
            assert out.num_pass == int((want_p | ~want_a).sum())
        else:
            assert (np.ma.getmaskarray(got) == ~want_a).all()
            assert (got.data[want_a] == want_p[want_a]).all()
            assert (out.num_pass, out.num_applies) == (int(want_p.sum()), int(want_a.sum()))
        all_pass &= want_p | ~want_a
    got = res.as_bool("logic")
    if where is None or mode == "TRUE":
        assert (np.ma.getdata(got) == all_pass).all() and not np.ma.getmaskarray(got).any()
    else:  # every constraint has the same filter: a row applies to the check iff the filter is TRUE
        want_a = O.OracleExpr(where).eval_bool(ocols, n)[0]
        assert (np.ma.getmaskarray(got) == ~want_a).all()
        assert (got.data[want_a] == all_pass[want_a]).all()


# ---- patterns -------------------------------------------------------------------------------------------------------

def pattern_values(n=1100, seed=9):
    rng = np.random.default_rng(seed)
    pool = [None, "", "a", "b", "abc", "x@y.co", "someone@example.com", "né@ex.fr", "日本語abc", "ab c", "user@host",
            "cab" * 30, "ü", "@", "a@b.c"]
    vals = [pool[int(i)] for i in rng.integers(0, len(pool), size=n)]
    # a long value whose bytes lie across the end of a 512-row wave step's rows
    vals[511] = "z" * 200 + "abc"
    vals[512] = "q" * 150 + "someone@example.com"
    return vals


@pytest.mark.parametrize("dtype", ["utf8", "large_utf8"])
def test_patterns(dq, dtype):
    from deequ_amd.analyzers import Patterns
    from deequ_amd.checks import Check, CheckLevel
    from deequ_amd.rowlevel import row_level_results

    table, ocols, n = both({"s": (dtype, pattern_values()), "k": ("i32", list(range(1100)))})
    check = (Check(CheckLevel.Error, "pat").hasPattern("s", r"[a-c]+").containsEmail("s")
             .hasPattern("s", r"[a-c]+", name="filtered").where("k >= 300"))
    res = row_level_results([check], table)
    assert res.skipped == []
    for key, pred, where in (("PatternMatchConstraint(s, [a-c]+)", ("regex", "s", r"[a-c]+"), None),
                             ("containsEmail(s)", ("regex", "s", Patterns.EMAIL), None),
                             ("filtered", ("regex", "s", r"[a-c]+"), "k >= 300")):
        want_p, want_a = oracle_pass(ocols, n, pred, where)
        assert not want_p[~ocols["s"].valid].any()  # a NULL value fails
        assert (res.as_bool(key) == (want_p | ~want_a)).all(), key
        assert res.constraints[key].num_pass == int((want_p | ~want_a).sum())


# ---- consistency with the fused scan --------------------------------------------------------------------------------

def test_counts_equal_scan_metrics(dq):
    from deequ_amd.checks import Check, CheckLevel
    from deequ_amd.rowlevel import row_level_results

    data = logic_data(n=2600, seed=21)
    data["t"] = ("utf8", pattern_values(2600, seed=22))
    table, _, n = both(data)
    check = (Check(CheckLevel.Error, "c").isComplete("a").hasCompleteness("c", lambda v: True).where("b > 0")
             .satisfies("a > b OR c IS NULL", "p0").satisfies("COALESCE(a, 0) = 0", "p1").where("c < 0.5")
             .isNonNegative("c").isContainedIn("s", ["x", "y"]).isLessThan("a", "b").where("s = 'x'")
             .hasPattern("t", r"[a-c]+").containsEmail("t").where("a >= 0"))
    res = row_level_results([check], table, filteredRow="NULL")
    assert res.skipped == [] and len(res.constraints) == 9
    for c in check.constraints:
        metric = c.inner.analyzer.calculate(table)
        out = res.constraints[str(c)]
        # integer counts on both sides: the doubles are exactly equal
        assert out.num_pass / out.num_applies == metric.value.get(), str(c)


# ---- uniqueness -----------------------------------------------------------------------------------------------------

def unique_reference(ocols_chunks, columns):
    """Per chunk the oracle's unique rows: every key column non-null and the tuple's count over all chunks 1."""
    freq = {}
    for ocols, n in ocols_chunks:
        for k, c in O.frequencies(ocols, columns, n).items():
            freq[k] = freq.get(k, 0) + c
    out = []
    for ocols, n in ocols_chunks:
        out.append(np.array([all(ocols[c].valid[i] for c in columns) and
                             freq[tuple(O._group_key(ocols[c], i) for c in columns)] == 1 for i in range(n)], dtype=bool))
    return out, sum(1 for c in freq.values() if c == 1)


def key_data(n, seed, kind):
    rng = np.random.default_rng(seed)
    hi = {"distinct": 10 * n + 10, "equal": 1, "mixed": max(2, n // 2)}[kind]
    ids = rng.permutation(10 * n + 10)[:n] if kind == "distinct" else rng.integers(0, hi, size=n)

    def nulls(vals, p=0.1):
        return [None if kind != "distinct" and rng.random() < p else v for v in vals]

    return {"i": ("i64", nulls([int(v) - 5 for v in ids])),
            "s": ("utf8", nulls(["k%d" % v if v != ids[0] else "" for v in ids])),
            "j": ("i32", nulls([int(v) % 3 for v in ids])),
            "d": ("decimal(20,2)", nulls([int(v) * 10 ** 12 + 7 for v in ids]))}


UNIQUE_KEYS = [["i"], ["s"], ["j", "s"], ["d"]]
TWO_TILES = 2 * 2048 + 5  # kCompactRows = 2048 rows per compaction tile (dq_group.hip)


@pytest.mark.parametrize("n,kind", [(1, "mixed"), (64, "mixed"), (65, "distinct"), (65, "equal"), (2049, "mixed"),
                                    (TWO_TILES, "mixed")])
def test_unique_rows(dq, n, kind):
    from deequ_amd.grouping import Uniqueness, build_frequencies
    from deequ_amd.rowlevel import RowForm, _unique_outcome

    table, ocols, _ = both(key_data(n, n, kind))
    for cols in UNIQUE_KEYS:
        out = _unique_outcome(RowForm("u", "unique", columns=tuple(cols)), [table])
        want, n_unique = unique_reference([(ocols, n)], cols)
        got = bits_of(out.chunks[0].bitmap, n)
        assert (got == want[0]).all(), cols
        assert not np.unpackbits(out.chunks[0].bitmap.cpu().numpy(), bitorder="little")[n:].any()
        state = build_frequencies(table, cols)
        assert out.num_pass == int(want[0].sum()) == n_unique == state.frequencies.summary(n).num_unique
        assert out.num_pass / n == Uniqueness(cols).calculate(table).value.get()  # Uniqueness x numRows


def test_unique_rows_across_chunks(dq):
    from deequ_amd.checks import Check, CheckLevel
    from deequ_amd.rowlevel import row_level_results

    a, b = key_data(300, 1, "mixed"), key_data(200, 2, "mixed")
    # a value that occurs once in each chunk is unique in neither
    a["i"][1][0], b["i"][1][0] = 10 ** 9, 10 ** 9
    a["s"][1][1], b["s"][1][1] = "only-twice", "only-twice"
    a["i"][1][2], b["i"][1][2] = 10 ** 9 + 1, 10 ** 9 + 2
    ta, oa, na = both(a)
    tb, ob, nb = both(b)
    check = Check(CheckLevel.Error, "u").isUnique("i").isUnique("s").isPrimaryKey("j", "s").hasUniqueness(["d"], lambda v: True)
    res = row_level_results([check], [ta, tb])
    for c, cols in zip(check.constraints, UNIQUE_KEYS):
        want, n_unique = unique_reference([(oa, na), (ob, nb)], cols)
        got = res.as_bool(str(c))
        assert (got == np.concatenate(want)).all(), cols
        assert res.constraints[str(c)].num_pass == n_unique
    i_bits = res.as_bool("UniquenessConstraint(Uniqueness(List(i)))")
    assert not i_bits[0] and not i_bits[na] and i_bits[2] and i_bits[na + 2]


def test_unique_rows_rejects_a_foreign_table(dq):
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.grouping import build_frequencies

    ta, _, _ = both({"i": ("i64", [1, 2, 3, 4]), "s": ("utf8", ["a", "b", "c", "d"])})
    tb, _, _ = both({"i": ("i64", [1, 2, 9, 4]), "s": ("utf8", ["a", "b", "zz", "d"])})
    bitmap = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for col in ("i", "s"):
        state = build_frequencies(ta, [col])
        views = (L.ColumnView * 1)(tb.columns[col].view())
        rc = L.lib.dq_freq_unique_rows(state.frequencies.handle, None, views, 4, bitmap.data_ptr(), None, None, None, None)
        assert rc == L.DQ_E_INVALID and b"no group" in L.lib.dq_last_error()
        views = (L.ColumnView * 1)(ta.columns[col].view())
        nu = ctypes.c_int64()
        L.check(L.lib.dq_freq_unique_rows(state.frequencies.handle, None, views, 4, bitmap.data_ptr(), None, None,
                                          ctypes.byref(nu), None))
        assert nu.value == 4
        # a probe of another type than the table's is refused before the launch
        other = (ctypes.c_int32 * 1)(L.TYPE_F64)
        assert L.lib.dq_freq_unique_rows(state.frequencies.handle, other, views, 4, bitmap.data_ptr(), None, None, None,
                                         None) == L.DQ_E_INVALID


def test_unique_rows_of_a_dictionary_column(dq):
    from deequ_amd.rowlevel import RowForm, _unique_outcome
    from deequ_amd.table import Table

    rng = np.random.default_rng(3)
    vals = [None if rng.random() < 0.1 else "v%d" % v for v in rng.integers(0, 150, size=400)]
    vals[7] = "once-only"
    plain, ocols, n = both({"s": ("utf8", vals)})
    encoded = Table.from_pydict({"s": ("dict_utf8", vals)})
    form = RowForm("u", "unique", columns=("s",))
    want, n_unique = unique_reference([(ocols, n)], ["s"])
    a = _unique_outcome(form, [plain]).chunks[0]
    b = _unique_outcome(form, [encoded]).chunks[0]  # the table from the indices, the probe on the decoded column
    assert (bits_of(a.bitmap, n) == want[0]).all() and (bits_of(b.bitmap, n) == want[0]).all()
    assert a.num_pass == b.num_pass == n_unique and want[0][7]


# ---- end to end -----------------------------------------------------------------------------------------------------

def column_rows(col):
    vals, valid, _ = host_column(col, col.n_rows)
    return [v if ok else None for v, ok in zip(list(vals), valid)]


def test_end_to_end(dq):
    from deequ_amd.checks import Check, CheckLevel, VerificationSuite

    n = 900
    rng = np.random.default_rng(77)
    ids = [int(v) for v in rng.integers(0, 700, size=n)]
    data = {"id": ("i64", [None if rng.random() < 0.05 else v for v in ids]),
            "x": ("f64", nullable_f64(rng, n)),
            "s": ("utf8", [None if rng.random() < 0.1 else str(rng.choice(["a", "b", "c", "abc", "zz"])) for _ in range(n)]),
            "d": ("dict_utf8", [None if rng.random() < 0.1 else str(rng.choice(["a@b.co", "nope", "ab"])) for _ in range(n)])}
    from deequ_amd.table import Table

    table = Table.from_pydict(data)
    plain = dict(data)
    plain["d"] = ("utf8", data["d"][1])
    _, ocols, _ = both(plain)
    c1 = (Check(CheckLevel.Error, "first").isComplete("id").isUnique("id")
          .satisfies("x >= 0", "x positive").where("id > 300").hasSize(lambda v: v > 0))
    c2 = Check(CheckLevel.Warning, "second").isContainedIn("s", ["a", "b"]).hasPattern("d", r"[a-c]+")
    result = VerificationSuite().onData(table).addCheck(c1).addCheck(c2).run()
    res = result.rowLevelResults(table)
    assert [k for k, _ in res.skipped] == ["SizeConstraint(Size(None))"]
    uniq, _ = unique_reference([(ocols, n)], ["id"])
    p_x, a_x = oracle_pass(ocols, n, ("sql", "x >= 0"), "id > 300")
    want1 = oracle_pass(ocols, n, ("sql", "id IS NOT NULL"))[0] & uniq[0] & (p_x | ~a_x)
    want2 = (oracle_pass(ocols, n, ("sql", "`s` IS NULL OR `s` IN ('a','b')"))[0] &
             oracle_pass(ocols, n, ("regex", "d", r"[a-c]+"))[0])
    assert (res.as_bool("first") == want1).all() and (res.as_bool("second") == want2).all()
    assert (res.as_bool() == (want1 & want2)).all()
    assert (res.checks["first"].num_pass, res.checks["second"].num_pass) == (int(want1.sum()), int(want2.sum()))

    # failing_rows: exactly the failing rows, in source order, values and validity intact; with passing_rows a partition
    source = {name: list(vals) for name, (_, vals) in plain.items()}
    for name, want in ((None, want1 & want2), ("first", want1), ("UniquenessConstraint(Uniqueness(List(id)))", uniq[0])):
        failing, passing = res.failing_rows(name), res.passing_rows(name)
        assert failing.num_rows == int((~want).sum()) and passing.num_rows == int(want.sum())
        assert failing.num_rows + passing.num_rows == n
        for col, vals in source.items():
            expect = [None if v is None else (v.encode() if isinstance(v, str) else v) for v in vals]
            got_f, got_p = column_rows(failing.columns[col]), column_rows(passing.columns[col])
            assert got_f == [expect[i] for i in np.flatnonzero(~want)], (name, col)
            assert got_p == [expect[i] for i in np.flatnonzero(want)], (name, col)


def test_thirty_three_outputs(dq):
    from deequ_amd.checks import Check, CheckLevel
    from deequ_amd.rowlevel import row_level_results

    table, ocols, n = both(logic_data(n=600, seed=33))
    check = Check(CheckLevel.Error, "many")
    texts = [f"a >= {i % 6} OR c > {i / 10}" for i in range(33)]
    for i, p in enumerate(texts):
        check = check.satisfies(p, f"p{i}")
    res = row_level_results([check], table)
    # 32 outputs fit one program's roots, but 32 x (two atoms, OR, STORE) = 128 instructions exceed the program's 96
    # (kMaxInstr): the group of 32 is halved, the 33rd output is a program of its own
    assert [len(p.forms) for p in res.plan.programs] == [16, 16, 1] and len(res.constraints) == 33
    want_all = np.ones(n, dtype=bool)
    for c, p in zip(check.constraints, texts):
        want, _ = oracle_pass(ocols, n, ("sql", p))
        assert (res.as_bool(str(c)) == want).all(), p
        want_all &= want
    assert (res.as_bool("many") == want_all).all()
