"""The device DFA walk (pred_atom_regex_utf8 / pred_atom_regex in dq_kernels.hip, schema_regex_nonempty in
dq_schema.h) row by row against the oracle, over the case tables of tests/regex_cases.py: the handover at byte 28, the
four offset alignments, multi-byte characters across the handover, the window's end at (total & ~3) - 32, tables under
32 bytes, the wave-uniform break with one live lane, several DFAs in one program, the DFA budget of one plan as the
device grants it, and the schema kernel's DFAs in LDS and in global memory.

Every comparison is exact.  The row-level kernel's bitmaps are compared bit for bit; the fused scan's counts are taken
over tables of one class, where the count must be the number of valid rows or 0, so two wrong rows cannot cancel.
tests/test_regex_cases_host.py holds every case to its design on the CPU."""

import numpy as np
import pytest

from tests import regex_cases as RC
from tests import schema_ref as R
from tests.test_regex import _host_match
from tests.test_regex_cases_host import compiled, oracle_match

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd
    from deequ_amd import rowlevel, schema  # noqa: F401

    return deequ_amd


# ---- tables and expectations ----------------------------------------------------------------------------------------

def string_column(name, rows, dtype):
    """A device column of (bytes, valid) rows.  utf8 / large_utf8: the bytes of a NULL slot stay in the buffer (Arrow
    allows it; nothing may read them as a value); dict_utf8: a NULL row has no entry."""
    import torch

    from deequ_amd.table import dict_utf8_column, encode_dictionary, pack_validity, utf8_column

    if dtype == "dict_utf8":
        indices, entries = encode_dictionary([b if ok else None for b, ok in rows])
        return dict_utf8_column(name, indices, entries)
    col = utf8_column(name, [b for b, _ in rows], large=dtype == "large_utf8")
    col.validity = torch.from_numpy(pack_validity(np.array([ok for _, ok in rows], dtype=bool))).to(col.values.device)
    return col


def index_column(n):
    from deequ_amd.table import column_from_numpy

    return column_from_numpy("k", "i64", np.arange(n, dtype=np.int64), np.ones(n, dtype=bool))


_MATCH = {}


def want_bits(pred, rows):
    """bool[n]: the row is valid and the oracle matches it (a NULL row never passes)."""
    key = RC.pred_id(pred)
    out = np.zeros(len(rows), dtype=bool)
    for r, (b, ok) in enumerate(rows):
        if ok:
            if (key, b) not in _MATCH:
                _MATCH[(key, b)] = oracle_match(pred, b)
            out[r] = _MATCH[(key, b)]
    return out


def all_bits(t):
    return np.unpackbits(t.cpu().numpy(), bitorder="little").astype(bool)


def mismatches(dq, pred, rows, got, want, limit=6):
    """What a failing comparison prints: the row, its bytes, o0 & 3, and whether the host walk of the same DFA agrees
    with the oracle (it does: the device walk is wrong; it does not: the compiler is)."""
    lines, o = [], np.concatenate([[0], np.cumsum([len(b) for b, _ in rows])])
    pattern, mode = compiled(pred)
    for r in np.flatnonzero(got != want)[:limit]:
        b, ok = rows[r]
        _, host = _host_match(dq, pattern, mode, [b])
        lines.append(f"row {r} valid={ok} o0={o[r]} o0&3={o[r] & 3} len={len(b)} total={o[-1]} bytes={b!r}: device "
                     f"{bool(got[r])}, oracle {bool(want[r])}, host walk {bool(host[0])}")
    return f"{RC.pred_id(pred)}: {int((got != want).sum())} rows differ\n" + "\n".join(lines)


def check_bitmap(dq, pred, rows, bitmap, num_pass=None):
    n = len(rows)
    bits = all_bits(bitmap)
    want = want_bits(pred, rows)
    assert not bits[n:].any(), "bits past n_rows"
    assert (bits[:n] == want).all(), mismatches(dq, pred, rows, bits[:n], want)
    if num_pass is not None:
        assert num_pass == int(want.sum())


def add_constraint(check, pred, column, name):
    if isinstance(pred, str):
        return check.hasPattern(column, pred, name=name)
    return check.satisfies(RC.sql_of(pred, column), name)


def analyzer_of(dq, pred, column, name, where=None):
    if isinstance(pred, str):
        return dq.PatternMatch(column, pred, where)
    return dq.Compliance(name, RC.sql_of(pred, column), where)


def row_program(preds, table, columns=None):
    """(RowProgram, table as the program reads it): pred i over columns[i] (default "s")."""
    from deequ_amd.rowlevel import RowForm, RowProgram, _plain_schema
    from deequ_amd.table import plain_utf8

    table = plain_utf8(table)  # a dictionary-encoded column is decoded on the device
    forms = []
    for i, p in enumerate(preds):
        c = "s" if columns is None else columns[i]
        forms.append(RowForm(f"p{i}", "predicate", ("regex", c, p) if isinstance(p, str) else ("sql", RC.sql_of(p, c))))
    return RowProgram(forms, _plain_schema(table.schema)), table


# ---- the row-level kernel, bit for bit ------------------------------------------------------------------------------

def run_mixed(dq, rows, dtype):
    from deequ_amd.checks import Check, CheckLevel
    from deequ_amd.rowlevel import row_level_results
    from deequ_amd.table import Table

    if dtype == "dict_utf8":  # no bytes in a NULL slot: the offsets a failure prints are the decoded column's
        rows = [(b if ok else b"", ok) for b, ok in rows]
    check = Check(CheckLevel.Error, "walk")
    for i, p in enumerate(RC.PREDS):
        check = add_constraint(check, p, "s", f"p{i}")
    res = row_level_results([check], Table([string_column("s", rows, dtype)]))
    assert res.skipped == [] and len(res.constraints) == len(RC.PREDS)
    for c, p in zip(check.constraints, RC.PREDS):
        out = res.constraints[str(c)]
        check_bitmap(dq, p, rows, out.chunks[0].bitmap, out.num_pass)


@pytest.mark.parametrize("lead", RC.LEADS)
@pytest.mark.parametrize("dtype", ["utf8", "large_utf8", "dict_utf8"])
def test_row_level_every_value_every_pred(dq, dtype, lead):
    """Every value of every case in one column, every pred over it: over the four leads each value is walked at each
    o0 & 3 (int32 offsets), beside lanes of other lengths."""
    run_mixed(dq, RC.mixed_rows(lead), dtype)


def test_row_level_two_ranges(dq):
    run_mixed(dq, RC.mixed_rows(1, RC.TWO_RANGES), "utf8")


@pytest.mark.parametrize("dtype", ["utf8", "large_utf8", "dict_utf8"])
def test_row_level_layouts(dq, dtype):
    """The fixed layouts -- one live lane in a row group, the end of the byte buffer at every total % 4, tables under
    32 bytes -- through one program."""
    from deequ_amd.table import Table, plain_utf8

    prog, failures = None, []
    for lay in RC.LAYOUTS:
        table = Table([string_column("s", lay.rows, dtype)])
        if prog is None:
            prog, _ = row_program([RC.END_PRED], table)
        (bitmap, _, num_pass, _), = prog.evaluate(plain_utf8(table), [False])
        want = want_bits(lay.pred, lay.rows)
        n_valid = sum(ok for _, ok in lay.rows)
        assert int(want.sum()) == (n_valid if lay.cls == "pos" else 0), lay.name
        bits = all_bits(bitmap)
        assert not bits[len(lay.rows):].any(), lay.name
        got = bits[:len(lay.rows)]
        if not (got == want).all():
            failures.append(f"{lay.cls}: {lay.name}\n" + mismatches(dq, lay.pred, lay.rows, got, want))
        else:
            assert num_pass == int(want.sum()), lay.name
    prog.close()
    assert not failures, f"{len(failures)} layouts differ\n" + "\n".join(failures)


def test_three_dfas_over_two_columns(dq):
    """Three DFAs at their own offsets (lit_i) in one program's blob, over two string columns: each output is its own
    pattern over its own column."""
    from deequ_amd.table import Table

    s, t = RC.mixed_rows(1, 1300), RC.mixed_rows(2, 1300)
    table = Table([string_column("s", s, "utf8"), string_column("t", t, "large_utf8")])
    preds, cols = ["x$", "a€z", "^a{28}x"], ["s", "t", "s"]
    prog, table = row_program(preds, table, cols)
    assert prog.info()[:2] == (3, 3)
    res = prog.evaluate(table, [False] * 3)
    for p, c, (bitmap, _, num_pass, _) in zip(preds, cols, res):
        check_bitmap(dq, p, s if c == "s" else t, bitmap, num_pass)
    prog.close()


# ---- the fused scan kernel, by counts over one class ----------------------------------------------------------------

_CLASS = {}


def class_table(cls, lead, dtype):
    from deequ_amd.table import Table

    if (cls, lead, dtype) not in _CLASS:
        cols = RC.class_table(cls, lead)
        _CLASS[(cls, lead, dtype)] = (cols, Table([string_column(c, rows, dtype) for c, rows in cols.items()] +
                                                  [index_column(RC.N_CLASS_ROWS)]))
    return _CLASS[(cls, lead, dtype)]


WHERE, WHERE_ROWS = "k >= 37 AND k < 1001", slice(37, 1001)  # a strict subset that starts and ends inside a word


def expect_counts(cls, cols, states, analyzers, rows_slice=slice(None)):
    for i, p in enumerate(RC.PREDS):
        rows = cols[f"c{i}"][rows_slice]
        n_valid = sum(ok for _, ok in rows)
        st = states[analyzers[i]]
        want = (n_valid if cls == "pos" else 0, len(rows))
        assert (st.numMatches, st.count) == want, (RC.pred_id(p), cls, (st.numMatches, st.count), want)


@pytest.mark.parametrize("lead", RC.LEADS)
@pytest.mark.parametrize("dtype", ["utf8", "large_utf8"])
@pytest.mark.parametrize("cls", ["pos", "neg"])
def test_scan_counts_of_one_class(dq, cls, dtype, lead):
    """PatternMatch / Compliance over a table of positives is exactly (n_valid, n), over negatives (0, n): each pred
    alone, all fused with ApproxCountDistinct, Completeness and a numeric Compliance, and under a `where`."""
    from deequ_amd.runner import scan_states

    cols, table = class_table(cls, lead, dtype)
    n = RC.N_CLASS_ROWS
    own = [analyzer_of(dq, p, f"c{i}", f"p{i}") for i, p in enumerate(RC.PREDS)]
    for i, a in enumerate(own):  # alone: one plan per pred
        st = scan_states(table, [a])[a]
        n_valid = sum(ok for _, ok in cols[f"c{i}"])
        assert (st.numMatches, st.count) == (n_valid if cls == "pos" else 0, n), (RC.pred_id(RC.PREDS[i]), cls)
    extra = [dq.ApproxCountDistinct("c0"), dq.Completeness("c7"), dq.Compliance("numeric", "k >= 300"), dq.Size()]
    states = scan_states(table, own + extra)
    expect_counts(cls, cols, states, own)
    numeric = states[extra[2]]
    assert (numeric.numMatches, numeric.count) == (n - 300, n) and states[extra[3]].numMatches == n
    comp = states[extra[1]]
    assert (comp.numMatches, comp.count) == (sum(ok for _, ok in cols["c7"]), n)
    filtered = [analyzer_of(dq, p, f"c{i}", f"p{i}", WHERE) for i, p in enumerate(RC.PREDS)]
    expect_counts(cls, cols, scan_states(table, filtered), filtered, WHERE_ROWS)


@pytest.mark.parametrize("dtype", ["utf8", "large_utf8"])
def test_scan_counts_of_layouts(dq, dtype):
    """The fixed layouts through one plan of the fused scan: (n_valid, n) or (0, n)."""
    from deequ_amd.runner import ScanPlan
    from deequ_amd.table import Table

    a = dq.PatternMatch("s", RC.END_PRED)
    plan, failures = ScanPlan([a], [("s", dtype, True)]), []
    for lay in RC.LAYOUTS:
        plan.scan(Table([string_column("s", lay.rows, dtype)]))
        st = a._from_result(plan.finish()[0])
        plan.reset()
        n_valid = sum(ok for _, ok in lay.rows)
        if (st.numMatches, st.count) != (n_valid if lay.cls == "pos" else 0, len(lay.rows)):
            failures.append(f"{lay.cls}: {lay.name}: ({st.numMatches}, {st.count}) of {n_valid} valid rows")
    plan.close()
    assert not failures, f"{len(failures)} layouts differ\n" + "\n".join(failures)


# ---- the DFA budget of one plan, on the device ----------------------------------------------------------------------

def budget_preds(k):
    return [(RC.long_literal(j),) for j in range(k)]


def budget_tables():
    """The budget rows by class: table j holds literal j alone (and NULLs) -- pred j counts its valid rows, every other
    pred 0 -- and the last table every near miss, where every pred counts 0."""
    rows = RC.budget_rows()
    lits = [RC.long_literal(j).encode() for j in range(4)]
    tables = [[(b"" if v is None else v, v is not None) for v in rows if v is None or v == lit] for lit in lits]
    tables.append([(b"" if v is None else v, v is not None) for v in rows if v is None or v not in lits])
    return tables


@pytest.mark.parametrize("k", [3, 4])
def test_dfa_budget_in_the_fused_scan(dq, k):
    """Three 300-byte literals are 27141 words of DFAs: one plan, whose dq_pred_scan<true> asks for
    4 waves x 128 x (1 + 3 + 3) + 54288 = 57872 bytes of dynamic LDS; four are over kMaxRegexWords and run as two."""
    from deequ_amd.runner import ScanPlan, explain
    from deequ_amd.table import Table

    preds = budget_preds(k)
    analyzers = [analyzer_of(dq, p, "s", f"l{j}") for j, p in enumerate(preds)]
    schema = [("s", "utf8", True)]
    text = explain(analyzers, schema)
    assert ("2 fused plans" in text) == (k == 4) and ("fused plans" in text) == (k == 4)
    plan = ScanPlan(analyzers, schema)
    for t, rows in enumerate(budget_tables()):
        plan.scan(Table([string_column("s", rows, "utf8")]))
        states = [a._from_result(r) for a, r in zip(analyzers, plan.finish())]
        plan.reset()
        n_valid = sum(ok for _, ok in rows)
        assert n_valid > 0
        for j, st in enumerate(states):
            assert (st.numMatches, st.count) == (n_valid if j == t else 0, len(rows)), (t, j)
    plan.close()


def test_dfa_budget_in_a_row_program(dq):
    """Three long literals run as one row program, row-exact; four are refused (DQ_E_UNSUPPORTED) when the program is
    created, before any launch."""
    from deequ_amd.predicates import UnsupportedPredicate
    from deequ_amd.table import Table

    rows = [(b"" if v is None else v, v is not None) for v in RC.budget_rows()]
    table = Table([string_column("s", rows, "utf8")])
    with pytest.raises(UnsupportedPredicate, match="LDS budget"):
        row_program(budget_preds(4), table)
    prog, table = row_program(budget_preds(3), table)
    for p, (bitmap, _, num_pass, _) in zip(budget_preds(3), prog.evaluate(table, [False] * 3)):
        check_bitmap(dq, p, rows, bitmap, num_pass)
        assert num_pass == 10
    prog.close()


FULL_BUDGET = ["^.{26,30}$", "^.{26,28}$"]  # 16848 + 15756 = 32604 of kMaxRegexWords = 32768 words


def test_a_plan_at_the_full_dfa_budget(dq):
    """Two character-count patterns fill the budget: 4 x 128 x (1 + 2 + 2) + 65216 = 67776 bytes of dynamic LDS, with
    the kernels' static LDS more than 64 KiB a workgroup.  Both interpreter kernels must be granted it and walk
    row-exactly (the scan's counts over all rows equal the bitmaps' popcounts)."""
    from deequ_amd.runner import explain, scan_states
    from deequ_amd.table import Table

    vals = RC.schema_values()
    rows = RC.column_rows(vals, vals, 900, 1, seed=11)
    table = Table([string_column("s", rows, "utf8")])
    prog, _ = row_program(FULL_BUDGET, table)
    res = prog.evaluate(table, [False] * 2)
    for p, (bitmap, _, num_pass, _) in zip(FULL_BUDGET, res):
        check_bitmap(dq, p, rows, bitmap, num_pass)
    prog.close()
    analyzers = [dq.PatternMatch("s", p) for p in FULL_BUDGET]
    assert "fused plans" not in explain(analyzers, table.schema)
    states = scan_states(table, analyzers)
    for a, p in zip(analyzers, FULL_BUDGET):
        assert (states[a].numMatches, states[a].count) == (int(want_bits(p, rows).sum()), len(rows))


# ---- the schema kernel: DFAs in LDS and in global memory ------------------------------------------------------------

@pytest.mark.parametrize("columns,large", [(("s",), ()), (("s", "t"), ()), (("s", "t"), ("t",))])
def test_schema_matches_in_lds_and_global(dq, columns, large):
    """One `matches` DFA (16848 words) is staged in LDS; two (33696) exceed kDfaLdsWords and are walked in global
    memory.  Both verdict bitmaps row by row against the restatement."""
    from deequ_amd.schema import RowLevelSchema, RowLevelSchemaValidator
    from deequ_amd.table import Table, utf8_column

    rows = RC.schema_rows()
    defs = [{"name": c, "kind": "string", "matches": p} for c, p in zip(columns, RC.SCHEMA_PATTERNS)]
    schema = RowLevelSchema()
    for d in defs:
        schema = schema.withStringColumn(d["name"], True, None, None, d["matches"])
    table = Table([utf8_column(c, [r[c] for r in rows], large=c in large) for c in ("s", "t")])
    v = RowLevelSchemaValidator.verdict(table, schema)
    verdicts = [R.cnf(defs, r) for r in rows]
    n = len(rows)
    valid, invalid = all_bits(v.valid), all_bits(v.invalid)
    assert not valid[n:].any() and not invalid[n:].any()
    for name, got, want in (("valid", valid[:n], np.array([m is True for m in verdicts])),
                            ("invalid", invalid[:n], np.array([m is False for m in verdicts]))):
        bad = np.flatnonzero(got != want)
        assert not len(bad), (name, [(int(r), rows[r], bool(got[r])) for r in bad[:5]])
    assert (v.num_valid, v.num_invalid) == (verdicts.count(True), verdicts.count(False))
    assert 0 < v.num_valid < n and v.num_invalid > 0
