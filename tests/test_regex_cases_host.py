"""The regex walk's case tables (tests/regex_cases.py) on the CPU: the oracle classifies every value as the table
says, the host walk of the compiled DFA (dq_regex_match_host) agrees row by row, the compiler takes every pattern,
and the tables have the layouts their names promise.  A case the oracle does not classify as designed is a bug in the
table."""
from __future__ import annotations

import pytest

from oracle import dq_oracle as O
from tests import regex_cases as RC
from tests.test_regex import _host_match


@pytest.fixture(scope="module")
def lib():
    import deequ_amd

    return deequ_amd


def compiled(pred):
    """(pattern, mode) the library walks for a pred: the pattern itself, or the whole-value pattern of the literals."""
    from deequ_amd import _lib as L
    from deequ_amd.analyzers import PlanBuilder

    if isinstance(pred, str):
        return pred, L.REGEX_EXTRACT_NONEMPTY
    b = PlanBuilder([("s", "utf8", True)])
    b.pred(RC.sql_of(pred))
    return b.pool.patterns[-1], L.REGEX_FULL


def dfa_words(pattern: str):
    """(states, 16-bit words) of a pattern's DFA: a 4-word header, 256 byte classes, the accept flags, the table."""
    import ctypes

    from deequ_amd import _lib as L

    ns, nc = ctypes.c_int32(), ctypes.c_int32()
    assert L.lib.dq_regex_info(pattern.encode("utf-8"), L.REGEX_EXTRACT_NONEMPTY, ctypes.byref(ns), ctypes.byref(nc)) == 0
    return ns.value, 4 + 256 + ns.value + ns.value * nc.value


def oracle_match(pred, value: bytes) -> bool:
    if isinstance(pred, str):
        return O.regexp_extract_nonempty(value, pred)
    return value in {x.encode("utf-8") for x in pred}  # whole-value mode: byte equality


def one_byte_apart(a: bytes, b: bytes) -> bool:
    if len(a) == len(b):
        return sum(x != y for x, y in zip(a, b)) == 1
    lo, hi = sorted((a, b), key=len)
    return len(hi) == len(lo) + 1 and hi[:-1] == lo


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_case_is_classified_as_designed(lib, case):
    from deequ_amd import _lib as L

    pattern, mode = compiled(case.pred)
    assert L.lib.dq_regex_info(pattern.encode("utf-8"), mode, None, None) == L.DQ_OK, L.lib.dq_last_error()
    assert case.positives and case.negatives
    for v in case.positives + case.negatives:
        assert b"\r" not in v
        v.decode("utf-8")  # every value is valid UTF-8
    assert [v for v in case.positives if not oracle_match(case.pred, v)] == []
    assert [v for v in case.negatives if oracle_match(case.pred, v)] == []
    values = case.positives + case.negatives
    st, got = _host_match(lib, pattern, mode, values)
    assert st == L.DQ_OK, L.lib.dq_last_error()
    assert list(got) == [True] * len(case.positives) + [False] * len(case.negatives)
    if case.paired:
        assert len(case.positives) == len(case.negatives)
        assert all(one_byte_apart(p, n) for p, n in zip(case.positives, case.negatives))


def test_case_shapes():
    """The lengths and straddles the issue names are in the tables."""
    by = {c.name: c for c in RC.CASES}
    assert sorted({len(v) for v in by["last byte"].positives}) == [1, 3, 4, 5] + list(range(24, 34)) + [56, 57, 200]
    for k in (26, 27, 28, 29):
        assert [v.index(b"x") for v in by[f"byte {k}"].positives] == [k, k]
    # the three-byte character starts at 25, 26, 27 (bytes 26 .. 28 straddle the handover); the four-byte at 24 .. 27
    assert sorted({v.index("€".encode()) for v in by["euro across"].positives}) == [25, 26, 27]
    assert sorted({v.index("𝄞".encode()) for v in by["clef across"].positives}) == [24, 25, 26, 27]
    assert sorted({len(v) for v in by["trailing terminator"].positives}) == [27, 28, 29, 30]
    assert [len(c.pred[0]) for c in RC.CASES if c.name.startswith("literal ")] == [27, 28, 29, 32]
    chars = by["char count"].positives + by["char count in bytes"].positives
    assert any(len(v) != len(v.decode()) and len(v) > 30 >= len(v.decode()) for v in chars)


def test_char_count_dfa_size(lib):
    """`^.{26,30}$` is the large DFA of the tables: 638 states, 16848 words (half of one plan's budget)."""
    assert dfa_words("^.{26,30}$") == (638, 16848)


@pytest.mark.parametrize("layout", RC.LAYOUTS, ids=lambda l: f"{l.cls}: {l.name}")
def test_layout_is_classified_as_designed(lib, layout):
    from deequ_amd import _lib as L

    pattern, mode = compiled(layout.pred)
    values = [b for b, ok in layout.rows if ok]
    assert values
    want = layout.cls == "pos"
    assert [oracle_match(layout.pred, v) for v in values] == [want] * len(values)
    st, got = _host_match(lib, pattern, mode, values)
    assert st == L.DQ_OK and list(got) == [want] * len(values)


def test_layout_shapes():
    names = {}
    for l in RC.LAYOUTS:
        names.setdefault(l.name, []).append(l)
    for m in (0, 1, 2, 3):
        for last in (1, 5, 28):
            for l in names[f"total 100+{m} ends in {last} bytes"]:
                assert RC.layout_total(l.rows) == 100 + m and len(l.rows[-1][0]) == last and l.rows[-1][1]
        win = ((100 + m) & ~3) - 32
        starts = set()
        for start in range(68, 76):
            for l in names[f"total 100+{m} last value at {start}"]:
                assert RC.layout_total(l.rows) == 100 + m and RC.layout_total(l.rows[:-1]) == start
                starts.add(start & ~3)
        assert starts == {win, win + 4}
    totals = {RC.layout_total(l.rows) for n, ls in names.items() if n.startswith("whole table") for l in ls}
    assert {32, 35, 36} <= totals and {t for t in totals if t < 32} >= {1, 2, 6, 9, 28, 31}
    assert {len(l.rows) for n, ls in names.items() if n.startswith("whole table") for l in ls} >= {1, 2, 3}
    for lane in (0, 31, 63):
        for n in (28, 29):
            for l in names[f"one live lane {lane} of {n} bytes"]:
                live = [r for r, (b, _) in enumerate(l.rows) if b]
                assert live == [lane, 7 * 64 + lane, 512] and len(l.rows) == 513
                assert [len(l.rows[r][0]) for r in live] == [n, 57 - n, 40]
                # both live rows of the first step are walked from the window: it is whole for them
                win = (RC.layout_total(l.rows) & ~3) - 32
                assert all((RC.layout_total(l.rows[:r]) & ~3) <= win for r in live[:2])
    for name in ("last row NULL", "last row empty"):
        assert all(l.rows[-1][0] == b"" and l.rows[-1][1] == (name == "last row empty") for l in names[name])
    # each class of each layout but the empty last row (an empty value cannot match)
    assert all(sorted(l.cls for l in ls) == ["neg", "pos"] for n, ls in names.items() if "empty" not in n)


def test_tables_cover_every_alignment():
    """Over the four leads every value of the mixed table is met at each o0 & 3; the tables are longer than one
    512-row step, about one row in eight is NULL, and a NULL slot of a class table holds the other class."""
    seen = {}
    for lead in RC.LEADS:
        rows = RC.mixed_rows(lead)
        assert len(rows) == RC.N_MIXED_ROWS > 512 and rows[0] == (b"q" * lead, False)
        nulls = sum(1 for _, ok in rows if not ok)
        assert len(rows) / 12 < nulls < len(rows) / 6
        o = 0
        for b, ok in rows:
            if ok:
                seen.setdefault(b, set()).add(o & 3)
            o += len(b)
    assert set(seen) == set(RC.all_values()) and all(a == {0, 1, 2, 3} for a in seen.values())
    for cls in ("pos", "neg"):
        t = RC.class_table(cls, 1)
        assert list(t) == [f"c{i}" for i in range(len(RC.PREDS))]
        for i, p in enumerate(RC.PREDS):
            rows = t[f"c{i}"]
            assert len(rows) == RC.N_CLASS_ROWS
            assert {oracle_match(p, b) for b, ok in rows if ok} == {cls == "pos"}
            assert {oracle_match(p, b) for b, ok in rows[1:] if not ok} == {cls != "pos"}


def test_budget_and_schema_inputs(lib):
    from deequ_amd import _lib as L

    rows = RC.budget_rows()
    assert 60 <= len(rows) <= 72 and None in rows
    lits = [RC.long_literal(k).encode() for k in range(4)]
    assert all(len(x) == 300 for x in lits) and len(set(lits)) == 4
    for x in lits:
        assert x in rows and x[:-1] in rows and x + b"#" in rows and x[:-1] + b"#" in rows
        assert x[:150] + b"#" + x[151:] in rows
    words = [dfa_words(p)[1] for p in RC.SCHEMA_PATTERNS]
    # kDfaLdsWords (dq_schema.hip) is 24 * 1024: one DFA is staged in LDS, the two together are walked in global memory
    assert words[0] <= 24 * 1024 < words[0] + words[1]
    vals = RC.schema_values()
    rows = RC.schema_rows()
    for c in ("s", "t"):  # every value at each o0 & 3, about one row in eight NULL
        seen, o = {}, 0
        for r in rows:
            if r[c] is not None:
                seen.setdefault(r[c], set()).add(o & 3)
                o += len(r[c])
        assert all(seen[v] == {0, 1, 2, 3} for v in vals if v)
        nulls = sum(r[c] is None for r in rows)
        assert len(rows) > 512 and len(rows) / 12 < nulls < len(rows) / 6
    assert [r["s"] for r in rows] != [r["t"] for r in rows]
    for p in RC.SCHEMA_PATTERNS:
        st, got = _host_match(lib, p, L.REGEX_EXTRACT_NONEMPTY, vals)
        want = [O.regexp_extract_nonempty(v, p) for v in vals]
        assert st == 0 and list(got) == want and True in want and False in want
