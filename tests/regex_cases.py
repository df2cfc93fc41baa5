"""Named inputs of the regex walk tests (test_regex_walk_gpu.py), in plain Python so that test_regex_cases_host.py
checks every case against the oracle and the host DFA walk without a GPU.

The device walk (pred_atom_regex_utf8 / pred_atom_regex in dq_kernels.hip, schema_regex_nonempty in dq_schema.h)
reads a value's first 32 bytes as two 16-byte buffer loads at o0 & ~3, realigns them by o0 & 3, walks the first 28
bytes in 4-byte groups and hands a longer value over to a dword loop at byte 28; a value whose window would reach
past (total & ~3) - 32 goes through the dword loop alone.  The cases sit on those edges.

A case is (name, pred, positives, negatives): every positive must match, no negative may, and where `paired`
positives[i] and negatives[i] differ in one decisive byte (changed or appended).  pred is a pattern (str: hasPattern /
PatternMatch) or a tuple of literals (whole-value mode: `s = 'l'` for one literal, `s IN (...)` for several).
Keeping the classes apart makes a count row-exact: over a table of positives it must equal the number of valid rows,
over a table of negatives 0, and two wrong rows cannot cancel.

A layout is a whole single-column table with its rows in a fixed order (name, pred, cls, rows): the wave-uniform break
with one live lane, and the end of the byte buffer.  cls "pos": every valid row matches; "neg": none does.

No value holds "\\r" (the documented `\\r$` gap stays out of scope).  Nothing here is random but the fixed-seed row
shuffles.
"""
from __future__ import annotations

import random
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

Pred = Union[str, Tuple[str, ...]]
Row = Tuple[bytes, bool]  # (bytes of the slot, valid): a NULL slot may hold bytes, which nothing may read as a value


class Case(NamedTuple):
    name: str
    pred: Pred
    positives: List[bytes]
    negatives: List[bytes]
    paired: bool = True


class Layout(NamedTuple):
    name: str
    pred: Pred
    cls: str
    rows: List[Row]


def u(s: str) -> bytes:
    return s.encode("utf-8")


def sql_of(pred: Tuple[str, ...], column: str = "s") -> str:
    """The predicate text of a whole-value case."""
    if len(pred) == 1:
        return f"{column} = '{pred[0]}'"
    return f"{column} IN (" + ", ".join(f"'{x}'" for x in pred) + ")"


def pred_id(pred: Pred) -> str:
    return pred if isinstance(pred, str) else sql_of(pred)


# ---- value cases ----------------------------------------------------------------------------------------------------

LAST_BYTE_LENGTHS = [1, 3, 4, 5] + list(range(24, 34)) + [56, 57, 200]
LITERAL_LENGTHS = (27, 28, 29, 32)
ALPHABET = "abcdefghijklmnopqrstuvwxyz"


def literal(n: int) -> str:
    """An ASCII literal of n bytes; literals of different lengths share no prefix."""
    return "".join(ALPHABET[(j + n) % 26] for j in range(n))


def _cases() -> List[Case]:
    out: List[Case] = []
    # handover and alignment: filler `a`, the decisive byte last ...
    out.append(Case("last byte", "x$", [u("a" * (n - 1) + "x") for n in LAST_BYTE_LENGTHS],
                    [u("a" * (n - 1) + "y") for n in LAST_BYTE_LENGTHS]))
    # ... and at index 26 .. 29, last or followed by three more bytes
    for k in (26, 27, 28, 29):
        out.append(Case(f"byte {k}", "^a{%d}x" % k, [u("a" * k + "x"), u("a" * k + "xaaa")],
                        [u("a" * k + "y"), u("a" * k + "yaaa")]))
    # multi-byte characters across byte 28: a three-byte character at bytes k .. k + 2, a four-byte one at k .. k + 3
    out.append(Case("euro across", "a€z", [u("a" * k + "€z") for k in (25, 26, 27)] * 2,
                    [u("a" * k + "₭z") for k in (25, 26, 27)] + [u("a" * k + "€y") for k in (25, 26, 27)]))
    out.append(Case("clef across", "𝄞$", [u("a" * k + "𝄞") for k in (24, 25, 26, 27)],
                    [u("a" * k + "𝄟") for k in (24, 25, 26, 27)]))
    # 26 .. 30 characters, not bytes (638 states, 16848 words): one byte appended or removed crosses a bound
    out.append(Case("char count", "^.{26,30}$",
                    [u("é" * 30), u("é" * 25 + "a"), u("a" * 30), u("a" * 26), u("é" * 13 + "a" * 13), u("a" * 27 + "é"),
                     u("é" * 30 + "\n")],
                    [u("é" * 30 + "a"), u("é" * 25), u("a" * 31), u("a" * 25), u("é" * 13 + "a" * 12), u("a" * 24 + "é"),
                     u("é" * 30 + "\na")], paired=False))
    out.append(Case("char count in bytes", "^.{26,30}$", [u("é" * n) for n in (26, 27, 28, 29)],
                    [u("é" * 14), u("é" * 15), u("a" * 14), u("é" * 31)], paired=False))
    # a two-byte class twice: à = C3 A0 is the class's first member, ß = C3 9F the code point before it
    out.append(Case("two-byte class", "[à-ÿ]{2}", [u("a" * k + "éà") for k in (24, 25, 26, 27)],
                    [u("a" * k + "éß") for k in (24, 25, 26, 27)]))
    # `$` before a final line terminator, total lengths 27 .. 30
    pos, neg = [], []
    for n in (27, 28, 29, 30):
        pos += [u("a" * (n - 1) + "x"), u("a" * (n - 2) + "x\n")]
        neg += [u("a" * (n - 1) + "y"), u("a" * (n - 2) + "x\nq")]
    out.append(Case("trailing terminator", "^a+x$", pos, neg))
    # sticky accept at byte 0, and the dead state at byte 0, of values the dword loop would otherwise walk
    out.append(Case("sticky accept", "x", [u("x" + "y" * 40)], [u("y" * 41)]))
    out.append(Case("dead at once", "^b", [u("b" + "a" * 39)], [u("a" * 40)]))
    # whole-value mode: the literal; its last byte changed, one byte more, one byte less
    for n in LITERAL_LENGTHS:
        lit = literal(n)
        out.append(Case(f"literal {n}", (lit,), [u(lit)] * 3, [u(lit[:-1] + "#"), u(lit + "#"), u(lit[:-1])]))
    lits = tuple(literal(n) for n in LITERAL_LENGTHS)
    out.append(Case("literals", lits, [u(x) for x in lits] * 3,
                    [u(x[:-1] + "#") for x in lits] + [u(x + "#") for x in lits] + [u(x[:-1]) for x in lits]))
    return out


CASES: List[Case] = _cases()
PREDS: List[Pred] = list(dict.fromkeys(c.pred for c in CASES))


def class_values(pred: Pred) -> Tuple[List[bytes], List[bytes]]:
    """(positives, negatives) of every case of a pred."""
    pos = [v for c in CASES if c.pred == pred for v in c.positives]
    neg = [v for c in CASES if c.pred == pred for v in c.negatives]
    return list(dict.fromkeys(pos)), list(dict.fromkeys(neg))


def all_values() -> List[bytes]:
    return list(dict.fromkeys(v for c in CASES for v in c.positives + c.negatives))


# ---- tables of the value cases --------------------------------------------------------------------------------------

N_CLASS_ROWS = 1100   # more than one 512-row wave step
N_MIXED_ROWS = 2100
TWO_RANGES = 2 * 16384 + 17  # the predicate pass runs max(1, n / 16384) ranges
LEADS = (0, 1, 2, 3)


def column_rows(values: Sequence[bytes], null_bytes: Sequence[bytes], n: int, lead: int, seed: int) -> List[Row]:
    """n rows: a NULL first row of `lead` bytes (so every value is met at each o0 & 3 over the four leads), then the
    values repeated in freshly shuffled rounds; every eighth row is NULL and its slot holds a value of
    null_bytes (the other class), which a walk that ignored validity would count."""
    rng = random.Random(seed)
    rows: List[Row] = [(b"q" * lead, False)]
    k = 0
    while len(rows) < n:
        block = list(values)
        rng.shuffle(block)
        for v in block:
            if len(rows) >= n:
                break
            if len(rows) % 8 == 7:
                rows.append((null_bytes[k % len(null_bytes)], False))
                k += 1
            rows.append((v, True))
    return rows[:n]


def class_table(cls: str, lead: int) -> Dict[str, List[Row]]:
    """One column per pred (c0, c1, ... in PREDS order) holding that pred's positives (cls "pos") or negatives."""
    out = {}
    for i, p in enumerate(PREDS):
        pos, neg = class_values(p)
        own, other = (pos, neg) if cls == "pos" else (neg, pos)
        out[f"c{i}"] = column_rows(own, other, N_CLASS_ROWS, lead, seed=100 * i + lead)
    return out


def mixed_rows(lead: int, n: int = N_MIXED_ROWS) -> List[Row]:
    """Every value of every case in one column: each pred is evaluated over all of them."""
    vals = all_values()
    return column_rows(vals, vals, n, lead, seed=7 + lead)


# ---- layouts --------------------------------------------------------------------------------------------------------

END_PRED = "^a*x$"   # filler-sensitive: a filler byte misread (a zeroed dword) kills the match, as does the last byte


def _end(n: int, cls: str) -> bytes:
    return b"a" * (n - 1) + (b"x" if cls == "pos" else b"y")


def _rows_of_lengths(lengths: Sequence[Optional[int]], cls: str) -> List[Row]:
    """Rows of END_PRED values of the given byte lengths (None: a NULL row, 0: an empty value -- "neg" only)."""
    return [(b"", False) if n is None else ((b"", True) if n == 0 else (_end(n, cls), True)) for n in lengths]


def _prefix(nbytes: int) -> List[int]:
    """Row lengths summing to nbytes, of mixed sizes and alignments."""
    out, cycle, k = [], (30, 7, 2, 13, 29, 5), 0
    while nbytes > 0:
        n = min(cycle[k % len(cycle)], nbytes)
        out.append(n)
        nbytes -= n
        k += 1
    return out


def _layouts() -> List[Layout]:
    out: List[Layout] = []
    for cls in ("pos", "neg"):
        # wave-uniform break: one live lane among 63 NULL (or empty) rows, in row groups 0 and 7 of a 512-row step.
        # A 40-byte value in row 512 (the next wave's step) keeps both live values' windows whole -- (o0 & ~3) <=
        # (total & ~3) - 32 -- so both are walked from the window, not by the dword loop.
        for lane in (0, 31, 63):
            for n in (28, 29):
                rows = [(b"", cls == "neg" and r % 2 == 0) for r in range(512)]
                rows[lane] = (_end(n, cls), True)
                rows[7 * 64 + lane] = (_end(57 - n, cls), True)
                rows.append((_end(40, cls), True))
                out.append(Layout(f"one live lane {lane} of {n} bytes", END_PRED, cls, rows))
        # buffer end: total % 4 = m, the last row 1, 5 or 28 bytes long and decided by the buffer's final byte
        for m in (0, 1, 2, 3):
            for last in (1, 5, 28):
                out.append(Layout(f"total 100+{m} ends in {last} bytes", END_PRED, cls,
                                  _rows_of_lengths(_prefix(100 + m - last) + [last], cls)))
            # win = (total & ~3) - 32 = 68: the last value starts at win + a (window whole) and at win + 4 + a (not)
            for start in range(68, 76):
                out.append(Layout(f"total 100+{m} last value at {start}", END_PRED, cls,
                                  _rows_of_lengths(_prefix(start) + [100 + m - start], cls)))
        # whole tables under 32 bytes (every value through the dword loop), and at 32, 35, 36 (win = 0, 0, 4)
        for lengths in ([9], [1], [28], [31], [3, 28], [1, 1], [5, 9, 17], [1, 2, 3], [28, 4], [3, 29], [30, 5],
                        [4, 28, 4], [2, 30, 4], [32], [35], [36], [7, 29]):
            out.append(Layout("whole table " + "+".join(map(str, lengths)), END_PRED, cls, _rows_of_lengths(lengths, cls)))
        # the last row NULL, and (no match: "neg" only) empty
        out.append(Layout("last row NULL", END_PRED, cls, _rows_of_lengths([30, 5, 28, None], cls)))
        out.append(Layout("last row NULL, short", END_PRED, cls, _rows_of_lengths([5, 9, None], cls)))
    out.append(Layout("last row empty", END_PRED, "neg", _rows_of_lengths([30, 5, 28, 0], "neg")))
    out.append(Layout("last row empty, short", END_PRED, "neg", _rows_of_lengths([5, 9, 0], "neg")))
    return out


LAYOUTS: List[Layout] = _layouts()


def layout_total(rows: Sequence[Row]) -> int:
    return sum(len(b) for b, _ in rows)


# ---- the DFA budget -------------------------------------------------------------------------------------------------

def long_literal(k: int) -> str:
    """tests/lower_check.cpp's recipe: 300 bytes 'a' + (j + k) % 26; a whole-value DFA of ~300 states x 27 classes."""
    return "".join(ALPHABET[(j + k) % 26] for j in range(300))


def budget_rows() -> List[Optional[bytes]]:
    """~64 rows: the four literals, each with its last byte changed, with byte 150 changed, cut to 299 bytes and
    extended to 301, with NULLs between; shuffled once."""
    rows: List[Optional[bytes]] = []
    for k in range(4):
        lit = long_literal(k)
        rows += [u(lit), u(lit), u(lit[:-1] + "#"), u(lit[:150] + "#" + lit[151:]), u(lit[:-1]), u(lit + "#"), None]
    rows += [u(long_literal(k)) for k in range(4)] * 8 + [None] * 4
    random.Random(3).shuffle(rows)
    return rows


# ---- the schema kernel ----------------------------------------------------------------------------------------------

SCHEMA_PATTERNS = ("^.{26,30}$", "^.{25,30}$")   # 16848 + ~17 K words: one fits kDfaLdsWords (24576), both do not


def schema_values() -> List[bytes]:
    """Character counts 24 .. 31 as ASCII (bytes = characters, across byte 28) and as `é` (two bytes each), with and
    without a final terminator, plus short values and a long one."""
    out = []
    for n in range(24, 32):
        out += [u("a" * n), u("é" * n), u("a" * n + "\n"), u("é" * (n - 1) + "a"), u("a" * (n - 1) + "é")]
    out += [b"", u("a"), u("é" * 14), u("a" * 28 + "\nq"), u("a" * 200)]
    return out


def schema_column(seed: int) -> List[Optional[bytes]]:
    """Twelve rounds of schema_values() in one fixed-seed order, every eighth row NULL (no bytes); a pad row before
    each round makes a round's bytes 1 mod 4, so every value is met at each o0 & 3, in more than one 512-row step."""
    vals = schema_values()
    random.Random(seed).shuffle(vals)
    size = sum(len(v) for v in vals)
    out: List[Optional[bytes]] = []
    for _ in range(12):
        out.append(b"q" * ((1 - size) % 4 or 4))
        for k, v in enumerate(vals):
            out.append(v)
            if k % 7 == 6:
                out.append(None)
    return out


def schema_rows() -> List[Dict[str, Optional[bytes]]]:
    """Columns s and t: the same values in two orders, NULLs in the same rows."""
    return [{"s": a, "t": b} for a, b in zip(schema_column(5), schema_column(6))]
