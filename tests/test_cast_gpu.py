"""dq_cast_utf8 / deequ_amd.casts on the device: Spark 2.2's Cast(StringType -> LongType | DoubleType) as the
ColumnProfiler's second pass uses it (profiles/ColumnProfiler.scala:133-151, 219-235, 330-339, 399-417; pinned by
ColumnProfilerTest.scala:76-113, transcribed into tests/golden/profiler_cast_kats.json).

Expected values come from tests/test_cast_host.py's Python restatement (to_long_ref / to_double_ref) and are
compared bit for bit -- values through view(int64), any NaN being Double.NaN, NULL rows holding 0 -- together with
every validity bit, the zero bits past n_rows included: correct rounding admits no tolerance.  Sizes 1, 63, 64, 65
and 4097 put the column's end before, on and after a 64-row validity word and past one 2048-row block.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_cast_host import adversarial, random_numeric, to_double_ref, to_long_ref

pytestmark = pytest.mark.gpu

REF = {"i64": to_long_ref, "f64": to_double_ref}


@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import deequ_amd

    return deequ_amd


@pytest.fixture(scope="module")
def pool():
    """(the adversarial list padded with random numeric strings to the largest size, the list's own length)"""
    c = adversarial()
    assert len(c) < 4097
    return c + random_numeric(np.random.default_rng(11), 4097 - len(c)), len(c)


def _expected(strings, to):
    """(bits as uint64[n], valid as bool[n]) of the cast of strings (None = NULL row)."""
    want = [None if s is None else REF[to](s) for s in strings]
    valid = np.array([w is not None for w in want], dtype=bool)
    bits = np.array([0 if w is None else w & ((1 << 64) - 1) for w in want], dtype=np.uint64)
    return bits, valid


def _check(col, strings, to):
    n = len(strings)
    bits, valid = _expected(strings, to)
    assert (col.name, col.dtype, col.n_rows) == ("s", to, n)
    got = col.values.cpu().numpy()
    assert len(got) >= 8 * n + 16 and len(got) % 16 == 0
    got_bits = got[:8 * n].view(np.uint64)
    words = (n + 63) // 64
    bm = col.validity.cpu().numpy()
    assert len(bm) == (words + 1) * 8
    got_valid = np.unpackbits(bm[:words * 8], bitorder="little").astype(bool)
    bad = np.nonzero(got_valid[:n] != valid)[0]
    assert len(bad) == 0, [(int(r), strings[r], bool(got_valid[r])) for r in bad[:5]]
    assert not got_valid[n:].any()  # bits past n_rows are zero
    bad = np.nonzero(got_bits != bits)[0]
    assert len(bad) == 0, [(int(r), strings[r], hex(int(got_bits[r])), hex(int(bits[r]))) for r in bad[:5]]


@pytest.mark.parametrize("to", ["i64", "f64"])
@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("bitmap", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_cast_adversarial(dq, pool, n, bitmap, large, to):
    """Every string of the pool in columns of n rows: with a validity bitmap (some rows NULL), and nullable=False
    with a NULL bitmap pointer."""
    from deequ_amd.casts import cast_column
    from deequ_amd.table import utf8_column

    pool, n_adv = pool
    rng = np.random.default_rng(n)
    for lo in range(0, n_adv, n):  # (one column at 4097)
        strings = list(pool[lo:lo + n])
        strings += pool[:n - len(strings)]
        if bitmap:
            strings = [None if rng.random() < 0.15 else s for s in strings]
        col = utf8_column("s", strings, large=large, nullable=bitmap)
        assert (col.validity is None) == (not bitmap)
        _check(cast_column(col, to), strings, to)


@pytest.mark.parametrize("to", ["i64", "f64"])
def test_last_byte_of_the_buffer(dq, to):
    """A 1-byte string that is the very last byte of the data, at offset 4 k, so that its dword is a partial one.  The
    data tensor is the 9-byte head of a longer allocation whose next bytes are digits: a walk that ran past a
    string's end (or took the last dword's other bytes for the string's) would read them and return another number."""
    import torch

    from deequ_amd.casts import cast_column
    from deequ_amd.table import Column

    strings = [b"12.5", b"-3", b"", b"40", b"7"]  # 9 bytes: "7" is byte 8, the first of the third dword
    raw = b"".join(strings)
    assert len(raw) % 4 == 1
    backing = torch.from_numpy(np.frombuffer(raw + b"5" * 23, dtype=np.uint8).copy()).cuda()
    offs = np.zeros(len(strings) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(s) for s in strings])
    col = Column("s", "utf8", len(strings), backing[:len(raw)], None, torch.from_numpy(offs.view(np.uint8).copy()).cuda(),
                 nullable=False, data_bytes=len(raw))
    assert col.values.numel() == 9 and col.values.data_ptr() == backing.data_ptr()
    _check(cast_column(col, to), strings, to)


def test_profile_pass2_reads_chunks_once(dq):
    """profile_pass2 over an iterator of chunks (read once), and over no chunks at all."""
    from deequ_amd.casts import profile_pass2

    chunks = [dq.Table.from_pydict({"item": ("utf8", v)}) for v in (["1", "2", "3"], ["4", "5", "6"])]
    ctx1 = dq.AnalysisRunner.onData(chunks).addAnalyzers([dq.DataType("item")]).run()
    ctx2 = profile_pass2(iter(chunks), ctx1)
    assert ctx2.metric(dq.Sum("item")).value.get() == 21.0 and ctx2.metric(dq.Mean("item")).value.get() == 3.5
    with pytest.raises(ValueError):
        profile_pass2(iter([]), ctx1)


@pytest.mark.parametrize("cap", [None, "16"])
def test_all_hard_column(dq, monkeypatch, cap):
    """65 rows of 40-digit fractions: every row goes through the host's exact tier; with a first list of 16 rows the
    list overflows and the cast is rerun with a list sized for the count."""
    from deequ_amd.casts import cast_column
    from deequ_amd.table import utf8_column
    from tests.test_cast_host import is_hard_ref

    if cap is None:
        monkeypatch.delenv("DQ_CAST_HARD_CAP", raising=False)
    else:
        monkeypatch.setenv("DQ_CAST_HARD_CAP", cap)
    rng = np.random.default_rng(40)
    strings = [("-" if r % 3 == 0 else "") + str(r) + "." + "".join(str(int(d)) for d in rng.integers(1, 10, 40))
               for r in range(65)]
    strings = [s.encode() for s in strings]
    assert all(is_hard_ref(s) for s in strings)
    _check(cast_column(utf8_column("s", strings), "f64"), strings, "f64")


@pytest.mark.parametrize("to", ["i64", "f64"])
def test_cast_then_analyzers(dq, to):
    """cast_column, then Minimum ... Completeness in one scan and ApproxQuantile, over two chunks: the states equal
    those over an i64 / f64 column built by the Python reference from the same strings."""
    from deequ_amd.casts import cast_column
    from deequ_amd.runner import scan_states
    from deequ_amd.table import Table, column_from_numpy, utf8_column

    rng = np.random.default_rng(3)
    rows = random_numeric(rng, 700) + [b"", b"1e5", b"abc", b" 9 ", b"1.5", b"-0.25", b"12345678901234567890", b"."]
    rows = [None if rng.random() < 0.1 else s for s in rows]
    chunks, ref_chunks = [], []
    for part in (rows[:451], rows[451:]):
        chunks.append(Table([cast_column(utf8_column("s", part), to)]))
        bits, valid = _expected(part, to)
        ref_chunks.append(Table([column_from_numpy("s", to, bits.view(np.int64 if to == "i64" else np.float64), valid)]))
    analyzers = [dq.Minimum("s"), dq.Maximum("s"), dq.Mean("s"), dq.StandardDeviation("s"), dq.Sum("s"),
                 dq.Completeness("s")]
    got, want = scan_states(chunks, analyzers), scan_states(ref_chunks, analyzers)
    for a in analyzers:
        assert got[a] is not None and got[a] == want[a], (a, got[a], want[a])
    assert want[dq.Completeness("s")].numMatches < len(rows) * 0.95  # the cast produced NULLs of its own
    for q in (0.1, 0.5, 0.9):
        g, w = dq.ApproxQuantile("s", q).calculate(chunks), dq.ApproxQuantile("s", q).calculate(ref_chunks)
        assert g.value.isSuccess and g.value.get() == w.value.get(), (q, g, w)


def test_profiler_numeric_string_column(dq):
    """ColumnProfilerTest.scala:76-113: the string column item = "1".."6" is typed Integral by pass 1, cast to long
    and profiled by pass 2."""
    from deequ_amd.casts import inferred_types, profile_pass2

    with open(os.path.join(ROOT, "tests", "golden", "profiler_cast_kats.json")) as f:
        kat = json.load(f)["numeric_string_item"]
    t = dq.Table.from_pydict({"item": ("utf8", kat["item"])})
    first = [dq.Completeness("item"), dq.ApproxCountDistinct("item"), dq.DataType("item")]
    ctx1 = dq.AnalysisRunner.onData(t).addAnalyzers(first).run()
    want = kat["expected"]
    assert inferred_types(ctx1) == {"item": want["dataType"]}
    hist = ctx1.metric(dq.DataType("item")).value.get()
    assert {k: v.absolute for k, v in hist.values.items()} == want["typeCounts"]
    assert ctx1.metric(dq.Completeness("item")).value.get() == want["completeness"]
    assert int(ctx1.metric(dq.ApproxCountDistinct("item")).value.get()) == want["approximateNumDistinctValues"]
    ctx2 = profile_pass2(t, ctx1)
    for name, a in (("mean", dq.Mean("item")), ("maximum", dq.Maximum("item")), ("minimum", dq.Minimum("item")),
                    ("sum", dq.Sum("item")), ("stdDev", dq.StandardDeviation("item"))):
        assert ctx2.metric(a).value.get() == want[name], name
    pct = [m for a, m in ctx2.metricMap.items() if isinstance(a, dq.ApproxQuantiles)]
    assert len(pct) == 1 and pct[0].value.isSuccess and len(pct[0].value.get()) == 100
    assert set(pct[0].value.get().values()) <= {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}


def test_regex_numeric_but_cast_fails(dq):
    """Strings that DataType's regex classes numeric but the cast rejects become NULLs of the cast column:
    ".", "- 1.5" and "+ .5" in a Fractional column, "" in an Integral one (ColumnProfiler casts by the inferred type
    of the column, not per value)."""
    from deequ_amd.casts import cast_numeric_string_columns, inferred_types

    frac = ["1.5", ".", "- 1.5", "+ .5", "2.25", None]
    integ = ["1", "", "3", "-4", None, "6"]
    t = dq.Table.from_pydict({"f": ("utf8", frac), "i": ("utf8", integ), "k": ("i64", [1, 2, 3, 4, 5, 6]),
                              "w": ("utf8", ["a", "b", "1", "2", "3", "4"])})
    ctx1 = dq.AnalysisRunner.onData(t).addAnalyzers([dq.DataType(c) for c in ("f", "i", "w")]).run()
    inferred = inferred_types(ctx1)
    assert inferred == {"f": "Fractional", "i": "Integral", "w": "String"}
    casted = cast_numeric_string_columns(t, inferred)
    assert [(n, d) for n, d, _ in casted.schema] == [("f", "f64"), ("i", "i64"), ("k", "i64"), ("w", "utf8")]
    assert casted.columns["k"] is t.columns["k"] and casted.columns["w"] is t.columns["w"]
    ctx = dq.AnalysisRunner.onData(casted).addAnalyzers(
        [dq.Completeness("f"), dq.Completeness("i"), dq.Sum("f"), dq.Sum("i")]).run()
    assert ctx.metric(dq.Completeness("f")).value.get() == 2 / 6   # "1.5" and "2.25"
    assert ctx.metric(dq.Completeness("i")).value.get() == 4 / 6   # "" and the NULL row
    assert ctx.metric(dq.Sum("f")).value.get() == 3.75
    assert ctx.metric(dq.Sum("i")).value.get() == 6.0
    chunks = cast_numeric_string_columns([t, t], inferred)
    assert isinstance(chunks, list) and len(chunks) == 2 and chunks[1].columns["f"].dtype == "f64"
