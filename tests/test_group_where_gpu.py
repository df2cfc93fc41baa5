"""`where` on the grouping, histogram and quantile analyzers, on the GPU.

The oracle is the definition: A(..., where=w) is the unfiltered A over the table that holds exactly the rows for which
w is TRUE, in their order.  That table is built with the existing predicate_bitmaps + schema.take_rows (for a filter
that selects no row: from the rows' host arrays, an empty table), the unfiltered analyzer runs on it, and states and
metrics are compared exactly -- frequency tables by exported keys and counts (a hashed table's by its groups' values
through take_values), quantiles as exact order statistics.  Entropy and MutualInformation are also held against the
50-digit value of tests/group_ref.py within twice its derived rounding bound, the tolerance
tests/test_group_metrics_exact_gpu.py uses.

The filter of the size / selection grid is `w = 1` over a flag column, so that the selection (all, none, first row,
last row, every 64th row, a random half) is chosen by the test; `a % 2 = 0` and string filters run in their own tests.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

from tests import group_ref as R
from tests import quantile_ref as Q

pytestmark = pytest.mark.gpu

# 1 .. 65: the selection's 32- and 64-bit word edges; 2047 .. 2049 and 3 * 2048 + 17: group_compact's 2048-row tile;
# 255 .. 257 and 1023 .. 1025: the quantile kernels' 256-thread block and the digest pass's 1024-row iteration
SIZES = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 2048 + 17]
SELECTIONS = ["all", "none", "first", "last", "every64", "half"]
MARGIN = 2.0


@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import deequ_amd

    return deequ_amd


def _mask(n: int, kind: str, rng) -> np.ndarray:
    m = np.zeros(n, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "every64":
        m[::64] = True
    elif kind == "half":
        m = rng.random(n) < 0.5
    return m


def _arrays(n: int, mask: np.ndarray, seed: int) -> dict:
    """Host columns: name -> (dtype, values, valid or None)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(-3, 4, n).astype(np.float64)
    f[rng.random(n) < 0.1] = np.nan
    f[rng.random(n) < 0.1] = -0.0
    f[rng.random(n) < 0.1] = 0.0
    words = [b"", b"red", b"green", b"blue", b"a longer value than the others"]
    s = [words[i] for i in rng.integers(0, len(words), n)]
    s_valid = rng.random(n) > 0.2
    # the flag: 1 selected, 0 or NULL not (a NULL `where` is not TRUE)
    w = mask.astype(np.int32)
    w_valid = mask | (rng.random(n) < 0.5)
    return {
        "a": ("i64", rng.integers(0, 7, n).astype(np.int64), rng.random(n) > 0.25),
        "u": ("i64", rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64), None),
        "f": ("f64", f, rng.random(n) > 0.2),
        "i": ("i32", rng.integers(-5, 6, n).astype(np.int32), None),
        "b": ("bool", rng.random(n) < 0.5, rng.random(n) > 0.3),
        "s": ("utf8", [v if ok else None for v, ok in zip(s, s_valid)], None),
        "d": ("decimal(20,2)", [int(v) for v in rng.integers(-3, 4, n)], rng.random(n) > 0.2),
        "w": ("i32", w, w_valid),
    }


def _table(dq, arrays: dict, rows=None):
    from deequ_amd.table import Table, column_from_numpy, utf8_column

    cols = []
    for name, (dt, vals, valid) in arrays.items():
        if rows is not None:
            vals = [vals[i] for i in rows] if isinstance(vals, list) else vals[rows]
            valid = None if valid is None else valid[rows]
        if dt == "utf8":
            cols.append(utf8_column(name, vals))
        else:
            cols.append(column_from_numpy(name, dt, vals, valid))
    return Table(cols)


def _oracle_table(dq, table, arrays, mask, where):
    """The filtered table: predicate_bitmaps + take_rows; for no selected row, the empty table of the same columns."""
    from deequ_amd.rowlevel import _popcount, predicate_bitmaps
    from deequ_amd.schema import take_rows
    from deequ_amd.table import plain_utf8

    bm = predicate_bitmaps([table], where)[0]
    cnt = _popcount(bm)
    assert cnt == int(mask.sum())
    if cnt == 0:
        return _table(dq, arrays, np.zeros(0, dtype=np.int64))
    return take_rows(plain_utf8(table), bm, cnt)


def _groups(state):
    """A frequency state as comparable data: (numRows, sorted (values..., count))."""
    from deequ_amd import _lib as L

    keys, counts = state.frequencies.export()
    if len(keys) == 0:
        return state.numRows, []
    types = state.frequencies.types
    if len(types) == 1 and types[0] not in (L.TYPE_UTF8, L.TYPE_LARGE_UTF8) and (types[0] & 0xFF) != (L.decimal_type(20, 2) & 0xFF):
        return state.numRows, list(zip(keys.tolist(), counts.tolist()))  # one fixed-width column: the keys are the values
    state.materialize()
    vals = [state.frequencies.take_values(keys, c) for c in range(len(state.frequencies.types))]
    return state.numRows, sorted(zip(*vals, counts.tolist()))


def _same_metric(a, b):
    if a.value.isSuccess != b.value.isSuccess:
        return False
    if not a.value.isSuccess:
        return type(a.value.failed) is type(b.value.failed)
    x, y = a.value.get(), b.value.get()
    if isinstance(x, float):
        return Q.same(x, y)
    return x == y


GROUPINGS = [["a"], ["u"], ["f"], ["i"], ["b"], ["s"], ["d"], ["s", "a"]]


@pytest.mark.parametrize("kind", SELECTIONS)
@pytest.mark.parametrize("n", SIZES)
def test_frequencies_and_quantiles_equal_the_filtered_table(dq, n, kind):
    from deequ_amd.grouping import build_frequencies

    rng = np.random.default_rng(n * 7 + len(kind))
    mask = _mask(n, kind, rng)
    arrays = _arrays(n, mask, n)
    table = _table(dq, arrays)
    where = "w = 1"
    oracle = _oracle_table(dq, table, arrays, mask, where)
    for cols in GROUPINGS:
        got = _groups(build_frequencies(table, cols, where))
        want = _groups(build_frequencies(oracle, cols))
        assert got == want, (cols, got[0], want[0])
        assert got[0] == int(mask.sum())
    for cls in (dq.Uniqueness, dq.Distinctness, dq.CountDistinct, dq.UniqueValueRatio):
        m, o = cls(["a"], where).calculate(table), cls(["a"]).calculate(oracle)
        assert _same_metric(m, o), (cls.__name__, m, o)
        if not o.value.isSuccess:  # the unfiltered analyzer's exception text, under the filtered analyzer's name
            assert str(m.value.failed) == str(o.value.failed).replace(str(cls(["a"])), str(cls(["a"], where)))
    # quantiles: rank select and the digest state at relativeError 0 and 0.01
    sel_rows = np.flatnonzero(mask)
    for col in ("a", "f", "i"):
        dt, vals, valid = arrays[col]
        v = vals[sel_rows]
        ok = np.ones(len(v), bool) if valid is None else valid[sel_rows]
        qs = [0.0, 0.25, 0.5, 0.9, 1.0]
        m = dq.ApproxQuantiles(col, qs, 0.0, where=where).calculate(table)
        o = dq.ApproxQuantiles(col, qs, 0.0).calculate(oracle)
        assert m.value.isSuccess and o.value.isSuccess
        assert set(m.value.get()) == set(o.value.get())
        for k in o.value.get():
            assert Q.same(m.value.get()[k], o.value.get()[k]), (col, k)
        ref = Q.select(v.astype(np.float64), ok, qs, 0.0)
        if ref is not None:
            assert all(Q.same(m.value.get()[k], r) for k, r in zip(m.value.get(), ref))
        m1, o1 = dq.ApproxQuantile(col, 0.5, where=where).calculate(table), dq.ApproxQuantile(col, 0.5).calculate(oracle)
        assert _same_metric(m1, o1), (col, m1, o1)
        for rel in (0.0, 0.01):
            s = dq.ApproxQuantile(col, 0.5, rel, where=where).computeStateFrom(table)
            so = dq.ApproxQuantile(col, 0.5, rel).computeStateFrom(oracle)
            assert s == so, (col, rel)


def test_padding_bits_null_pointers_and_chunk_lists_at_the_c_level(dq):
    """dq_freq_build_where over three chunks: a bitmap whose bits past n_rows are all set, a NULL selection pointer
    (every row) and an all-zero bitmap; plus an empty chunk.  Counted against numpy."""
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.grouping import FreqTable, _views
    from deequ_amd.table import Table, column_from_numpy

    rng = np.random.default_rng(5)
    sizes = [70, 130, 0, 2049]
    vals = [rng.integers(0, 5, n).astype(np.int64) for n in sizes]
    valid = [rng.random(n) > 0.2 for n in sizes]
    chunks = [Table([column_from_numpy("x", "i64", v, ok)]) for v, ok in zip(vals, valid)]
    masks = [rng.random(70) < 0.5, None, np.zeros(0, bool), np.zeros(2049, bool)]
    bitmaps = []
    for n, m in zip(sizes, masks):
        if m is None:
            bitmaps.append(None)
            continue
        words = (n + 63) // 64
        bits = np.ones((words + 1) * 64, dtype=bool)  # padding bits past n_rows set: they must not count
        bits[:n] = m
        bitmaps.append(torch.from_numpy(np.packbits(bits, bitorder="little")).cuda())
    ptrs = (ctypes.c_void_p * len(chunks))(*[None if b is None else b.data_ptr() for b in bitmaps])
    types = (ctypes.c_int32 * 1)(L.TYPE_I64)
    views, rows = _views(chunks, ["x"])
    h = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib.dq_freq_build_where(types, 1, views, rows, ptrs, len(chunks), torch.cuda.current_device(), stream,
                                      ctypes.byref(h)))
    keys, counts = FreqTable(h, [L.TYPE_I64]).export()
    picked = np.concatenate([vals[0][masks[0] & valid[0]], vals[1][valid[1]]])
    want_keys, want_counts = np.unique(picked, return_counts=True)
    assert keys.astype(np.int64).tolist() == want_keys.tolist() and counts.tolist() == want_counts.tolist()
    # the same chunks, no selection array at all: dq_freq_build's table
    h2, h3 = ctypes.c_void_p(), ctypes.c_void_p()
    L.check(L.lib.dq_freq_build_where(types, 1, views, rows, None, len(chunks), torch.cuda.current_device(), stream,
                                      ctypes.byref(h2)))
    L.check(L.lib.dq_freq_build(types, 1, views, rows, len(chunks), torch.cuda.current_device(), stream, ctypes.byref(h3)))
    a, b = FreqTable(h2, [L.TYPE_I64]).export(), FreqTable(h3, [L.TYPE_I64]).export()
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


def _chunked(dq, n_per=(300, 0, 2100, 64)):
    """Chunks (one empty; the last has no selected row) and their host arrays."""
    rng = np.random.default_rng(11)
    parts = []
    for k, n in enumerate(n_per):
        mask = np.zeros(n, bool) if k == len(n_per) - 1 else rng.random(n) < 0.4
        parts.append((_arrays(n, mask, 100 + k), mask))
    return [_table(dq, a) for a, _ in parts], parts


def test_chunk_lists_with_an_empty_and_an_unselected_chunk(dq):
    from deequ_amd.grouping import build_frequencies

    chunks, parts = _chunked(dq)
    oracle = [_oracle_table(dq, t, a, m, "w = 1") for t, (a, m) in zip(chunks, parts)]
    for cols in (["a"], ["s"], ["s", "a"], ["d"]):
        assert _groups(build_frequencies(chunks, cols, "w = 1")) == _groups(build_frequencies(oracle, cols))
    m = dq.ApproxQuantile("f", 0.5, where="w = 1").calculate(chunks)
    assert _same_metric(m, dq.ApproxQuantile("f", 0.5).calculate(oracle))


def test_dictionary_column_keeps_its_indices_unless_the_filter_reads_it(dq):
    from deequ_amd import table as T
    from deequ_amd.grouping import build_frequencies

    rng = np.random.default_rng(3)
    n = 2049
    words = ["x", "yy", "zzz", None, "w"]
    idx = [None if r < 0.1 else int(i) for r, i in zip(rng.random(n), rng.integers(0, len(words), n))]
    flag = (rng.random(n) < 0.5).astype(np.int32)
    t = T.Table([T.dict_utf8_column("ds", idx, words), T.column_from_numpy("w", "i32", flag)])
    plain = T.plain_utf8(T.Table([T.dict_utf8_column("ds", idx, words), T.column_from_numpy("w", "i32", flag)]))
    host = [None if i is None or words[i] is None else words[i].encode() for i in idx]

    def expected(mask):
        vals, counts = np.unique(np.array([v for v, m in zip(host, mask) if m and v is not None], dtype=object),
                                 return_counts=True)
        return int(mask.sum()), sorted(zip(vals.tolist(), counts.tolist()))

    before = T.Dictionary.decode_calls
    got = _groups(build_frequencies(t, ["ds"], "w = 1"))
    assert T.Dictionary.decode_calls == before  # counted on the indices
    assert got == expected(flag == 1)
    assert got == _groups(build_frequencies(plain, ["ds"], "w = 1"))
    mask = np.array([v is not None and v != b"yy" for v in host])
    got = _groups(build_frequencies(t, ["ds"], "ds != 'yy'"))
    assert T.Dictionary.decode_calls > before  # the filter reads the column: it is decoded
    assert got == expected(mask)


def test_histogram_exact_binned_and_detail_bins_under_a_filter(dq):
    from deequ_amd.binning import Bins

    rng = np.random.default_rng(9)
    n = 3 * 2048 + 17
    mask = rng.random(n) < 0.3
    arrays = _arrays(n, mask, 9)
    arrays["x"] = ("f64", np.where(rng.random(n) < 0.05, np.nan, rng.normal(0, 3, n)), rng.random(n) > 0.1)
    table = _table(dq, arrays)
    oracle = _oracle_table(dq, table, arrays, mask, "w = 1")
    for col in ("s", "a", "d"):  # exact, with the NullValue bin of the selected NULL rows only
        got = dq.Histogram(col, where="w = 1").calculate(table).value.get()
        want = dq.Histogram(col).calculate(oracle).value.get()
        assert got == want
        valid = arrays[col][2] if arrays[col][2] is not None else np.array([v is not None for v in arrays[col][1]])
        assert got.values["NullValue"].absolute == int((mask & ~valid).sum())
    bins = Bins.edges([-4.0, -1.0, 0.0, 1.0, 4.0])  # below / above / NaN slots are hit
    got = dq.Histogram("x", binning=bins, where="w = 1").calculate(table).value.get()
    want = dq.Histogram("x", binning=bins).calculate(oracle).value.get()
    assert got == want and got.numberOfBins == 8  # 4 bins + below + above + NaN + NullValue
    got = dq.Histogram("u", maxDetailBins=5, where="w = 1").calculate(table).value.get()
    want = dq.Histogram("u", maxDetailBins=5).calculate(oracle).value.get()
    assert got == want and len(got.values) == 5 and got.numberOfBins == int(mask.sum())


def test_entropy_and_mutual_information_under_a_filter(dq):
    rng = np.random.default_rng(21)
    n = 3 * 2048 + 17
    mask = rng.random(n) < 0.5
    arrays = _arrays(n, mask, 21)
    table = _table(dq, arrays)
    oracle = _oracle_table(dq, table, arrays, mask, "w = 1")
    rows = np.flatnonzero(mask)
    N = len(rows)
    ref = R.ref_table([("i64", arrays["a"][1][rows])], [arrays["a"][2][rows]])
    value, bound = R.ref_entropy(ref.counts, N)
    got = dq.Entropy("a", "w = 1").calculate(table).value.get()
    print("entropy |error| / bound", R.error_ratio(got, value, bound))
    assert R.error_ratio(got, value, bound) <= MARGIN
    assert got == dq.Entropy("a").calculate(oracle).value.get()
    ref = R.ref_table([("i64", arrays["a"][1][rows]), ("i32", arrays["i"][1][rows])], [arrays["a"][2][rows], None])
    value, bound = R.ref_mi(ref.joint, N)
    mi = dq.MutualInformation("a", "i", where="w = 1")
    got = mi.calculate(table).value.get()
    print("mi |error| / bound", R.error_ratio(got, value, bound))
    assert R.error_ratio(got, value, bound) <= MARGIN
    want = dq.MutualInformation("a", "i").calculate(oracle).value.get()
    assert R.error_ratio(want, value, bound) <= MARGIN and abs(got - want) <= 2 * MARGIN * bound
    # the state path (joint frequencies of the selected rows)
    prov = dq.InMemoryStateProvider()
    via_state = mi.calculate(table, saveStatesWith=prov).value.get()
    assert R.error_ratio(via_state, value, bound) <= MARGIN and prov.load(mi).numRows == N


def test_filter_with_an_arithmetic_operand_and_a_string_filter(dq):
    from deequ_amd.grouping import build_frequencies

    n = 2049
    arrays = _arrays(n, np.ones(n, bool), 4)
    table = _table(dq, arrays)
    a, a_ok = arrays["a"][1], arrays["a"][2]
    for where, mask in (("a % 2 = 0", a_ok & (a % 2 == 0)),
                        ("s != 'red'", np.array([v is not None and v != b"red" for v in arrays["s"][1]]))):
        oracle = _oracle_table(dq, table, arrays, mask, where)
        for cols in (["u"], ["s"], ["s", "a"]):
            assert _groups(build_frequencies(table, cols, where)) == _groups(build_frequencies(oracle, cols))
        assert _same_metric(dq.ApproxQuantile("f", 0.25, where=where).calculate(table),
                            dq.ApproxQuantile("f", 0.25).calculate(oracle))


def test_runner_shares_builds_and_bitmaps_and_keeps_filters_apart(dq, monkeypatch):
    from deequ_amd import grouping

    n = 4100
    rng = np.random.default_rng(8)
    mask = rng.random(n) < 0.5
    arrays = _arrays(n, mask, 8)
    table = _table(dq, arrays)
    calls = []
    real = grouping.build_frequencies
    monkeypatch.setattr(grouping, "build_frequencies", lambda *a, **k: calls.append(a[1:3]) or real(*a, **k))
    w1, w2 = "w = 1", "a > 2"
    analyzers = [dq.Uniqueness(["u"], w1), dq.Distinctness(["u"], w1), dq.Uniqueness(["u"], w2), dq.Uniqueness(["u"]),
                 dq.Histogram("s", where=w1), dq.ApproxQuantile("f", 0.5, where=w1), dq.Entropy("a", w1)]
    before = grouping.selection_builds
    prov = dq.InMemoryStateProvider()
    ctx = dq.AnalysisRunner.doAnalysisRun(table, analyzers, saveStatesWith=prov)
    assert grouping.selection_builds - before == 2  # w1 once for four kinds of analyzer, w2 once
    assert sorted(map(str, calls)) == sorted(map(str, [(["u"], w1), (["u"], w2), (["u"], None), (["s"], w1), (["a"], w1)]))
    for a in analyzers:
        assert ctx.metric(a).value.isSuccess, (a, ctx.metric(a))
        assert _same_metric(ctx.metric(a), a.calculate(table))
    s1, s2, s0 = (prov.load(a) for a in (analyzers[0], analyzers[2], analyzers[3]))
    assert s1.numRows == int(mask.sum()) and s0.numRows == n
    assert s2.numRows == int((arrays["a"][2] & (arrays["a"][1] > 2)).sum())
    assert prov.load(analyzers[1]) == s1  # same (columns, where): one state


def test_incremental_filtered_halves_equal_the_filtered_whole(dq, tmp_path):
    from deequ_amd.state_provider import HdfsStateProvider

    n = 3000
    rng = np.random.default_rng(13)
    mask = rng.random(n) < 0.5
    arrays = _arrays(n, mask, 13)
    whole = _table(dq, arrays)
    halves = [_table(dq, arrays, np.arange(0, 1400)), _table(dq, arrays, np.arange(1400, n))]
    w = "w = 1"
    analyzers = [dq.Uniqueness(["s", "a"], w), dq.CountDistinct(["u"], w), dq.Entropy("s", w), dq.Histogram("s", where=w),
                 dq.ApproxQuantile("f", 0.5, 0.0, where=w)]
    provs = [HdfsStateProvider(str(tmp_path / f"half{k}")) for k in range(2)]
    for t, p in zip(halves, provs):
        dq.AnalysisRunner.doAnalysisRun(t, analyzers, saveStatesWith=p)
    merged = dq.AnalysisRunner.runOnAggregatedStates(whole.schema, analyzers, provs)
    direct = dq.AnalysisRunner.doAnalysisRun(whole, analyzers)
    for a in analyzers:
        assert _same_metric(merged.metric(a), direct.metric(a)), (a, merged.metric(a), direct.metric(a))
    # aggregateWith: the second half on top of the first half's states
    agg = dq.AnalysisRunner.doAnalysisRun(halves[1], analyzers, aggregateWith=provs[0])
    for a in analyzers:
        assert _same_metric(agg.metric(a), direct.metric(a)), a
    # two filters over the same columns: two files
    p = HdfsStateProvider(str(tmp_path / "two"))
    dq.AnalysisRunner.doAnalysisRun(whole, [dq.Uniqueness(["u"], w), dq.Uniqueness(["u"], "a > 2"), dq.Uniqueness(["u"])],
                                    saveStatesWith=p)
    names = sorted(f.name for f in tmp_path.iterdir() if f.name.startswith("two"))
    assert len(names) == len(set(names)) >= 3


def _orders(dq):
    from deequ_amd.table import Table, column_from_numpy, utf8_column

    ids = np.array([1, 2, 2, 3, 4, 4, 5], dtype=np.int64)
    status = [b"ok", b"ok", b"cancelled", b"ok", b"cancelled", b"cancelled", None]
    return Table([column_from_numpy("id", "i64", ids), utf8_column("status", status)])


def test_verification_suite_filtered_is_unique(dq):
    t = _orders(dq)
    check = dq.Check(dq.CheckLevel.Error, "orders")
    res = dq.VerificationSuite().onData(t).addCheck(check.isUnique("id")).run()
    assert res.status != dq.CheckStatus.Success
    res = dq.VerificationSuite().onData(t).addCheck(check.isUnique("id").where("status != 'cancelled'")).run()
    assert res.status == dq.CheckStatus.Success
    # the reverse: the filter isolates duplicates (id 4 twice among the cancelled rows)
    res = dq.VerificationSuite().onData(t).addCheck(check.isUnique("id").where("status = 'cancelled'")).run()
    assert res.status != dq.CheckStatus.Success
    res = dq.VerificationSuite().onData(t).addCheck(
        check.hasApproxQuantile("id", 0.5, lambda v: v == 2.0).where("status = 'ok'")).run()
    assert res.status == dq.CheckStatus.Success


def test_row_level_filtered_is_unique(dq):
    t = _orders(dq)
    check = dq.Check(dq.CheckLevel.Error, "orders").isUnique("id").where("status = 'cancelled'")
    res = dq.row_level_results([check], t)
    # selected rows 2, 4, 5 (ids 2, 4, 4): rows 4 and 5 are the duplicated selected rows; unselected rows pass
    assert res.as_bool().tolist() == [True, True, True, True, False, False, True]
    failing = res.failing_rows()
    assert failing.num_rows == 2
    ids = failing.columns["id"].values[:16].cpu().numpy().view(np.int64).tolist()
    assert ids == [4, 4]
    masked = dq.row_level_results([check], t, filteredRow="NULL").as_bool()
    assert masked.mask.tolist() == [True, True, False, True, False, False, True]
    assert masked.compressed().tolist() == [True, False, False]
