"""Grouping and histograms of a dictionary-encoded string column on its indices: dq_dict_count, dq_freq_build_weighted
and the routing of build_frequencies / compute_histograms.  Every case builds the data twice -- the dict_utf8 column
and its table.plain_utf8 twin -- and the reference is the plain path (pinned by the reference KATs): frequency states,
every metric of the six single-column grouping analyzers (Entropy bit for bit), compute_histograms and the column's
profile must be EQUAL, never close.  Row counts hit partial 64-row groups, the 2048-row workgroup iteration + 1 and
(1e5 rows) several workgroups; dictionary sizes both sides of the LDS counter table (4096 entries) and of the
"entries <= rows" routing rule."""
import ctypes
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LDS_ENTRIES = 4096  # dq_dict.hip kDictCountLdsEntries: counters in LDS up to here, global adds above
WORDS = ["x", "someone@example.org", "", "12", "été", "NullValue", "long " * 30]


def _mods():
    import deequ_amd as dq
    from deequ_amd import _lib as L, grouping, profiles, runner, table

    return dq, L, grouping, profiles, runner, table


def _analyzers(dq, c="c"):
    return [dq.Uniqueness(c), dq.Distinctness(c), dq.CountDistinct(c), dq.UniqueValueRatio(c), dq.Entropy(c),
            dq.Histogram(c), dq.Histogram(c, None, 2)]


def _bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def _same_metric(got, want):
    """Equal metrics: a float value bit for bit (NaN included), anything else and failures by ==."""
    if got.value.isSuccess and want.value.isSuccess:
        assert _bits(got.value.get()) == _bits(want.value.get()), (got, want)
        assert (got.name, got.instance) == (want.name, want.instance)
    else:
        assert got == want, (got, want)


def _column(indices, entries, nullable=True, large=False, name="c"):
    table = _mods()[5]
    return table.dict_utf8_column(name, list(indices), entries, nullable=nullable, large=large)


def _indices(n, d, null_every=0):
    """every index of [0, d) in turn (so every counter, the last one included, is used once n >= d)"""
    return [None if null_every and i % null_every == null_every - 1 else i % d for i in range(n)]


def _check(data, on_indices=True, columns=("c",), profile=True):
    """`data` (a dictionary Table or chunk list) against its plain_utf8 twin, everything the change covers; returns
    the dictionary side's state."""
    dq, L, grouping, profiles, runner, table = _mods()
    plain = table.plain_utf8(data)
    chunks = runner._chunks(data)
    assert all(t.columns["c"].dtype == "dict_utf8" for t in chunks)
    assert all(t.columns["c"].dtype in ("utf8", "large_utf8") for t in runner._chunks(plain))
    cols = list(columns)
    assert (grouping.index_path_dictionaries(chunks, cols) is not None) == on_indices
    before = table.Dictionary.decode_calls
    sd, sp = grouping.build_frequencies(data, cols), grouping.build_frequencies(plain, cols)
    if on_indices:
        assert table.Dictionary.decode_calls == before
    assert sd == sp  # FrequenciesAndNumRows.__eq__: numRows, keys and counts in export order
    assert sd.frequencies.types == sp.frequencies.types
    a, b = sd.frequencies.summary(sd.numRows), sp.frequencies.summary(sp.numRows)
    assert (a.num_groups, a.num_unique, a.num_values, _bits(a.entropy)) == \
        (b.num_groups, b.num_unique, b.num_values, _bits(b.entropy))
    if cols == ["c"]:
        an = _analyzers(dq)
        got = dq.AnalysisRunner.onData(data).addAnalyzers(an).run()
        want = dq.AnalysisRunner.onData(plain).addAnalyzers(an).run()
        for x in an:
            _same_metric(got.metric(x), want.metric(x))
            _same_metric(x.calculate(data), want.metric(x))
        assert profiles.compute_histograms(data, ["c"]) == profiles.compute_histograms(plain, ["c"])
        if profile:
            assert profiles.ColumnProfiler.profile(data).profiles["c"] == profiles.ColumnProfiler.profile(plain).profiles["c"]
    return sd


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049, 100_003])
def test_row_counts(n):
    dq = _mods()[0]
    d = min(len(WORDS), n)
    s = _check(dq.Table([_column(_indices(n, d, null_every=10), WORDS[:d])]))
    assert s.numRows == n


@pytest.mark.parametrize("d", [1, 2, LDS_ENTRIES, LDS_ENTRIES + 1])
def test_dictionary_sizes(d):
    dq = _mods()[0]
    n = 2 * (LDS_ENTRIES + 1) + 1  # every entry at least once, most twice: groups of count 1, 2 and 3
    entries = [f"v{k}" for k in range(d)]
    s = _check(dq.Table([_column(_indices(n, d, null_every=7), entries)]))
    assert s.frequencies.summary(n).num_groups == d


def test_more_entries_than_rows_takes_the_decoded_path():
    dq, _, _, _, _, table = _mods()
    entries = [f"v{k}" for k in range(300)]
    t = dq.Table([_column([299, 0, None, 7, 299] * 13, entries)])
    before = table.Dictionary.decode_calls
    _check(t, on_indices=False)
    assert table.Dictionary.decode_calls == before + 1  # (the twin's decode: the column keeps it)
    assert dq.grouping.build_frequencies(t, ["c"])._source[0][0].columns["c"].dtype == "utf8"
    # the boundary of the rule: as many entries as rows is still the index path
    _check(dq.Table([_column(_indices(300, 300), entries)]), on_indices=True)
    _check(dq.Table([_column(_indices(299, 299), entries)]), on_indices=False)


@pytest.mark.parametrize("large", [False, True])
def test_duplicate_unused_null_and_empty_entries(large):
    dq = _mods()[0]
    # "a" under 0, 1 and 7: one group; entry 2 NULL; "" a value of its own; 5 and 6 never referenced: no group of count 0
    entries = ["a", "a", None, "", "b", "unused", None, "a", "été"]
    idx = [0, 1, 2, 3, None, 4, 7, 8, 0, 3] * 31
    s = _check(dq.Table([_column(idx, entries, large=large)]))
    keys, counts = s.frequencies.export()
    assert sorted(counts.tolist()) == sorted([4 * 31, 2 * 31, 31, 31])  # a, "", b, été
    assert s.frequencies.summary(s.numRows).num_values == 8 * 31  # the rows of index None and of the NULL entry: NULL
    h = dq.Histogram("c").calculate(dq.Table([_column(idx, entries, large=large)])).value.get()
    assert {k: v.absolute for k, v in h.values.items()} == {"a": 124, "": 62, "b": 31, "été": 31, "NullValue": 62}
    assert h.numberOfBins == 5


@pytest.mark.parametrize("case", ["null_rows", "null_entries", "no_entries"])
def test_all_rows_null(case):
    dq = _mods()[0]
    idx, entries = {"null_rows": ([None] * 70, ["a", "b"]), "null_entries": ([0, 1] * 35, [None, None]),
                    "no_entries": ([None] * 70, [])}[case]
    s = _check(dq.Table([_column(idx, entries)]))
    assert s.frequencies.summary(70).num_groups == 0
    m = dq.Uniqueness("c").calculate(dq.Table([_column(idx, entries)]))
    assert m.value.isFailure and "Empty state" in str(m.value.failed)


def test_nullable_column_without_a_null_and_no_validity_buffer():
    dq = _mods()[0]
    idx = _indices(2049, len(WORDS))
    c = _column(idx, WORDS)
    assert c.validity is not None
    _check(dq.Table([c]))
    c = _column(idx, WORDS + [None], nullable=False)
    assert c.validity is None
    _check(dq.Table([c]))


def test_chunks_sharing_one_dictionary():
    dq, _, _, _, _, table = _mods()
    d = table.Dictionary(table.utf8_column("d", [w.encode() for w in WORDS]))
    chunks = [dq.Table([_column(_indices(2049, 5, null_every=9), d)]), dq.Table([_column([6, 5, None, 6, 0] * 13, d)])]
    s = _check(chunks)
    assert len(s._source[0]) == 1 and s._source[0][0].num_rows == len(WORDS)  # one weighted input chunk: the entries
    assert s.numRows == 2049 + 65


def test_chunks_with_different_overlapping_dictionaries():
    dq = _mods()[0]
    chunks = [dq.Table([_column(_indices(2049, 4, null_every=11), ["a", "b", "c", None])]),
              dq.Table([_column([0, 1, 2, 2, None] * 13, ["c", "d", "a"])]),
              dq.Table([_column([0] * 63, ["only-here"])])]
    s = _check(chunks)
    assert len(s._source[0]) == 3  # one weighted input chunk per distinct Dictionary
    assert s.frequencies.summary(s.numRows).num_groups == 5  # a b c d only-here: equal values of two dictionaries merged


def test_multi_column_grouping_and_mixed_chunks_take_the_decoded_path():
    dq, _, grouping, _, _, table = _mods()
    n = 300
    t = dq.Table([_column(_indices(n, 5, null_every=8), WORDS[:5]),
                  table.column_from_numpy("k", "i64", np.arange(n) % 3, np.arange(n) % 13 != 0)])
    _check(t, on_indices=False, columns=("c", "k"))
    plain = table.plain_utf8(t)
    for a in (dq.Uniqueness(["c", "k"]), dq.CountDistinct(["k", "c"]), dq.MutualInformation("c", "k")):
        _same_metric(dq.AnalysisRunner.onData(t).addAnalyzers([a]).run().metric(a),
                     dq.AnalysisRunner.onData(plain).addAnalyzers([a]).run().metric(a))
    # a plain chunk among dictionary chunks: the whole column is read as bytes
    a, b = dq.Table([_column([0, 1, None, 1] * 20, ["p", "q"])]), dq.Table.from_pydict({"c": ("utf8", ["q", "r", None] * 9)})
    assert grouping.index_path_dictionaries([a, b], ["c"]) is None
    assert grouping.build_frequencies([a, b], ["c"]) == grouping.build_frequencies([table.plain_utf8(a), b], ["c"])


def _raw_column(idx, valid, dictionary):
    """a dict_utf8 column of the int32 indices as given: no host check"""
    table = _mods()[5]
    c = table.column_from_numpy("c", "i32", np.asarray(idx, dtype=np.int32), np.asarray(valid, dtype=bool))
    return table.Column("c", "dict_utf8", c.n_rows, c.values, c.validity, None, nullable=True, dictionary=dictionary)


def _dict_count(col, counts_ptr):
    import torch

    L = _mods()[1]
    view = col.view()
    L.check(L.lib.dq_dict_count(ctypes.byref(view), col.n_rows, counts_ptr, torch.cuda.current_device(),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _bincount(idx, valid, entries):
    idx, valid = np.asarray(idx, dtype=np.int64), np.asarray(valid, dtype=bool)
    nonnull = np.array([e is not None for e in entries] + [False], dtype=bool)
    ok = valid & (idx >= 0) & (idx < len(entries))
    ok &= nonnull[np.where(ok, idx, len(entries))]
    return np.bincount(idx[ok], minlength=len(entries))


@pytest.mark.parametrize("d", [1, 2, LDS_ENTRIES, LDS_ENTRIES + 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049, 100_003])
def test_dict_count_against_bincount_and_accumulates(n, d):
    import torch

    table = _mods()[5]
    rng = np.random.default_rng(n * 7 + d)
    entries = [None if k % 5 == 3 else f"e{k}" for k in range(d)]
    dic = table.Dictionary(table.utf8_column("d", [None if e is None else e.encode() for e in entries]))
    idx = rng.integers(0, d, n)
    idx[: min(n, d)] = np.arange(d)[::-1][: min(n, d)]  # the last entries for certain
    valid = rng.random(n) >= 0.1
    col = _raw_column(idx, valid, dic)
    counts = torch.zeros(d, dtype=torch.int64, device="cuda")
    want = _bincount(idx, valid, entries)
    _dict_count(col, counts.data_ptr())
    assert counts.cpu().numpy().tolist() == want.tolist()
    _dict_count(col, counts.data_ptr())  # the call adds to what is there
    assert counts.cpu().numpy().tolist() == (2 * want).tolist()


@pytest.mark.parametrize("d", [5, LDS_ENTRIES + 1])
def test_out_of_range_index_in_a_valid_row_is_counted_nowhere(d):
    """The kernel's own compare: indices just outside [0, D) in valid rows (the host check bypassed), exactly D
    counters with a guard region on both sides.  Such a row adds nothing, inside or outside counts[0, D)."""
    import torch

    table = _mods()[5]
    guard, sentinel = 64, -0x0123456789ABCDEF
    entries = [f"e{k}" for k in range(d)]
    dic = table.Dictionary(table.utf8_column("d", [e.encode() for e in entries]))
    rng = np.random.default_rng(d)
    n = 4099
    idx = rng.integers(0, d, n)
    bad = np.array([d, d + 1, d + guard - 1, -1, -2, -guard])
    at = rng.choice(n, size=4 * len(bad), replace=False)
    idx[at] = np.tile(bad, 4)
    valid = np.ones(n, dtype=bool)
    valid[at[: len(bad)]] = False  # some of them in NULL rows as well
    assert (valid[at]).sum() == 3 * len(bad)
    buf = torch.full((guard + d + guard,), sentinel, dtype=torch.int64, device="cuda")
    buf[guard:guard + d] = 0
    _dict_count(_raw_column(idx, valid, dic), buf.data_ptr() + 8 * guard)
    got = buf.cpu().numpy()
    assert (got[:guard] == sentinel).all() and (got[guard + d:] == sentinel).all()
    want = _bincount(idx, valid, entries)
    assert got[guard:guard + d].tolist() == want.tolist()
    assert want.sum() == n - 4 * len(bad)


def test_weighted_build_refuses_an_exact_key_column():
    import torch

    dq, L, grouping, _, _, table = _mods()
    t = dq.Table.from_pydict({"k": ("i64", [1, 2, 2])})
    views, rows = grouping._views([t], ["k"])
    w = torch.ones(3, dtype=torch.int64, device="cuda")
    h = ctypes.c_void_p()
    rc = L.lib.dq_freq_build_weighted((ctypes.c_int32 * 1)(L.TYPE_I64), 1, views, rows,
                                      (ctypes.c_void_p * 1)(w.data_ptr()), 1, torch.cuda.current_device(),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(h))
    assert rc == L.DQ_E_UNSUPPORTED and not h.value


def _rows(seed, n):
    rng = np.random.default_rng(seed)
    words = WORDS + ["only-%d" % seed]
    return [None if rng.random() < 0.1 else words[int(i)] for i in rng.integers(0, len(words), n)]


def test_state_round_trips(tmp_path):
    dq, L, grouping, _, _, table = _mods()
    from deequ_amd.state_provider import HdfsStateProvider

    r1, r2 = _rows(1, 700), _rows(2, 400)
    td = dq.Table.from_pydict({"c": ("dict_utf8", r1)})
    tp1, tp2, both = (dq.Table.from_pydict({"c": ("utf8", r)}) for r in (r1, r2, r1 + r2))
    # materialize: the values come from the entries the representative rows point into
    sd, sp = grouping.build_frequencies(td, ["c"]), grouping.build_frequencies(tp1, ["c"])
    assert not sd.frequencies.self_contained()
    sd.materialize()
    assert sd.frequencies.self_contained() and sd._source is None and sd == sp
    assert sd.frequencies.to_bytes() == sp.materialize().frequencies.to_bytes()
    h = dq.Histogram("c")
    assert h.computeMetricFrom(sd) == h.calculate(tp1)
    # persist -> load -> sum with a plain-built state of other rows == the all-plain run
    an = _analyzers(dq)
    pd, pp = HdfsStateProvider(str(tmp_path / "d")), HdfsStateProvider(str(tmp_path / "p"))
    first = dq.AnalysisRunner.onData(td).addAnalyzers(an).saveStatesWith(pd).run()
    want_first = dq.AnalysisRunner.onData(tp1).addAnalyzers(an).saveStatesWith(pp).run()
    want = dq.AnalysisRunner.onData(both).addAnalyzers(an).run()
    for a in an:
        _same_metric(first.metric(a), want_first.metric(a))
        loaded = pd.load(a)
        assert loaded == pp.load(a)
        _same_metric(a.computeMetricFrom(loaded.sum(grouping.build_frequencies(tp2, ["c"]))), want.metric(a))
    # aggregateWith: a dictionary batch on top of the persisted plain state, and the other way round
    got = dq.AnalysisRunner.onData(dq.Table.from_pydict({"c": ("dict_utf8", r2)})).addAnalyzers(an).aggregateWith(pp).run()
    got2 = dq.AnalysisRunner.onData(tp2).addAnalyzers(an).aggregateWith(pd).run()
    for a in an:
        _same_metric(got.metric(a), want.metric(a))
        _same_metric(got2.metric(a), want.metric(a))
    # runOnAggregatedStates over a dictionary-built and a plain-built partition
    p2 = HdfsStateProvider(str(tmp_path / "p2"))
    dq.AnalysisRunner.onData(tp2).addAnalyzers(an).saveStatesWith(p2).run()
    agg = dq.AnalysisRunner.runOnAggregatedStates(tp1.schema, an, [pd, p2])
    for a in an:
        _same_metric(agg.metric(a), want.metric(a))


def test_groupings_and_histograms_of_other_columns_do_not_decode_it():
    """The dictionary column beside groupings that take the decoded route of build_frequencies for OTHER columns (a
    single numeric column, a tuple, MutualInformation) and beside a plain string column over the histogram pass's
    capacity (its fallback is build_frequencies too): none of them may decode it."""
    dq, _, _, profiles, _, table = _mods()
    cap = dq.lib.dq_cat_hist_capacity()
    n = 2 * (cap + 1) + 1
    data = {"c": ("dict_utf8", _rows(5, n)), "k": ("i64", [None if i % 11 == 10 else i % 5 for i in range(n)]),
            "j": ("i64", [i % 3 for i in range(n)]), "p": ("utf8", [None if i > cap and i % 9 == 8 else f"p{i % (cap + 1)}" for i in range(n)])}  # cap + 1 values
    t = dq.Table.from_pydict(data)
    an = [dq.Histogram("c"), dq.Uniqueness("c"), dq.Entropy("c"), dq.Completeness("c"), dq.ApproxCountDistinct("c"),
          dq.Uniqueness("k"), dq.Uniqueness(["k", "j"]), dq.CountDistinct(["j", "p"]), dq.MutualInformation("k", "j"),
          dq.Histogram("p")]
    before = table.Dictionary.decode_calls
    ctx = dq.AnalysisRunner.onData(t).addAnalyzers(an).run()
    assert all(ctx.metric(a).value.isSuccess for a in an), ctx.allMetrics
    assert table.Dictionary.decode_calls == before and getattr(t.columns["c"], "_decoded", None) is None
    hists = profiles.compute_histograms(t, ["c", "p"])
    assert table.Dictionary.decode_calls == before and getattr(t.columns["c"], "_decoded", None) is None
    assert len(hists["p"].values) == cap + 2  # (over capacity: it came through the fallback; + "NullValue")
    prof = profiles.ColumnProfiler.profile(t)
    assert table.Dictionary.decode_calls == before and getattr(t.columns["c"], "_decoded", None) is None
    plain = table.plain_utf8(t)  # the reference, decoded only now
    want = dq.AnalysisRunner.onData(plain).addAnalyzers(an).run()
    for a in an:
        _same_metric(ctx.metric(a), want.metric(a))
    assert hists == profiles.compute_histograms(plain, ["c", "p"])
    assert prof == profiles.ColumnProfiler.profile(plain)


def test_a_run_on_indices_does_not_decode():
    dq, _, _, profiles, _, table = _mods()
    t = dq.Table.from_pydict({"c": ("dict_utf8", _rows(3, 2049))})
    before = table.Dictionary.decode_calls
    an = [dq.Histogram("c"), dq.Uniqueness("c"), dq.Completeness("c"), dq.ApproxCountDistinct("c")]
    ctx = dq.AnalysisRunner.onData(t).addAnalyzers(an).run()
    assert all(ctx.metric(a).value.isSuccess for a in an), ctx.allMetrics
    hist = profiles.compute_histograms(t, ["c"])["c"]
    assert table.Dictionary.decode_calls == before
    assert getattr(t.columns["c"], "_decoded", None) is None
    assert hist == ctx.metric(an[0]).value.get()  # (one Distribution, two routes to it)
    table.plain_utf8(t)  # the counter does see a decode
    assert table.Dictionary.decode_calls == before + 1
    # an analyzer that reads the bytes in the same run: the column is decoded, the results do not change
    mixed = dq.AnalysisRunner.onData(dq.Table.from_pydict({"c": ("dict_utf8", _rows(3, 2049))})).addAnalyzers(
        an + [dq.PatternMatch("c", r"\d+")]).run()
    assert table.Dictionary.decode_calls == before + 2
    for a in an:
        _same_metric(mixed.metric(a), ctx.metric(a))
