"""Dictionary-encoded string columns (dict_utf8) on the GPU: the entry pass (dq_dict_entries), the plan's dictionary
row pass, dq_dict_decode and the Python routing, against oracle.dq_oracle on the DECODED Python values.  The plain
utf8 path over the decoded column is a second assertion, never the reference.  Row counts hit partial 64-row groups,
32-row validity words and the 2048-row workgroup iteration + 1; dictionary sizes both sides of the LDS staging
threshold (2048 entries) and of one 512-register HLL table."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 65, 2049, 4097]
# one entry per DataType class with the classifier's edge forms, multi-byte UTF-8, every byte length 0..40 (every
# tail round of the hash, the 28-byte window edge, one 32-byte stripe) and one entry over 100 bytes
EDGE = ["12", "-1", "1.5", "true", "x", " 1", "", "false", "+ 7", "-.", "1.2.3", "tru", "é", "日本語テキスト", "12é"]
LENGTHS = ["".join(chr(97 + (i * 7 + k) % 26) for k in range(i)) for i in range(41)]
LONG = ["9" * 101, "long-" + "ab" * 70]
ENTRY_SET = EDGE + LENGTHS[1:] + LONG


def _mods():
    import deequ_amd as dq
    from deequ_amd import _lib as L, runner, table
    from oracle import dq_oracle as O

    return dq, L, runner, table, O


def _decode(indices, entries):
    return [None if i is None or entries[i] is None else entries[i] for i in indices]


def _ocol(values):
    _, _, _, _, O = _mods()
    b = [None if v is None else v.encode("utf-8") for v in values]
    return O.OColumn("utf8", b, np.array([v is not None for v in values], dtype=bool))


def _same(got, want):
    """a deequ_amd state against the oracle's, field by field (HLL words bit-exact)."""
    if want is None:
        assert got is None
        return
    assert got is not None
    for f in dataclasses.fields(want):
        g, w = getattr(got, f.name), getattr(want, f.name)
        assert (tuple(g) if isinstance(w, tuple) else g) == w, (f.name, g, w)


def _analyzers(where=None):
    dq = _mods()[0]
    return [dq.Completeness("c", where), dq.ApproxCountDistinct("c", where), dq.DataType("c", where)]


def _check(tables, values, extra_cols=None, where=None, pred_pass="auto"):
    """the three states of the dictionary table(s) == the oracle on the decoded `values` (and == the plain path)"""
    dq, L, runner, table, O = _mods()
    n = len(values)
    cols = {"c": _ocol(values)}
    cols.update(extra_cols or {})
    an = _analyzers(where)
    got = runner.scan_states(tables, an, pred_pass)
    # (the plain path's Completeness-with-where is a NOT NULL atom on a string column, which only the interpreter
    # takes: the cross-check runs with the default pass, the dictionary path with the one asked for)
    plain = runner.scan_states(table.plain_utf8(tables), an)
    for a, name in zip(an, ("Completeness", "ApproxCountDistinct", "DataType")):
        want = O.compute_state((name, "c", where), cols, n)
        _same(got[a], want)
        _same(plain[a], want)


def _rand_indices(rng, n, d, null_frac):
    idx = [int(i) for i in rng.integers(0, max(d, 1), n)]
    if d == 0:
        return [None] * n
    return [None if rng.random() < null_frac else i for i in idx]


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("null_frac", [0.0, 0.1, 1.0])
def test_row_counts_and_nulls(n, null_frac):
    dq = _mods()[0]
    rng = np.random.default_rng(n + int(null_frac * 10))
    idx = _rand_indices(rng, n, len(ENTRY_SET), null_frac)
    t = dq.Table.from_pydict({"c": ("dict_utf8", (idx, ENTRY_SET))})
    _check(t, _decode(idx, ENTRY_SET))


@pytest.mark.parametrize("d,n", [(1, 65), (2, 2049), (511, 4097), (513, 4097), (2048, 4097), (2049, 4097), (5000, 4097),
                                 (5000, 63), (0, 65)])
def test_dictionary_sizes(d, n):
    dq = _mods()[0]
    rng = np.random.default_rng(d * 31 + n)
    entries = [f"v{k}" if k % 3 else str(k) for k in range(d)]
    idx = _rand_indices(rng, n, d, 0.1)
    t = dq.Table.from_pydict({"c": ("dict_utf8", (idx, entries))})
    _check(t, _decode(idx, entries))


def test_unused_duplicate_null_and_empty_entries():
    dq = _mods()[0]
    # entries 4.. are never referenced: counted, they would add FRACTIONAL / BOOLEAN values and HLL registers
    entries = ["a", "a", None, "", "3.25", "true", "unused-1", "unused-2"] + [f"u{k}" for k in range(600)]
    idx = [0, 1, 2, 3, None, 0, 2, 3, 1] * 29
    t = dq.Table.from_pydict({"c": ("dict_utf8", (idx, entries))})
    values = _decode(idx, entries)
    assert values.count(None) == 3 * 29
    _check(t, values)
    _check(dq.Table.from_pydict({"c": ("dict_utf8", (idx, entries))}, nullable={"c": False}),
           _decode([0 if i is None else i for i in idx], entries))  # (no validity buffer: only entry NULLs)


def test_no_validity_buffer():
    dq, _, _, table, _ = _mods()
    idx = list(range(len(ENTRY_SET))) * 3
    c = table.dict_utf8_column("c", idx, ENTRY_SET, nullable=False)
    assert c.validity is None
    _check(dq.Table([c]), _decode(idx, ENTRY_SET))


def test_chunks_with_different_dictionaries():
    dq = _mods()[0]
    rng = np.random.default_rng(5)
    base = ENTRY_SET[:30]
    dicts = [base, list(reversed(base)), base + ["extra", "7.5"], [f"other{k}" for k in range(9)]]
    tables, values = [], []
    for k, (entries, n) in enumerate(zip(dicts, [2049, 65, 4097, 63])):
        idx = _rand_indices(rng, n, len(entries), 0.1)
        tables.append(dq.Table.from_pydict({"c": ("dict_utf8", (idx, entries))}))
        values += _decode(idx, entries)
    _check(tables, values)


@pytest.mark.parametrize("pred_pass", ["interpreter", "compiled"])
def test_where(pred_pass):
    dq, _, _, _, O = _mods()
    rng = np.random.default_rng(11)
    n = 4097
    idx = _rand_indices(rng, n, len(ENTRY_SET), 0.1)
    x = [None if rng.random() < 0.2 else int(v) for v in rng.integers(-5, 6, n)]
    t = dq.Table.from_pydict({"c": ("dict_utf8", (idx, ENTRY_SET)), "x": ("i64", x)})
    ox = O.OColumn("i64", np.array([0 if v is None else v for v in x]), np.array([v is not None for v in x]))
    _check(t, _decode(idx, ENTRY_SET), {"x": ox}, where="x > 0", pred_pass=pred_pass)


@pytest.mark.parametrize("large", [False, True])
def test_entry_table_words(large):
    """dq_dict_entries word by word against xxhash.xxh64(seed 42) (or the oracle's XXH64) and the oracle's classifier"""
    dq, L, _, table, O = _mods()
    try:
        import xxhash

        h64 = lambda b: xxhash.xxh64(b, seed=42).intdigest()  # noqa: E731
    except ImportError:
        h64 = lambda b: O.xxh64_bytes(b) & (2 ** 64 - 1)  # noqa: E731
    entries = ENTRY_SET + [None, "a", "a"]
    d = table.Dictionary(table.utf8_column("d", [None if e is None else e.encode() for e in entries], large=large))
    got = d.entry_table().cpu().numpy().view(np.uint32)[: len(entries)]
    for e, w in zip(entries, got):
        if e is None:
            assert w == 0
            continue
        b = e.encode()
        x = h64(b)
        v = ((x << 9) | 256) & (2 ** 64 - 1)
        pw = 64 - v.bit_length() + 1
        want = (x >> 55) | pw << 9 | O.datatype_class(b) << 15 | 1 << 18
        assert int(w) == want, (e, hex(int(w)), hex(want))


@pytest.mark.parametrize("large", [False, True])
def test_decode(large):
    dq, L, _, table, _ = _mods()
    entries = ENTRY_SET + [None]
    rng = np.random.default_rng(3)
    for n, nullable in [(0, True), (65, True), (4097, True), (130, False)]:
        idx = _rand_indices(rng, n, len(entries), 0.1 if nullable else 0.0)
        c = table.dict_utf8_column("c", idx, entries, nullable=nullable, large=large)
        assert (c.validity is None) == (not nullable)
        p = table.decoded(c)
        values = _decode(idx, entries)
        ot = np.int64 if large else np.int32
        offs = p.offsets.cpu().numpy().view(ot)[: n + 1]
        data = p.values.cpu().numpy().tobytes()
        bits = np.unpackbits(p.validity.cpu().numpy(), bitorder="little")[:n].astype(bool)
        want = [b"" if v is None else v.encode() for v in values]
        assert list(bits) == [v is not None for v in values]
        assert list(offs) == list(np.concatenate([[0], np.cumsum([len(w) for w in want], dtype=np.int64)]).astype(ot))
        assert data[: p.data_bytes] == b"".join(want)
        assert p.data_bytes == sum(len(w) for w in want)  # (the sizing call's answer)


def test_fast_path_launches_only_the_dictionary_kernel():
    dq, L, runner, _, _ = _mods()
    idx = list(range(len(ENTRY_SET))) * 40
    chunks = [dq.Table.from_pydict({"c": ("dict_utf8", (idx, ENTRY_SET))}) for _ in range(3)]
    plan = runner.ScanPlan(_analyzers(), chunks[0].schema)
    try:
        plan.enable_timing()
        for t in chunks:
            plan.scan(t)
        plan.finish()
        # the whole launch set: the dictionary row pass and the finalize per chunk -- no predicate pass, no pair pass,
        # no column-pass variant (so no utf8_* launch)
        assert plan.num_launches() == 2
        assert [plan.kernel_time(k)[1] for k in (0, 1, 2, 3, L.DICT_TIMER)] == [0, 0, 0, 3, 3]
        assert all(plan.kernel_time(16 + v)[1] == 0 for v in L.VARIANT_NAMES)
    finally:
        plan.close()


def test_entry_table_is_built_once_per_dictionary():
    dq, _, _, table, _ = _mods()
    d = table.Dictionary(table.utf8_column("d", [e.encode() for e in ENTRY_SET]))
    before = table.Dictionary.entries_calls
    chunks = [dq.Table([table.dict_utf8_column("c", [1, 2, None, 3] * 20, d)]) for _ in range(2)]
    _check(chunks, _decode([1, 2, None, 3] * 40, ENTRY_SET))
    assert table.Dictionary.entries_calls == before + 1
    d2 = table.Dictionary(table.utf8_column("d", [b"q", b"r"]))
    _check(chunks + [dq.Table([table.dict_utf8_column("c", [1, 0, None, 1] * 20, d2)])],
           _decode([1, 2, None, 3] * 40, ENTRY_SET) + _decode([1, 0, None, 1] * 20, ["q", "r"]))
    assert table.Dictionary.entries_calls == before + 2


def test_other_uses_are_refused_by_the_plan_and_routed_by_the_runner():
    dq, L, runner, _, O = _mods()
    entries = ["x", "someone@example.org", "y", None, "x@y.io"]
    idx = [0, 1, 2, 3, 4, None, 0, 0, 1] * 9
    values = _decode(idx, entries)
    n = len(values)
    t = dq.Table.from_pydict({"c": ("dict_utf8", (idx, entries))})
    with pytest.raises(L.DQError) as e:  # the C plan itself: DQ_E_UNSUPPORTED with a reason
        runner.ScanPlan([dq.Compliance("p", "c IS NULL")], t.schema)
    assert e.value.status == L.DQ_E_UNSUPPORTED and "dictionary" in str(e.value)
    cols = {"c": _ocol(values)}
    an = [dq.PatternMatch("c", dq.Patterns.EMAIL), dq.Compliance("p", "c = 'x'"), dq.Uniqueness(["c"]),
          dq.Completeness("c"), dq.ApproxCountDistinct("c")]
    specs = [("PatternMatch", "c", dq.Patterns.EMAIL, None), ("Compliance", "p", "c = 'x'", None), ("Uniqueness", ["c"]),
             ("Completeness", "c", None), ("ApproxCountDistinct", "c", None)]
    ctx = dq.AnalysisRunner.onData(t).addAnalyzers(an).run()
    for a, spec in zip(an, specs):
        assert ctx.metric(a).value.get() == O.compute_state(spec, cols, n).metricValue(), a


def test_split_returns_the_decoded_rows():
    dq, _, _, table, _ = _mods()
    from deequ_amd.split import random_split

    idx = [0, 1, None, 2, 1] * 50
    entries = ["a", "bb", "ccc"]
    t = dq.Table.from_pydict({"c": ("dict_utf8", (idx, entries))})
    a, b = random_split(t, 0.3, seed=9), random_split(table.plain_utf8(t), 0.3, seed=9)
    for x, y in ((a.train, b.train), (a.test, b.test)):
        assert x.num_rows == y.num_rows and x.columns["c"].dtype == "utf8"
        assert x.columns["c"].values.cpu().numpy().tobytes()[: x.columns["c"].data_bytes] == \
            y.columns["c"].values.cpu().numpy().tobytes()[: y.columns["c"].data_bytes]


def test_states_persist_load_merge():
    dq, _, runner, _, O = _mods()
    from deequ_amd.state_provider import InMemoryStateProvider

    idx = [0, 1, None, 2, 3, 1] * 30
    entries = ["12", "x", "1.5", "true"]
    dvals = _decode(idx, entries)
    pvals = ["zz", None, "7", "x"] * 25
    td = dq.Table.from_pydict({"c": ("dict_utf8", (idx, entries))})
    tp = dq.Table.from_pydict({"c": ("utf8", pvals)})
    an = _analyzers()
    s1, s2 = InMemoryStateProvider(), InMemoryStateProvider()
    dq.AnalysisRunner.onData(td).addAnalyzers(an).saveStatesWith(s1).run()
    dq.AnalysisRunner.onData(tp).addAnalyzers(an).saveStatesWith(s2).run()
    cols = {"c": _ocol(dvals + pvals)}
    for a, name in zip(an, ("Completeness", "ApproxCountDistinct", "DataType")):
        merged = s1.load(a).sum(s2.load(a))
        _same(merged, O.compute_state((name, "c", None), cols, len(dvals) + len(pvals)))


def test_from_pydict_list_form_encodes_in_first_occurrence_order():
    dq = _mods()[0]
    values = ["b", None, "a", "b", "", "12", "a", None] * 33
    t = dq.Table.from_pydict({"c": ("dict_utf8", values)})
    c = t.columns["c"]
    assert c.dtype == "dict_utf8" and c.dictionary.n_entries == 4
    assert list(c.values.cpu().numpy().view(np.int32)[:8]) == [0, 0, 1, 0, 2, 3, 1, 0]
    _check(t, values)


def _string_bytes(col):
    return col.values.cpu().numpy().tobytes()[: col.data_bytes]


def test_histogram_profile_and_schema_validation_read_the_decoded_column():
    dq, _, _, table, O = _mods()
    from deequ_amd.profiles import ColumnProfiler, compute_histograms
    from deequ_amd.schema import RowLevelSchema, RowLevelSchemaValidator

    entries = ["x", "12", "y", None, "7", "unused"]
    idx = [0, 1, 2, 3, 4, None, 0, 0, 1] * 21
    values = _decode(idx, entries)
    n = len(values)
    t = dq.Table.from_pydict({"c": ("dict_utf8", (idx, entries)), "k": ("i64", list(range(n)))})
    plain = table.plain_utf8(t)
    want = O.histogram({"c": _ocol(values)}, "c", n)  # {value: count}, NULL under "NullValue"
    h = dq.Histogram("c").calculate(t).value.get()
    assert {k: v.absolute for k, v in h.values.items()} == want
    assert {k: v.absolute for k, v in compute_histograms(t, ["c"])["c"].values.items()} == want
    prof, prof_plain = ColumnProfiler.profile(t), ColumnProfiler.profile(plain)
    pc, pp = prof.profiles["c"], prof_plain.profiles["c"]
    assert (pc.completeness, pc.approximateNumDistinctValues, pc.dataType, pc.typeCounts) == \
        (pp.completeness, pp.approximateNumDistinctValues, pp.dataType, pp.typeCounts)
    assert pc.completeness == sum(v is not None for v in values) / n
    assert {k: v.absolute for k, v in pc.histogram.values.items()} == want
    schema = RowLevelSchema().withStringColumn("c", isNullable=False, maxLength=1)
    a, b = RowLevelSchemaValidator.validate(t, schema), RowLevelSchemaValidator.validate(plain, schema)
    assert (a.numValidRows, a.numInvalidRows) == (b.numValidRows, b.numInvalidRows)
    assert a.numValidRows == sum(v is not None and len(v) <= 1 for v in values)
    for x, y in ((a.validRows, b.validRows), (a.invalidRows, b.invalidRows)):
        assert _string_bytes(x.columns["c"]) == _string_bytes(y.columns["c"])
        assert x.columns["k"].values.cpu().numpy().tobytes() == y.columns["k"].values.cpu().numpy().tobytes()


def _states_of(results, analyzers):
    return [a._from_result(r) for a, r in zip(analyzers, results)]


def test_arrow_end_to_end():
    pa = pytest.importorskip("pyarrow")
    dq, L, runner, table, O = _mods()
    from deequ_amd import ingest

    rng = np.random.default_rng(21)
    words = ENTRY_SET[:40]
    an = _analyzers()

    def values(n):
        return [None if rng.random() < 0.1 else words[int(i)] for i in rng.integers(0, len(words), n)]

    def check(batches, vals):
        cols = {"c": _ocol(vals)}
        for a, name, got in zip(an, ("Completeness", "ApproxCountDistinct", "DataType"),
                                _states_of(ingest.scan_arrow(batches, an), an)):
            _same(got, O.compute_state((name, "c", None), cols, len(vals)))

    for ity in (pa.int8(), pa.int16(), pa.int32()):  # index widths; two batches of different dictionaries
        v1, v2 = values(2049), values(65)
        bs = [pa.record_batch([pa.array(v).dictionary_encode().cast(pa.dictionary(ity, pa.string()))], names=["c"])
              for v in (v1, v2)]
        assert ingest.arrow_schema(bs[0])[0][1] == "dict_utf8"
        check(bs, v1 + v2)
    v = values(300)
    enc = pa.array(v).dictionary_encode()
    check([pa.record_batch([enc], names=["c"]).slice(3)], v[3:])  # a slice starting at row 3
    sliced = pa.DictionaryArray.from_arrays(pa.array([0, 2, None, 1, 2] * 13, type=pa.int16()),
                                            pa.array(["zero", "1", "2.5", None, "true"]).slice(1))
    check([pa.record_batch([sliced], names=["c"])], _decode([0, 2, None, 1, 2] * 13, ["1", "2.5", None, "true"]))
    # a run that reads the bytes (PatternMatch): the column is decoded on the device, per batch
    pm = [dq.PatternMatch("c", r"\d+"), dq.Completeness("c")]
    got = _states_of(ingest.scan_arrow([pa.record_batch([enc], names=["c"])], pm), pm)
    for g, spec in zip(got, [("PatternMatch", "c", r"\d+", None), ("Completeness", "c", None)]):
        _same(g, O.compute_state(spec, {"c": _ocol(v)}, len(v)))


def test_arrow_batches_sharing_a_dictionary_run_the_entry_pass_once():
    pa = pytest.importorskip("pyarrow")
    dq, L, runner, table, O = _mods()
    from deequ_amd import ingest

    d1 = pa.array(["a", "12", None, "x"])
    d2 = pa.array(["other", "3.5"])
    i1, i2, i3 = [0, 1, None, 2, 3] * 20, [3, 3, 1, None, 0] * 20, [1, 0, None] * 30
    batches = [pa.record_batch([pa.DictionaryArray.from_arrays(pa.array(i, type=pa.int8()), d)], names=["c"])
               for i, d in ((i1, d1), (i2, d1), (i3, d2))]
    an = _analyzers()
    plan = runner.ScanPlan(an, ingest.arrow_schema(batches[0]))
    sc = ingest.ArrowScanner(plan, 1 << 20)
    before = table.Dictionary.entries_calls
    try:
        sc.scan(batches[0])
        sc.scan(batches[1])
        assert (sc.dictionary_uploads, table.Dictionary.entries_calls - before) == (1, 1)  # shared: ran once
        sc.scan(batches[2])
        assert (sc.dictionary_uploads, table.Dictionary.entries_calls - before) == (2, 2)  # a new dictionary: again
        got = _states_of(plan.finish(), an)
    finally:
        sc.close()
        plan.close()
    vals = _decode(i1, d1.to_pylist()) + _decode(i2, d1.to_pylist()) + _decode(i3, d2.to_pylist())
    for a, name, g in zip(an, ("Completeness", "ApproxCountDistinct", "DataType"), got):
        _same(g, O.compute_state((name, "c", None), {"c": _ocol(vals)}, len(vals)))


def test_arrow_upload_rejects_an_index_outside_the_dictionary():
    """host-side rejection in dq_upload's copy loop: nothing reaches the device"""
    pa = pytest.importorskip("pyarrow")
    dq, L, runner, table, O = _mods()
    from deequ_amd import ingest

    bad = pa.DictionaryArray.from_arrays(pa.array([0, 1, 5, 1], type=pa.int8()), pa.array(["a", "b"]), safe=False)
    with pytest.raises(L.DQError) as e:
        ingest.scan_arrow([pa.record_batch([bad], names=["c"])], _analyzers())
    assert e.value.status == L.DQ_E_INVALID and "row 2" in str(e.value)
