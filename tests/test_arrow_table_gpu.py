"""Arrow tables and record batches as data for every runner (GPU): Table.from_arrow / ingest.tables_from_arrow build
Columns byte-identical to Table.from_pydict's, dictionaries are shared across batches, every runner gives for Arrow data
what it gives for the same Tables, and ingest.scan_arrow builds derived length / expression columns per batch."""
import datetime
import decimal

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
pytestmark = pytest.mark.gpu

ROWS = (0, 1, 63, 64, 65, 1000)
EPOCH = datetime.date(1970, 1, 1)


def _values(dtype, n, rng):
    """(python values for pyarrow, the same values as from_pydict takes them) without NULLs."""
    if dtype in ("f64", "f32"):
        v = rng.normal(size=n).astype(np.float64 if dtype == "f64" else np.float32).tolist()
        return v, v
    if dtype in ("i64", "i32", "i16", "i8"):
        hi = {"i64": 2 ** 62, "i32": 2 ** 31 - 1, "i16": 2 ** 15 - 1, "i8": 127}[dtype]
        v = [int(x) for x in rng.integers(-hi, hi, n)]
        return v, v
    if dtype == "bool":
        v = [bool(x) for x in rng.integers(0, 2, n)]
        return v, v
    if dtype == "date32":
        d = [int(x) for x in rng.integers(-20000, 20000, n)]
        return [EPOCH + datetime.timedelta(days=x) for x in d], d
    if dtype == "timestamp":
        v = [int(x) for x in rng.integers(-2 ** 50, 2 ** 50, n)]
        return v, v
    if dtype.startswith("decimal"):
        u = [int(x) * 10 ** 11 + int(y) for x, y in zip(rng.integers(-10 ** 8, 10 ** 8, n), rng.integers(0, 10 ** 11, n))]
        return [decimal.Decimal(x).scaleb(-2) for x in u], [decimal.Decimal(x).scaleb(-2) for x in u]
    words = ["", "a", "bb", "żółć", "x" * 33, "data quality"]
    v = [words[k] for k in rng.integers(0, len(words), n)]
    return v, v


ARROW_TYPE = {"f64": pa.float64(), "f32": pa.float32(), "i64": pa.int64(), "i32": pa.int32(), "i16": pa.int16(),
              "i8": pa.int8(), "bool": pa.bool_(), "date32": pa.date32(), "timestamp": pa.timestamp("us"),
              "utf8": pa.string(), "large_utf8": pa.large_string(), "decimal(20,2)": pa.decimal128(20, 2),
              "dict_utf8": pa.dictionary(pa.int16(), pa.string())}


def _host(col):
    """Every buffer of a Column copied back, with the fields the layout contract names."""
    buf = lambda t: None if t is None else t.cpu().numpy().tobytes()  # noqa: E731
    out = {"dtype": col.dtype, "n_rows": col.n_rows, "nullable": col.nullable, "null_count": col.null_count,
           "data_bytes": col.data_bytes, "values": buf(col.values), "validity": buf(col.validity),
           "offsets": buf(col.offsets)}
    if col.dictionary is not None:
        out["dictionary"] = _host(col.dictionary.entries)
    return out


def _same_tables(a, b):
    assert list(a.columns) == list(b.columns) and a.num_rows == b.num_rows
    for name in a.columns:
        assert _host(a.columns[name]) == _host(b.columns[name]), name


def _pair(dtype, n, seed, null_frac, offset=0):
    """(pyarrow array of n rows -- a slice at `offset` of a longer one --, the from_pydict column spec)."""
    rng = np.random.default_rng(seed)
    pav, pyv = _values(dtype, offset + n, rng)
    valid = rng.random(offset + n) >= null_frac
    if dtype == "dict_utf8":
        entries = sorted(set(pav)) + [None, "unused"]
        idx = [entries.index(v) if ok else None for v, ok in zip(pav, valid)]
        arr = pa.DictionaryArray.from_arrays(pa.array(idx, type=pa.int16()), pa.array(entries, type=pa.string()))
        spec = ("dict_utf8", (idx[offset:], entries))
    else:
        arr = pa.array([v if ok else None for v, ok in zip(pav, valid)], type=ARROW_TYPE[dtype])
        spec = (dtype, [v if ok else None for v, ok in zip(pyv[offset:], valid[offset:])])
    return arr.slice(offset), spec


@pytest.mark.parametrize("dtype", list(ARROW_TYPE))
def test_from_arrow_is_byte_identical_to_from_pydict(dtype):
    import deequ_amd as dq
    from deequ_amd import ingest

    for n in ROWS:
        # plain and sliced at 1, 8, 13 (bitmaps at every bit offset, string offsets not starting at 0)
        for offset in (0, 1, 8, 13):
            arr, spec = _pair(dtype, n, 100 * n + offset, 0.2, offset)
            _same_tables(dq.Table.from_arrow(pa.record_batch([arr], names=["c"])), dq.Table.from_pydict({"c": spec}))
        # all-NULL
        arr, spec = _pair(dtype, n, n, 1.1)
        _same_tables(dq.Table.from_arrow(pa.record_batch([arr], names=["c"])), dq.Table.from_pydict({"c": spec}))
        # a nullable field without a validity buffer (all rows valid), and a non-nullable field
        arr, spec = _pair(dtype, n, n + 7, -1.0)
        assert arr.buffers()[0] is None or arr.null_count == 0
        _same_tables(dq.Table.from_arrow(pa.record_batch([arr], names=["c"])), dq.Table.from_pydict({"c": spec}))
        schema = pa.schema([pa.field("c", arr.type, nullable=False)])
        got = dq.Table.from_arrow(pa.record_batch([arr], schema=schema))
        _same_tables(got, dq.Table.from_pydict({"c": spec}, nullable={"c": False}))
        assert got.columns["c"].validity is None and not got.columns["c"].nullable
        # a 3-chunk pyarrow.Table: one Table from from_arrow, three from tables_from_arrow
        # (no empty chunk here: whether to_batches() keeps one is pyarrow's business; zero rows are covered above)
        sizes = (n + 1, n // 2 + 1, n + 2)
        parts = [_pair(dtype, k, 31 * n + k, 0.2) for k in sizes]
        if dtype == "dict_utf8":  # (chunks of one column share one dictionary here)
            arr, spec = _pair(dtype, sum(sizes), 5 * n, 0.2)
            cuts = [(0, sizes[0]), (sizes[0], sizes[1]), (sizes[0] + sizes[1], sizes[2])]
            parts = [(arr.slice(a, k), ("dict_utf8", (spec[1][0][a:a + k], spec[1][1]))) for a, k in cuts]
        tab = pa.Table.from_batches([pa.record_batch([p[0]], names=["c"]) for p in parts])
        chunks = ingest.tables_from_arrow(tab)
        assert len(chunks) == 3
        for t, (_, spec) in zip(chunks, parts):
            _same_tables(t, dq.Table.from_pydict({"c": spec}))
        if dtype == "dict_utf8":
            whole = ("dict_utf8", (sum((p[1][1][0] for p in parts), []), parts[0][1][1][1]))
        else:
            whole = (dtype, sum((p[1][1] for p in parts), []))
        _same_tables(dq.Table.from_arrow(tab), dq.Table.from_pydict({"c": whole}))


def test_bytes_under_null_slots_are_dropped():
    import deequ_amd as dq

    full = pa.array(["abc", "secret", "", "zz"])
    valid = np.packbits([True, False, True, True], bitorder="little").tobytes()
    arr = pa.Array.from_buffers(pa.string(), 4, [pa.py_buffer(valid), full.buffers()[1], full.buffers()[2]])
    ints = pa.Array.from_buffers(pa.int32(), 4, [pa.py_buffer(valid), pa.py_buffer(np.array([1, 77, 3, 4], np.int32))])
    got = dq.Table.from_arrow(pa.record_batch([arr, ints], names=["s", "i"]))
    _same_tables(got, dq.Table.from_pydict({"s": ("utf8", ["abc", None, "", "zz"]), "i": ("i32", [1, None, 3, 4])}))


def test_refusals_on_the_device_path():
    import deequ_amd as dq

    raw = b"".join(int(u).to_bytes(16, "little", signed=True) for u in (5, 10 ** 20, -3))
    bad = pa.Array.from_buffers(pa.decimal128(20, 2), 3, [None, pa.py_buffer(raw)])
    with pytest.raises(ValueError, match=r"column 'amount'.*row 1 "):
        dq.Table.from_arrow(pa.record_batch([pa.array([1, 2, 3]), bad], names=["k", "amount"]))
    idx = pa.DictionaryArray.from_arrays(pa.array([0, 1, 5, None], type=pa.int8()), pa.array(["a", "b"]), safe=False)
    with pytest.raises(ValueError, match=r"column 'd'.*index 5 at row 2 "):
        dq.Table.from_arrow(pa.record_batch([idx], names=["d"]))


def test_batches_share_one_dictionary():
    import deequ_amd as dq
    from deequ_amd import ingest
    from deequ_amd.table import Dictionary

    rng = np.random.default_rng(5)
    entries = pa.array([f"value {k}" for k in range(40)] + [None])
    idx = [None if x == 41 else int(x) for x in rng.integers(0, 42, 900)]
    whole = pa.DictionaryArray.from_arrays(pa.array(idx, type=pa.int32()), entries)
    batches = [pa.record_batch([whole.slice(300 * k, 300)], names=["d"]) for k in range(3)]
    other = pa.record_batch([pa.array(["x", "y", None, "x"]).dictionary_encode()], names=["d"])
    b = ingest.ArrowTableBuilder()
    calls = Dictionary.entries_calls
    tables = ingest.tables_from_arrow(batches, builder=b)
    assert b.dictionary_uploads == 1
    assert len({id(t.columns["d"].dictionary) for t in tables}) == 1
    plain = [dq.Table.from_pydict({"d": ("utf8", whole.slice(300 * k, 300).to_pylist())}) for k in range(3)]
    an = [dq.Uniqueness(["d"]), dq.Histogram("d"), dq.ApproxCountDistinct("d")]
    got = dq.AnalysisRunner.onData(tables).addAnalyzers(an).run()
    want = dq.AnalysisRunner.onData(plain).addAnalyzers(an).run()
    assert got.successMetricsAsJson() == want.successMetricsAsJson() and len(got.allMetrics) == 3
    assert Dictionary.entries_calls - calls <= 1  # one dq_dict_entries pass for the three batches
    tables += ingest.tables_from_arrow(other, builder=b)
    assert b.dictionary_uploads == 2 and tables[3].columns["d"].dictionary is not tables[0].columns["d"].dictionary
    b.close()


# ------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def mixed():
    """(pyarrow.Table of 3 batches, the from_pydict chunk list) of ~2,000 mixed rows with ~10% NULLs."""
    import deequ_amd as dq

    sizes, names = (700, 650, 651), ["x", "l", "i", "b", "d", "t", "m", "s", "c"]
    dtypes = ["f64", "i64", "i32", "bool", "date32", "timestamp", "decimal(20,2)", "utf8", "dict_utf8"]
    whole = {n: _pair(dt, sum(sizes), 11 + k, 0.1) for k, (n, dt) in enumerate(zip(names, dtypes))}
    rng = np.random.default_rng(1)
    small = [None if x == 9 else int(x) for x in rng.integers(0, 10, sum(sizes))]
    whole["i"] = (pa.array(small, type=pa.int32()), ("i32", small))
    batches, chunks, at = [], [], 0
    for k in sizes:
        batches.append(pa.record_batch([whole[n][0].slice(at, k) for n in names], names=names))
        spec = {}
        for n in names:
            dt, vals = whole[n][1]
            spec[n] = (dt, (vals[0][at:at + k], vals[1]) if dt == "dict_utf8" else vals[at:at + k])
        chunks.append(dq.Table.from_pydict(spec))
        at += k
    return pa.Table.from_batches(batches), chunks


def _shapes(tab):
    return {"table": lambda: tab, "batches": lambda: tab.to_batches(),
            "reader": lambda: pa.RecordBatchReader.from_batches(tab.schema, tab.to_batches())}


def _check():
    import deequ_amd as dq

    return (dq.Check(dq.CheckLevel.Error, "families")
            .isComplete("x")
            .satisfies("l * 2 + i > 0", "arith", lambda v: v >= 0.0)
            .hasCompleteness("l", lambda v: v > 0.5)
            .hasPattern("s", r"^[a-z ]+$", lambda v: v >= 0.0)
            .isUnique("l")
            .hasNumberOfDistinctValues("i", lambda v: v <= 11)
            .hasEntropy("i", lambda v: v > 0.0)
            .hasApproxQuantile("x", 0.5, lambda v: abs(v) < 1.0)
            .hasMinLength("s", lambda v: v == 0.0)
            .hasCorrelation("x", "l", lambda v: abs(v) <= 1.0)
            .hasDataType("s", dq.ConstrainableDataTypes.String))


@pytest.mark.parametrize("shape", ["table", "batches", "reader"])
def test_verification_suite_on_arrow_equals_tables(mixed, shape):
    import deequ_amd as dq

    tab, chunks = mixed
    extra = [dq.Compliance("where", "x > 0", "i % 2 = 0"), dq.MaxLength("c")]
    want = dq.VerificationSuite().onData(chunks).addCheck(_check()).addRequiredAnalyzers(extra).run()
    got = dq.VerificationSuite().onData(_shapes(tab)[shape]()).addCheck(_check()).addRequiredAnalyzers(extra).run()
    assert got.status == want.status
    assert [(str(c.constraint), c.status, c.message) for r in got.checkResults.values() for c in r.constraintResults] == \
        [(str(c.constraint), c.status, c.message) for r in want.checkResults.values() for c in r.constraintResults]
    assert {str(a): str(m.value) for a, m in got.metrics.items()} == {str(a): str(m.value) for a, m in want.metrics.items()}
    assert dq.AnalyzerContext(got.metrics).successMetricsAsJson() == dq.AnalyzerContext(want.metrics).successMetricsAsJson()
    assert len(got.metrics) >= 12
    # the row-level results of the run, for every name
    rows_got, rows_want = got.rowLevelResults(_shapes(tab)[shape]()), want.rowLevelResults(chunks)
    names = list(rows_want.constraints) + list(rows_want.checks)
    assert list(rows_got.constraints) + list(rows_got.checks) == names and names
    for name in names:
        assert np.array_equal(rows_got.as_bool(name), rows_want.as_bool(name)), name


@pytest.mark.parametrize("shape", ["table", "batches", "reader"])
def test_profiler_and_suggestions_on_arrow_equal_tables(mixed, shape):
    import deequ_amd as dq
    from deequ_amd.suggestions import Rules

    tab, chunks = mixed
    want = dq.ColumnProfilerRunner().onData(chunks).run()
    got = dq.ColumnProfilerRunner().onData(_shapes(tab)[shape]()).run()
    assert got.numRecords == want.numRecords and list(got.profiles) == list(want.profiles)
    for name in want.profiles:
        assert repr(vars(got.profiles[name])) == repr(vars(want.profiles[name])), name
    sw = dq.ConstraintSuggestionRunner().onData(chunks).addConstraintRules(Rules.DEFAULT).run()
    sg = dq.ConstraintSuggestionRunner().onData(_shapes(tab)[shape]()).addConstraintRules(Rules.DEFAULT).run()
    flat = lambda r: [(c, s.description, s.codeForConstraint) for c, ss in r.constraintSuggestions.items() for s in ss]  # noqa: E731
    assert flat(sg) == flat(sw) and flat(sw)


def test_schema_validator_on_an_all_string_arrow_table():
    import deequ_amd as dq

    rng = np.random.default_rng(9)
    ids = [None if k % 17 == 0 else (str(k) if k % 5 else "x" + str(k)) for k in range(600)]
    names = [None if x < 0.1 else "n" * int(1 + 20 * x) for x in rng.random(600)]
    tab = pa.table({"id": pa.array(ids), "name": pa.array(names)})
    schema = dq.RowLevelSchema().withIntColumn("id", isNullable=False).withStringColumn("name", maxLength=12)
    want = dq.RowLevelSchemaValidator.validate(dq.Table.from_pydict({"id": ("utf8", ids), "name": ("utf8", names)}), schema)
    got = dq.RowLevelSchemaValidator.validate(tab.to_batches()[0], schema)
    assert (got.numValidRows, got.numInvalidRows) == (want.numValidRows, want.numInvalidRows)
    assert 0 < got.numInvalidRows < 600
    _same_tables(got.validRows, want.validRows)
    _same_tables(got.invalidRows, want.invalidRows)


def test_incremental_states_across_arrow_and_tables(mixed):
    import deequ_amd as dq
    from deequ_amd.state_provider import InMemoryStateProvider

    tab, chunks = mixed
    an = [dq.Size(), dq.Mean("x"), dq.Completeness("s"), dq.ApproxCountDistinct("l"), dq.Uniqueness(["i"]),
          dq.MinLength("s"), dq.Compliance("arith", "l * 2 + i > 0")]
    single = dq.AnalysisRunner.onData(chunks).addAnalyzers(an).run().successMetricsAsJson()
    batches = tab.to_batches()
    for first, second in ((batches[:1], chunks[1:]), (chunks[:1], batches[1:])):
        states = InMemoryStateProvider()
        dq.AnalysisRunner.onData(first).addAnalyzers(an).saveStatesWith(states).run()
        merged = dq.AnalysisRunner.onData(second).addAnalyzers(an).aggregateWith(states).run()
        assert merged.successMetricsAsJson() == single
    # runOnAggregatedStates takes the data for its schema
    states = InMemoryStateProvider()
    dq.AnalysisRunner.onData(tab).addAnalyzers(an).saveStatesWith(states).run()
    import json

    rows = lambda text: sorted(json.loads(text), key=str)  # noqa: E731  (it lists the metrics in the analyzers' order)
    assert rows(dq.AnalysisRunner.runOnAggregatedStates(tab, an, [states]).successMetricsAsJson()) == rows(single)


# ------------------------------------------------------------------------------------------ scan_arrow
def _scan_batches():
    import deequ_amd as dq

    rng = np.random.default_rng(21)
    sizes = (500, 333, 167)
    n = sum(sizes)
    cols = {"a": _pair("i64", n, 1, 0.1), "b": _pair("i32", n, 2, 0.1), "c": _pair("f64", n, 3, 0.1),
            "s": _pair("utf8", n, 4, 0.1), "d": _pair("dict_utf8", n, 5, 0.1)}
    small = [None if x == 0 else int(x) for x in rng.integers(0, 50, n)]
    cols["a"] = (pa.array(small, type=pa.int64()), ("i64", small))
    batches, chunks, at = [], [], 0
    for k in sizes:
        batches.append(pa.record_batch([cols[c][0].slice(at, k) for c in cols], names=list(cols)))
        spec = {}
        for c, (_, (dt, vals)) in cols.items():
            spec[c] = (dt, (vals[0][at:at + k], vals[1]) if dt == "dict_utf8" else vals[at:at + k])
        chunks.append(dq.Table.from_pydict(spec))
        at += k
    return batches, chunks


def _state_bytes(states):
    import ctypes

    return [ctypes.string_at(ctypes.addressof(s), ctypes.sizeof(s)) for s in states]


def test_scan_arrow_builds_derived_columns_per_batch():
    import deequ_amd as dq
    from deequ_amd import expressions
    from deequ_amd.ingest import scan_arrow
    from deequ_amd.runner import scan_results

    batches, chunks = _scan_batches()
    an = [dq.MinLength("s"), dq.MaxLength("s"), dq.MinLength("d"), dq.MaxLength("d"),
          dq.Compliance("p", "a * b + c > 0"), dq.Mean("b", where="a % 2 = 0")]
    want = scan_results(chunks, an)
    calls = expressions.eval_calls
    got = scan_arrow(batches, an)
    assert expressions.eval_calls - calls == 2 * 3
    assert _state_bytes(got) == _state_bytes(want)
    assert all(s.has_value[0] for s in got)


def test_scan_arrow_plans_without_derived_columns_are_unchanged():
    import deequ_amd as dq
    from deequ_amd import expressions
    from deequ_amd.ingest import scan_arrow
    from deequ_amd.runner import scan_results

    batches, chunks = _scan_batches()
    an = [dq.Size(), dq.Completeness("c"), dq.Mean("c"), dq.StandardDeviation("c"), dq.Minimum("a"), dq.Maximum("a"),
          dq.Sum("b"), dq.ApproxCountDistinct("s"), dq.ApproxCountDistinct("a"), dq.Correlation("c", "b"),
          dq.Compliance("k", "c > 3 AND a IS NOT NULL"), dq.Completeness("s"), dq.Mean("b", "c > 0")]
    calls = expressions.eval_calls
    got = scan_arrow(batches, an)
    assert expressions.eval_calls == calls
    assert _state_bytes(got) == _state_bytes(scan_results(chunks, an))
