"""String lengths without a GPU: dq_utf8_length_host's rule against Python's len() and against the byte rule in numpy,
and the Python layer of MinLength / MaxLength that needs no device -- names, serde, preconditions, the runner's derived
column name, dictionary routing, lowering."""
import numpy as np
import pytest


def host_lengths(slots, valid=None):
    """dq_utf8_length_host over the bytes of every slot (NULL rows' included)."""
    from deequ_amd import _lib as L

    data = np.frombuffer(b"".join(slots) or b"\0", np.uint8)
    offs = np.zeros(len(slots) + 1, np.int64)
    offs[1:] = np.cumsum([len(b) for b in slots])
    bits = None if valid is None else np.packbits(np.asarray(valid, bool), bitorder="little")
    out = np.full(len(slots), -1, np.int32)
    assert L.lib.dq_utf8_length_host(data.ctypes.data, offs.ctypes.data, len(slots),
                                     None if bits is None else bits.ctypes.data, out.ctypes.data) == L.DQ_OK
    return out


def test_host_lengths_equal_len():
    values = ["", "a", "é", "߿", "日", "€", "😀", "𝄞", "aé日😀", "", "x" * 33, "日本語のテキスト", "é" * 17 + "z"]
    assert host_lengths([v.encode() for v in values]).tolist() == [len(v) for v in values]
    long = "日" * 100_000
    assert host_lengths([b"ab", long.encode(), b""]).tolist() == [2, 100_000, 0]
    assert host_lengths([]).tolist() == []


def test_host_null_rows_hold_bytes():
    values = ["abc", None, "日本", None, ""]
    slots = ["ignored 日本語".encode() if v is None else v.encode() for v in values]
    got = host_lengths(slots, [v is not None for v in values])
    assert got.tolist() == [3, 0, 2, 0, 0]
    assert host_lengths(slots).tolist() == [3, 11, 2, 11, 0]  # no bitmap: no NULL row


def test_host_ill_formed_bytes_follow_the_byte_rule():
    slots = [b"\x80", b"\xbf\x80\x80", b"\xe6\x97", b"a\xe6\x97", b"\xff", b"\xff\xfe\x80a", b"\xc0\x80", b"\xf0\x9f\x98"]
    rng = np.random.default_rng(1)
    slots += [bytes(rng.integers(0, 256, rng.integers(0, 40), dtype=np.uint8)) for _ in range(500)]
    data = np.frombuffer(b"".join(slots), np.uint8)
    counts = np.concatenate([[0], np.cumsum((data & 0xC0) != 0x80)])
    offs = np.concatenate([[0], np.cumsum([len(b) for b in slots])])
    got = host_lengths(slots)
    assert np.array_equal(got, counts[offs[1:]] - counts[offs[:-1]])
    assert got[:8].tolist() == [0, 0, 1, 2, 1, 3, 1, 1]


def test_names():
    import deequ_amd as dq

    a, b = dq.MinLength("col"), dq.MaxLength("col", "x > 3")
    assert str(a) == "MinLength(col,None)" and str(b) == "MaxLength(col,Some(x > 3))"
    assert (a.name, b.name, a.instance, a.entity) == ("MinLength", "MaxLength", "col", dq.Entity.Column)
    assert a == dq.MinLength("col") and a != dq.MinLength("col", "x > 3") and a != dq.Minimum("col")
    assert hash(a) == hash(dq.MinLength("col")) and a != dq.MaxLength("col")
    check = (dq.Check(dq.CheckLevel.Error, "d").hasMinLength("col", lambda v: v >= 1)
             .hasMaxLength("col", lambda v: v <= 9).where("x > 3"))
    assert [str(c) for c in check.constraints] == ["MinLengthConstraint(MinLength(col,None))",
                                                   "MaxLengthConstraint(MaxLength(col,Some(x > 3)))"]
    assert [type(x).__name__ for x in check.requiredAnalyzers()] == ["MinLength", "MaxLength"]
    # the failure metric of an empty state carries the analyzer's name, as Minimum's does
    m = a.computeMetricFrom(None)
    assert m.value.isFailure and type(m.value.failed).__name__ == "EmptyStateException"
    assert (m.name, m.instance) == ("MinLength", "col")
    assert str(m.value.failed) == str(dq.Minimum("col").computeMetricFrom(None).value.failed).replace("Minimum", "MinLength")


def test_state_identifier_derives_from_to_string():
    import deequ_amd as dq
    from deequ_amd.state_provider import identifier

    ids = {identifier(a) for a in (dq.MinLength("s"), dq.MaxLength("s"), dq.MinLength("s", "x > 3"), dq.Minimum("s"))}
    assert len(ids) == 4


@pytest.mark.parametrize("where", [None, "x > 3"])
def test_repository_json_round_trip(where):
    import deequ_amd as dq
    from deequ_amd import repository as R

    for cls, name in ((dq.MinLength, "MinLength"), (dq.MaxLength, "MaxLength")):
        a = cls("s", where)
        node = R.serialize_analyzer(a)
        assert node == {"analyzerName": name, "column": "s", "where": where}
        assert R.deserialize_analyzer(node) == a and type(R.deserialize_analyzer(node)) is cls
    context = dq.AnalyzerContext({dq.MinLength("s", where): dq.DoubleMetric(dq.Entity.Column, "MinLength", "s", R.Success(0.0)),
                                  dq.MaxLength("s", where): dq.DoubleMetric(dq.Entity.Column, "MaxLength", "s", R.Success(17.0))})
    key = dq.ResultKey(5, {"t": "v"})
    text = R.AnalysisResultSerde.serialize([R.AnalysisResult(key, context)])
    back, = R.AnalysisResultSerde.deserialize(text)
    assert back.resultKey == key and back.analyzerContext.metricMap == context.metricMap
    # reuseExistingResultsForKey recognises the stored analyzers: with everything stored, no data is touched
    repository = dq.InMemoryMetricsRepository()
    repository.save(key, context)
    reused = (dq.AnalysisRunner.onData(None).addAnalyzers(list(context.metricMap)).useRepository(repository)
              .reuseExistingResultsForKey(key, failIfResultsMissing=True).run())
    assert reused.metricMap == context.metricMap


def test_preconditions():
    import deequ_amd as dq
    from deequ_amd.analyzers import Preconditions
    from deequ_amd.metrics import NoSuchColumnException, WrongColumnTypeException

    schema = [("n", "i64", True), ("s", "utf8", True), ("l", "large_utf8", True), ("d", "dict_utf8", True),
              ("p", "decimal(10,2)", True)]
    for cls in (dq.MinLength, dq.MaxLength):
        e = Preconditions.findFirstFailing(schema, cls("n").preconditions())
        assert type(e) is WrongColumnTypeException
        assert str(e) == "Expected type of column n to be StringType, but found LongType instead!"
        e = Preconditions.findFirstFailing(schema, cls("p").preconditions())
        assert str(e) == "Expected type of column p to be StringType, but found DecimalType(10,2) instead!"
        e = Preconditions.findFirstFailing(schema, cls("missing").preconditions())
        assert type(e) is NoSuchColumnException and str(e) == "Input data does not include column missing!"
        for ok in ("s", "l", "d"):
            assert Preconditions.findFirstFailing(schema, cls(ok).preconditions()) is None


def test_derived_column_name_avoids_user_columns():
    from deequ_amd.lengths import length_column_name

    assert length_column_name("s", ["s", "x"]) == "length(s)"
    assert length_column_name("s", ["s", "length(s)"]) == "_length(s)"
    assert length_column_name("s", ["s", "length(s)", "_length(s)", "__length(s)"]) == "___length(s)"
    assert length_column_name("t", ["s", "length(s)"]) == "length(t)"


def test_length_columns_needed_once_per_source():
    import deequ_amd as dq
    from deequ_amd.lengths import attach_length_columns, length_columns_needed

    an = [dq.MinLength("s"), dq.Completeness("q"), dq.MaxLength("s", "x > 1"), dq.MaxLength("t"), dq.MinLength("s", "x < 0")]
    assert length_columns_needed(an) == ["s", "t"]
    marker = object()
    assert attach_length_columns(marker, [dq.Completeness("q"), dq.Minimum("x")]) is marker  # nothing to attach


def test_lowering_reads_the_derived_column():
    import deequ_amd as dq
    from deequ_amd import _lib as L
    from deequ_amd.analyzers import PlanBuilder
    from deequ_amd.metrics import NoSuchColumnException, UnsupportedOnGpuPathException
    from deequ_amd.runner import explain, gpu_eligible

    schema = [("s", "utf8", True), ("x", "i64", True), ("length(s)", "i32", True)]
    lengths = {"s": "length(s)"}
    b = PlanBuilder(schema, lengths)
    assert dq.MinLength("s")._lower(b)[:4] == (L.OP_MIN, 0, -1, -1)
    op, col, _, _, where = dq.MaxLength("s", "x > 3")._lower(b)
    assert (op, col) == (L.OP_MAX, 0) and where >= 0
    assert b.columns == ["length(s)", "x"]  # the string column itself is not a column of the plan
    with pytest.raises(UnsupportedOnGpuPathException):
        dq.MinLength("s")._lower(PlanBuilder(schema))
    with pytest.raises(NoSuchColumnException):
        dq.MinLength("nope")._lower(PlanBuilder(schema, lengths))
    assert gpu_eligible(dq.MinLength("s", "x > 3"), schema, lengths) is None
    assert gpu_eligible(dq.MinLength("s", "length(s) > 3"), schema, lengths) is not None  # no function calls in `where`
    text = explain([dq.MinLength("s"), dq.MaxLength("s"), dq.Maximum("x")], schema, length_columns=lengths)
    i32_stats = [k for k, v in L.VARIANT_NAMES.items() if v == "i32_stats"][0]
    assert f"column pass: variant {i32_stats}, 1 task(s)" in text  # one task of the ordinary i32 pass for both
    assert L.lib.dq_abi_version() == 6 and len(L.VARIANT_NAMES) == 32


def test_dictionary_column_is_not_decoded_for_lengths():
    import deequ_amd as dq
    from deequ_amd.runner import dictionary_columns_to_decode

    schema = [("s", "dict_utf8", True), ("t", "dict_utf8", True), ("x", "i64", True)]
    keep = [dq.MinLength("s"), dq.MaxLength("s", "x > 3"), dq.Completeness("s"), dq.ApproxCountDistinct("s")]
    assert dictionary_columns_to_decode(schema, keep) == set()
    assert dictionary_columns_to_decode(schema, keep + [dq.MaxLength("t", "s = 'a'")]) == {"s"}  # the `where` reads s
    assert dictionary_columns_to_decode(schema, keep + [dq.PatternMatch("s", "a+")]) == {"s"}


def test_string_lengths_rejects_other_columns():
    import deequ_amd as dq

    col = dq.Column("x", "i64", 0, None, None)
    with pytest.raises(TypeError):
        dq.string_lengths(col)


def test_satisfies_with_length_is_still_refused():
    import deequ_amd as dq
    from deequ_amd.runner import gpu_eligible

    assert gpu_eligible(dq.Compliance("short", "length(s) <= 20"), [("s", "utf8", True)]) is not None
