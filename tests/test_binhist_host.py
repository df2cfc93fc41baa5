"""Binned histograms, host side only: Bins (validation, equal_width, labels, hashing), what Histogram's `binning` does
to the analyzer's identity (str, equality, preconditions) and the repository's serde.  No device."""
import math
import struct

import pytest


def _bits(x):
    return struct.pack("<d", x)


def test_edges_validation_names_the_position():
    from deequ_amd import Bins

    for bad, where in [([0.0, float("nan")], "edges[1]"), ([float("-inf"), 0.0], "edges[0]"),
                       ([0.0, 1.0, float("inf")], "edges[2]"), ([0.0, 1.0, 1.0], "edges[2]"),
                       ([0.0, 2.0, 1.0, 3.0], "edges[2]"), ([1.0, -1.0], "edges[1]"), ([0.0, -0.0], "edges[1]"),
                       ([0.0, "x"], "edges[1]"), ([0, 10 ** 400], "edges[1]")]:
        with pytest.raises(ValueError) as e:
            Bins.edges(bad)
        assert where in str(e.value), (bad, str(e.value))


def test_bin_count_limits():
    from deequ_amd import Bins

    for none in ([], [1.0]):  # k = 0
        with pytest.raises(ValueError, match="at least 2 edges"):
            Bins.edges(none)
    assert Bins.edges(range(4097)).num_bins == 4096
    with pytest.raises(ValueError, match="4097 bins"):
        Bins.edges(range(4098))
    with pytest.raises(ValueError, match="4097 bins"):
        Bins.equal_width(0.0, 1.0, 4097)
    for n in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            Bins.equal_width(0.0, 1.0, n)


def test_labels_length_mismatch():
    from deequ_amd import Bins

    with pytest.raises(ValueError, match="1 labels for 2 bins"):
        Bins.edges([0, 1, 2], labels=["a"])
    with pytest.raises(ValueError, match="3 labels for 2 bins"):
        Bins.edges([0, 1, 2], labels=["a", "b", "c"])
    with pytest.raises(ValueError, match=r"labels\[1\]"):
        Bins.edges([0, 1, 2], labels=["a", 7])
    assert Bins.edges([0, 1, 2], labels=["a", "b"]).bin_labels == ("a", "b")


def test_equal_width_edges():
    from deequ_amd import Bins

    lo, hi, n = 0.3, 0.9, 3
    b = Bins.equal_width(lo, hi, n)
    width = (hi - lo) / n
    assert [_bits(e) for e in b.bin_edges[:-1]] == [_bits(lo + i * width) for i in range(n)]
    assert _bits(b.bin_edges[-1]) == _bits(hi)  # exactly hi, not lo + n * width
    assert lo + n * width != hi  # (the case distinguishes the two)
    assert b == Bins.edges(b.bin_edges)  # from there it is Bins.edges
    assert Bins.equal_width(-3, 5, 1).bin_edges == (-3.0, 5.0)
    assert Bins.equal_width(0, 4096, 4096).num_bins == 4096
    for lo, hi in [(1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0), (-1.7e308, 1.7e308)]:
        with pytest.raises(ValueError):
            Bins.equal_width(lo, hi, 4)


def test_default_labels():
    from deequ_amd import Bins

    assert Bins.edges([0, 1]).slot_labels() == ["< 0.0", "[0.0, 1.0]", "> 1.0", "NaN"]
    assert Bins.edges([1e-5, 0.001, 2.5, 10000, 1e7, 1.5e300]).slot_labels() == [
        "< 1.0E-5", "[1.0E-5, 0.001)", "[0.001, 2.5)", "[2.5, 10000.0)", "[10000.0, 1.0E7)", "[1.0E7, 1.5E300]",
        "> 1.5E300", "NaN"]
    assert Bins.edges([-1.25e-7, -0.0, 123456.789]).slot_labels() == [
        "< -1.25E-7", "[-1.25E-7, 0.0)", "[0.0, 123456.789]", "> 123456.789", "NaN"]
    # given labels replace the k bin labels; the three extra ones stay
    assert Bins.edges([0, 18, 65], labels=["minor", "adult"]).slot_labels() == ["< 0.0", "minor", "adult", "> 65.0", "NaN"]


def test_default_labels_match_the_reference_restatement():
    from binhist_ref import default_labels
    from deequ_amd import Bins

    for edges in ([0, 1], [1e-5, 0.001, 2.5, 1e7], [-9.3e18, -1.0, 0.1, 2.0 ** 53, 9.3e18], [5e-324, 1e-310, 1.0]):
        assert Bins.edges(edges).slot_labels() == default_labels(edges)


def test_immutable_hashable_equal():
    from deequ_amd import Bins

    a, b = Bins.edges([0, 1, 2]), Bins.edges((0.0, 1.0, 2.0))
    assert a == b and hash(a) == hash(b) and str(a) == str(b)
    assert a != Bins.edges([0, 1, 2.5]) and a != Bins.edges([0, 1, 2], labels=["[0.0, 1.0)", "[1.0, 2.0]"])
    assert Bins.edges([0, 1, 2], ["x", "y"]) == Bins.edges([0, 1, 2], ("x", "y"))
    assert Bins.edges([0, 1, 2], ["x", "y"]) != Bins.edges([0, 1, 2], ["y", "x"])
    assert Bins.edges([-0.0, 1]) == Bins.edges([0.0, 1]) and str(Bins.edges([-0.0, 1])) == str(Bins.edges([0.0, 1]))
    assert len({a, b, Bins.equal_width(0, 2, 2)}) == 1
    assert a != (0.0, 1.0, 2.0) and a != "x"
    with pytest.raises(AttributeError):
        a.bin_edges = (0.0, 5.0)
    with pytest.raises(AttributeError):
        a.extra = 1
    with pytest.raises(AttributeError):
        del a.bin_labels


def test_histogram_str_and_identity():
    import deequ_amd as dq
    from deequ_amd import Bins

    # without bins: byte for byte what it was
    assert str(dq.Histogram("x")) == "Histogram(x,None,1000)"
    assert str(dq.Histogram("x", None, 7)) == "Histogram(x,None,7)"
    assert str(dq.Histogram("x", lambda v: v)) == "Histogram(x,Some(udf),1000)"
    assert dq.Histogram("x")._fields() == ("x", None, 1000)
    assert dq.Histogram("x", binning=None) == dq.Histogram("x")
    b1, b2 = Bins.edges([0, 1]), Bins.edges([0, math.nextafter(1.0, 2.0)])
    h1, h2 = dq.Histogram("x", binning=b1), dq.Histogram("x", binning=b2)
    assert str(h1) == "Histogram(x,None,1000,Bins(edges=[0.0, 1.0],labels=None))"
    assert str(h2) == "Histogram(x,None,1000,Bins(edges=[0.0, 1.0000000000000002],labels=None))"
    assert str(h1) != str(h2) and h1 != h2 and h1 != dq.Histogram("x")
    assert h1 == dq.Histogram("x", binning=Bins.equal_width(0, 1, 1)) and hash(h1) == hash(dq.Histogram("x", binning=b1))
    assert b1 in h1._fields()
    labelled = dq.Histogram("x", binning=Bins.edges([0, 1], labels=['a "q" é']))
    assert str(labelled) == 'Histogram(x,None,1000,Bins(edges=[0.0, 1.0],labels=["a \\"q\\" \\u00e9"]))'
    assert str(labelled) != str(h1) and labelled != h1
    # the persisted state's name comes from str: two binnings, two states
    from deequ_amd.state_provider import identifier

    assert len({identifier(dq.Histogram("x")), identifier(h1), identifier(h2), identifier(labelled)}) == 4
    with pytest.raises(TypeError):
        dq.Histogram("x", binning=[0, 1])


def test_both_udf_and_binning_refused():
    import deequ_amd as dq
    from deequ_amd import Bins
    from deequ_amd.analyzers import Preconditions
    from deequ_amd.metrics import IllegalAnalyzerParameterException, WrongColumnTypeException

    schema = [("x", "f64", True), ("s", "utf8", True), ("b", "bool", True), ("d", "decimal(9,2)", True)]
    both = dq.Histogram("x", lambda v: v, binning=Bins.edges([0, 1]))
    err = Preconditions.findFirstFailing(schema, both.preconditions())
    assert isinstance(err, IllegalAnalyzerParameterException)
    from types import SimpleNamespace

    m = both.calculate([SimpleNamespace(schema=schema)])  # (a stand-in chunk: the preconditions fail before any data is touched)
    assert m.value.isFailure and isinstance(m.value.failed, IllegalAnalyzerParameterException)
    bins = Bins.edges([0, 1])
    assert Preconditions.findFirstFailing(schema, dq.Histogram("x", binning=bins).preconditions()) is None
    assert Preconditions.findFirstFailing(schema, dq.Histogram("d", binning=bins).preconditions()) is None
    for col in ("s", "b"):  # a non-numeric column: the reference's wrong-column-type failure
        err = Preconditions.findFirstFailing(schema, dq.Histogram(col, binning=bins).preconditions())
        assert isinstance(err, WrongColumnTypeException), col
    assert Preconditions.findFirstFailing(schema, dq.Histogram("s").preconditions()) is None


def test_serde_round_trip_bit_exact():
    import json

    import deequ_amd as dq
    from deequ_amd import Bins
    from deequ_amd.metrics import Distribution, DistributionValue, HistogramMetric, Success
    from deequ_amd.repository import AnalysisResult, AnalysisResultSerde, ResultKey, deserialize_analyzer, serialize_analyzer

    assert serialize_analyzer(dq.Histogram("x", None, 5)) == {"analyzerName": "Histogram", "column": "x", "maxDetailBins": 5}
    edges = [-1.7976931348623157e308, -1e22, -0.1 - 0.2, 5e-324, 1e-5, 0.1, 1 / 3, 1.0, 2.0 ** 53, 1e21, 1.7976931348623157e308]
    plain = dq.Histogram("x", None, 10, binning=Bins.edges(edges))
    labelled = dq.Histogram("y", binning=Bins.edges([0, 1, 2], labels=["<lo & 'x'>", "NullValue"]))
    node = serialize_analyzer(plain)
    assert node["binning"]["labels"] is None and node["binning"]["edges"] == edges
    assert serialize_analyzer(labelled)["binning"] == {"edges": [0.0, 1.0, 2.0], "labels": ["<lo & 'x'>", "NullValue"]}
    metric = HistogramMetric("x", Success(Distribution({"[0.0, 1.0]": DistributionValue(3, 0.75)}, 2)))
    results = [AnalysisResult(ResultKey(1, {"t": "v"}),
                              dq.AnalyzerContext({plain: metric, labelled: metric, dq.Histogram("x"): metric}))]
    text = AnalysisResultSerde.serialize(results)
    back = list(AnalysisResultSerde.deserialize(text)[0].analyzerContext.metricMap)
    assert back == [plain, labelled, dq.Histogram("x")]
    assert [_bits(e) for e in back[0].binning.bin_edges] == [_bits(e) for e in edges]
    assert back[1].binning.bin_labels == ("<lo & 'x'>", "NullValue")
    assert str(back[0]) == str(plain) and str(back[1]) == str(labelled)
    # without a binning the analyzer's JSON has no such member
    plain_nodes = [e["analyzer"] for e in json.loads(text)[0]["analyzerContext"]["metricMap"]]
    assert "binning" in plain_nodes[0] and "binning" not in plain_nodes[2]
    assert deserialize_analyzer({"analyzerName": "Histogram", "column": "x", "maxDetailBins": 5}) == dq.Histogram("x", None, 5)


def test_checks_pass_the_binning_through():
    import deequ_amd as dq
    from deequ_amd import Bins

    bins = Bins.edges([0, 1])
    check = (dq.Check(dq.CheckLevel.Error, "c").hasHistogramValues("x", lambda d: True, binning=bins)
             .hasNumberOfDistinctValues("x", lambda n: True, binning=bins)
             .hasHistogramValues("x", lambda d: True))
    analyzers = list(check.requiredAnalyzers())
    assert dq.Histogram("x", binning=bins) in analyzers and dq.Histogram("x") in analyzers


def test_profile_field_is_last_and_optional():
    import dataclasses

    from deequ_amd import NumericColumnProfile

    f = dataclasses.fields(NumericColumnProfile)[-1]
    assert f.name == "distribution" and f.default is None
