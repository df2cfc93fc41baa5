"""ColumnProfiler.profile (deequ_amd/profiles.py) against the reference's ColumnProfilerTest.scala:51-203, transcribed
into tests/golden/profiler_kats.json, and the reference's typing rules (ColumnProfiler.scala:341-396, 492-516).
Tests that scan are marked gpu; the ones that only assemble profiles run anywhere.
"""
from __future__ import annotations

import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "profiler_kats.json")) as _f:
    KATS = json.load(_f)


@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import deequ_amd

    return deequ_amd


def _dataset(dq, name):
    ds = KATS["datasets"][name]
    return dq.Table.from_pydict({c: (ds["types"][c], v) for c, v in ds["columns"].items()})


def _distribution(spec):
    from deequ_amd.metrics import Distribution, DistributionValue

    return Distribution({k: DistributionValue(a, r) for k, (a, r) in spec["values"].items()}, spec["numberOfBins"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", KATS["cases"], ids=[c["name"] for c in KATS["cases"]])
def test_reference_cases(dq, case):
    from deequ_amd.profiles import ColumnProfiler, NumericColumnProfile, StandardColumnProfile

    kwargs = {}
    if case["lowCardinalityHistogramThreshold"] is not None:
        kwargs["lowCardinalityHistogramThreshold"] = case["lowCardinalityHistogramThreshold"]
    profiles = ColumnProfiler.profile(_dataset(dq, case["dataset"]), case["restrictToColumns"], False, **kwargs)
    assert profiles.numRecords == 6
    actual = profiles.profiles[case["column"]]
    want = case["expected"]
    if case["kind"] == "histogram_only":  # ColumnProfilerTest.scala:191-202
        assert actual.histogram is not None
        for key, (absolute, ratio) in want["histogram"]["values"].items():
            assert actual.histogram[key].absolute == absolute
            assert actual.histogram[key].ratio == ratio
        return
    histogram = None if want["histogram"] is None else _distribution(want["histogram"])
    if case["kind"] == "standard":  # case-class equality (:73, :173)
        assert actual == StandardColumnProfile(case["column"], want["completeness"], want["approximateNumDistinctValues"],
                                               want["dataType"], want["isDataTypeInferred"], want["typeCounts"], histogram)
        return
    # assertProfilesEqual (:30-47); the percentiles are not compared there
    assert isinstance(actual, NumericColumnProfile)
    assert actual.column == case["column"]
    assert actual.completeness == want["completeness"]
    assert abs(actual.approximateNumDistinctValues - want["approximateNumDistinctValues"]) <= 1
    assert actual.dataType == want["dataType"]
    assert actual.isDataTypeInferred == want["isDataTypeInferred"]
    assert actual.typeCounts == want["typeCounts"]
    assert actual.histogram == histogram
    for field in ("mean", "maximum", "minimum", "sum", "stdDev"):
        assert getattr(actual, field) == want[field], field
    # this project's own percentile check (as tests/test_cast_gpu.py): exact order statistics of the six values
    assert len(actual.approxPercentiles) == 100 and actual.approxPercentiles == sorted(actual.approxPercentiles)
    assert set(actual.approxPercentiles) <= {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}
    assert actual.approxPercentiles[0] == 1.0 and actual.approxPercentiles[-1] == 6.0


# every column type of the table layer -> (knownTypes entry, profile class); strings are inferred instead
KNOWN = {"i16": "Integral", "i32": "Integral", "i64": "Integral", "f32": "Fractional", "f64": "Fractional",
         "decimal(10,2)": "Fractional", "bool": "Boolean", "timestamp": "String", "i8": "Unknown", "date32": "Unknown"}


def test_known_type_mapping():
    from deequ_amd.profiles import known_type
    from deequ_amd.table import FIXED

    assert set(FIXED) <= set(KNOWN), "a fixed-width column type without a knownTypes expectation"
    for dtype, want in KNOWN.items():
        assert known_type(dtype) == want, dtype


@pytest.mark.gpu
def test_profile_of_every_column_type(dq):
    from deequ_amd.profiles import ColumnProfiler, NumericColumnProfile, StandardColumnProfile

    n = 6
    data = {"i16": ("i16", [1, 2, 3, 4, 5, None]), "i32": ("i32", [1, 2, 3, 4, 5, 6]), "i64": ("i64", [1, 2, 3, 4, 5, 6]),
            "f32": ("f32", [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), "f64": ("f64", [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]),
            "decimal(10,2)": ("decimal(10,2)", ["1.00", "2.00", "3.00", "4.00", "5.00", "6.00"]),
            "bool": ("bool", [True, False, None, True, True, False]),
            "timestamp": ("timestamp", [0, 1_000_000, 0, 0, None, 5]),
            "i8": ("i8", [1, 2, 3, 1, 2, 3]), "date32": ("date32", [1, 1, 1, 2, 2, None]),
            "utf8": ("utf8", ["a", "b", None, "a", "a", "c"]), "large_utf8": ("large_utf8", ["x", "x", "y", None, "x", "x"]),
            "boolish": ("utf8", ["true", "false", "true", None, "true", "false"]),
            "intish": ("utf8", ["1", "2", "3", "4", "5", "6"])}
    t = dq.Table.from_pydict(data)
    res = ColumnProfiler.profile(t)
    assert res.numRecords == n and list(res.profiles) == list(data)
    for name, want in KNOWN.items():
        p = res.profiles[name]
        assert p.dataType == want and p.isDataTypeInferred is False and p.typeCounts == {}, name
        if want in ("Integral", "Fractional"):
            assert isinstance(p, NumericColumnProfile), name
            assert p.histogram is None
        else:
            assert isinstance(p, StandardColumnProfile), name  # Byte and Date: Unknown, no second-pass metrics
    for name in ("i32", "i64", "f32", "f64", "decimal(10,2)"):
        p = res.profiles[name]
        assert (p.mean, p.minimum, p.maximum, p.sum) == (3.5, 1.0, 6.0, 21.0), name
    assert res.profiles["i16"].sum == 15.0 and res.profiles["i16"].completeness == 5 / 6
    for name in ("i32", "i64", "f64"):  # the column types ApproxQuantiles takes
        assert len(res.profiles[name].approxPercentiles) == 100
    # Timestamp is typed String, but only string and boolean columns get histograms (:498-511)
    assert res.profiles["timestamp"].histogram is None
    assert res.profiles["i8"].histogram is None and res.profiles["date32"].histogram is None
    b = res.profiles["bool"].histogram
    assert {k: v.absolute for k, v in b.values.items()} == {"true": 3, "false": 2, "NullValue": 1} and b.numberOfBins == 3
    assert {k: v.absolute for k, v in res.profiles["utf8"].histogram.values.items()} == {"a": 3, "b": 1, "c": 1, "NullValue": 1}
    assert {k: v.absolute for k, v in res.profiles["large_utf8"].histogram.values.items()} == {"x": 4, "y": 1, "NullValue": 1}
    # a string column inferred Boolean gets a histogram; one inferred Integral numeric statistics and no histogram
    p = res.profiles["boolish"]
    assert p.dataType == "Boolean" and p.isDataTypeInferred and isinstance(p, StandardColumnProfile)
    assert {k: v.absolute for k, v in p.histogram.values.items()} == {"true": 3, "false": 2, "NullValue": 1}
    assert p.histogram["true"].ratio == 0.5
    p = res.profiles["intish"]
    assert p.dataType == "Integral" and p.isDataTypeInferred and isinstance(p, NumericColumnProfile)
    assert p.histogram is None and (p.mean, p.sum, p.stdDev) == (3.5, 21.0, 1.707825127659933)


@pytest.mark.gpu
def test_profile_over_chunks_equals_one_table(dq):
    from deequ_amd.profiles import ColumnProfiler

    vals = {"s": ("utf8", ["a", None, "b", "a", "NullValue", "", "a", None]), "b": ("bool", [True, None, False] * 2 + [True, True]),
            "n": ("utf8", ["1.5", "2", None, "4", "5", "6", "7", "8"])}
    whole = ColumnProfiler.profile(dq.Table.from_pydict(vals))
    chunks = [dq.Table.from_pydict({k: (t, v[a:b]) for k, (t, v) in vals.items()}) for a, b in ((0, 3), (3, 3), (3, 8))]
    parts = ColumnProfiler.profile(chunks)
    for name in vals:
        assert parts.profiles[name].histogram == whole.profiles[name].histogram, name
        assert parts.profiles[name].dataType == whole.profiles[name].dataType
    assert whole.profiles["s"].histogram.numberOfBins == 4  # "NullValue" joins the NULLs: a, b, "", NullValue
    assert whole.profiles["s"].histogram["NullValue"].absolute == 3
    assert whole.profiles["n"].dataType == "Fractional" and whole.profiles["n"].histogram is None


@pytest.mark.gpu
def test_missing_column_and_repository_arguments(dq):
    from deequ_amd.profiles import ColumnProfiler

    t = _dataset(dq, "complete_and_incomplete")
    with pytest.raises(ValueError, match="Unable to find column nope"):
        ColumnProfiler.profile(t, ["att1", "nope"])
    with pytest.raises(NotImplementedError):
        ColumnProfiler.profile(t, metricsRepository=object())


def test_create_profiles_assembly():
    """createProfiles (:617-670) from hand-made statistics: no scan."""
    from deequ_amd.metrics import Distribution, DistributionValue
    from deequ_amd.profiles import (GenericColumnStatistics, NumericColumnProfile, NumericColumnStatistics,
                                    StandardColumnProfile, _distribution, create_profiles,
                                    find_target_columns_for_histograms)

    generic = GenericColumnStatistics(4, {"s": "String", "n": "Integral"}, {"k": "Fractional", "d": "Unknown"},
                                      {"s": {"String": 4}, "n": {"Integral": 4}}, {"s": 2, "n": 4, "k": 4, "d": 130},
                                      {"s": 0.5, "n": 1.0, "k": 1.0, "d": 1.0})
    assert generic.typeOf("s") == "String" and generic.typeOf("k") == "Fractional"
    numeric = NumericColumnStatistics({"n": 2.5}, {"n": 1.0}, {"n": 1.0}, {"n": 4.0}, {"n": 10.0}, {})
    hist = _distribution({"a": 1, "NullValue": 1}, 2)
    assert hist == Distribution({"a": DistributionValue(1, 0.25), "NullValue": DistributionValue(3, 0.75)}, 2)
    res = create_profiles(["s", "n", "k", "d"], generic, numeric, {"s": hist})
    assert res.numRecords == 4
    assert res.profiles["s"] == StandardColumnProfile("s", 0.5, 2, "String", True, {"String": 4}, hist)
    assert res.profiles["n"] == NumericColumnProfile("n", 1.0, 4, "Integral", True, {"Integral": 4}, None, 2.5, 4.0, 1.0,
                                                     10.0, 1.0, None)
    assert res.profiles["k"] == NumericColumnProfile("k", 1.0, 4, "Fractional", False, {}, None, *[None] * 6)
    assert res.profiles["d"] == StandardColumnProfile("d", 1.0, 130, "Unknown", False, {}, None)
    schema = [("s", "utf8", True), ("n", "utf8", True), ("k", "f64", True), ("d", "date32", True)]
    assert find_target_columns_for_histograms(schema, generic, 120) == ["s"]
    assert find_target_columns_for_histograms(schema, generic, 1) == []
