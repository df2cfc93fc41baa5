"""Segmented metrics without a device: the CPU reference (tests/segment_ref.py) against hand-written cases, the
vectorised chunk merge and finish against hand-computed states, and the API's refusals that need no launch."""
import math

import numpy as np
import pytest

import deequ_amd as dq
from deequ_amd import segments
from deequ_amd.grouping import Uniqueness
from tests import segment_ref as R

SCHEMA = [("country", "utf8", True), ("code", "dict_utf8", True), ("n", "i32", True), ("amount", "f64", True),
          ("price", "decimal(10,2)", True), ("ts", "timestamp", True), ("flag", "bool", True)]


# ---- the reference ---------------------------------------------------------------------------------------------------

def test_split_by_tuple_with_a_null_segment():
    parts = R.split([("a", 1), ("b", 1), ("a", 1), ("a", None), (None, 2), ("a", 2)])
    assert parts == {("a", 1): [0, 2], ("b", 1): [1], None: [3, 4], ("a", 2): [5]}
    assert R.split(["x", None, "x"]) == {("x",): [0, 2], None: [1]}


def test_reference_counts_and_ratios():
    assert R.metric("Size", 3) == ("ok", 3.0)
    assert R.metric("Size", 3, where=[True, False, None]) == ("ok", 1.0)
    assert R.metric("Size", 2, where=[False, False]) == ("ok", 0.0)       # FALSE is not NULL: sum(0, 0) = 0
    assert R.metric("Size", 2, where=[None, None]) == ("empty",)          # sum over NULLs is NULL
    assert R.metric("Completeness", 4, values=[1, None, 3, None]) == ("ok", 0.5)
    assert R.metric("Completeness", 4, values=[1, None, 3, None], where=[True, True, False, None]) == ("ok", 0.5)
    kind, v = R.metric("Completeness", 2, values=[1, 2], where=[False, False])
    assert kind == "ok" and math.isnan(v)                                  # 0 / 0
    assert R.metric("Compliance", 4, pred=[True, False, None, True]) == ("ok", 0.5)
    assert R.metric("Compliance", 2, pred=[None, None]) == ("empty",)
    assert R.metric("Compliance", 3, pred=[True, True, False], where=[True, False, True]) == ("ok", 0.5)


def test_reference_sums_moments_and_extremes():
    assert R.metric("Sum", 3, values=[1.5, None, 2.5]) == ("ok", 4.0)
    assert R.metric("Sum", 2, values=[None, None]) == ("empty",)
    assert R.metric("Sum", 2, values=[2 ** 62, 2 ** 62], integral=True) == ("ok", float(-2 ** 63))  # wrapping int64
    assert R.metric("Mean", 4, values=[1.0, 2.0, 6.0, 100.0], where=[True, True, True, False]) == ("ok", 3.0)
    assert R.metric("StandardDeviation", 4, values=[2.0, 4.0, 4.0, 6.0]) == ("ok", math.sqrt(2.0))
    assert math.isnan(R.metric("StandardDeviation", 2, values=[1.0, math.inf])[1])
    assert math.isnan(R.metric("Sum", 2, values=[math.inf, -math.inf])[1])
    assert R.metric("Sum", 2, values=[math.inf, 1.0]) == ("ok", math.inf)
    mn = R.metric("Minimum", 4, values=[0.0, -0.0, math.nan, 3.0])[1]
    mx = R.metric("Maximum", 3, values=[-0.0, 0.0, -1.0])[1]
    assert mn == 0.0 and math.copysign(1.0, mn) < 0 and mx == 0.0 and math.copysign(1.0, mx) > 0
    assert math.isnan(R.metric("Maximum", 2, values=[1.0, math.nan])[1])   # NaN is the largest value
    assert R.metric("Minimum", 2, values=[1.0, math.nan]) == ("ok", 1.0)
    assert math.isnan(R.metric("Minimum", 1, values=[math.nan])[1])
    assert R.sum_bound([1.0, -3.0]) == 2 * 2.0 ** -53 * 4.0
    assert abs(R.spark_order_sd([2.0, 4.0, 4.0, 6.0]) - math.sqrt(2.0)) < 1e-15


# ---- the chunk merge and the finish ----------------------------------------------------------------------------------

def _state(xs):
    s = segments.empty_states(1)
    if xs:
        m = sum(xs) / len(xs)
        s["n"], s["mean"], s["m2"], s["sum"] = len(xs), m, sum((x - m) ** 2 for x in xs), sum(xs)
        s["count"] = s["applies"] = len(xs)
        s["fmin"], s["fmax"] = min(xs), max(xs)
    return s


def test_merge_states_is_the_chan_merge_and_empty_is_neutral():
    a, b, e = _state([1.0, 2.0, 3.0]), _state([10.0, 20.0]), _state([])
    both = _state([1.0, 2.0, 3.0, 10.0, 20.0])
    got = segments.merge_states(a, b)
    for f in ("n", "count", "applies", "fmin", "fmax", "sum"):
        assert got[f][0] == both[f][0], f
    assert abs(got["mean"][0] - both["mean"][0]) < 1e-14 and abs(got["m2"][0] - both["m2"][0]) < 1e-12
    for x, y in ((a, e), (e, a)):
        got = segments.merge_states(x, y)
        assert got.tobytes() == a.tobytes()
    assert segments.merge_states(e, e).tobytes() == e.tobytes()
    # vectorised: several segments at once, -0.0 below 0.0, int64 sums wrap
    p, q = segments.empty_states(2), segments.empty_states(2)
    p["fmin"], q["fmin"], p["fmax"], q["fmax"] = [0.0, -0.0], [-0.0, 0.0], [-0.0, 0.0], [0.0, -0.0]
    p["isum"], q["isum"] = [2 ** 62, 1], [2 ** 62, 2]
    got = segments.merge_states(p, q)
    assert list(np.signbit(got["fmin"])) == [True, True] and list(np.signbit(got["fmax"])) == [False, False]
    assert list(got["isum"]) == [-2 ** 63, 3]


# ---- refusals before any launch --------------------------------------------------------------------------------------

def test_unsupported_analyzers_and_types_are_named():
    for a in (dq.ApproxCountDistinct("n"), dq.Correlation("n", "amount"), dq.DataType("country"),
              dq.PatternMatch("country", "a+"), Uniqueness("n"), dq.ApproxQuantile("amount", 0.5), dq.MaxLength("country"),
              dq.Histogram("country")):
        e = segments.unsupported_reason(a, SCHEMA)
        assert isinstance(e, segments.UnsupportedInSegmentedRunException), a
        assert "is not supported in segmented runs" in str(e) and str(a) in str(e)
    for a in (dq.Mean("price"), dq.Sum("price", where="n > 0"), dq.Minimum("price"), dq.StandardDeviation("price")):
        e = segments.unsupported_reason(a, SCHEMA)
        assert isinstance(e, segments.UnsupportedInSegmentedRunException)
        assert "type decimal(10,2) of column price is not supported in segmented runs" in str(e)
    for a in (dq.Completeness("price"), dq.Completeness("code"), dq.Completeness("flag"), dq.Size(), dq.Mean("n"),
              dq.Compliance("c", "n + 1 > 3"), dq.Maximum("amount", where="n % 2 = 0")):
        assert segments.unsupported_reason(a, SCHEMA) is None, a
    e = segments.unsupported_reason(dq.Mean("nope"), SCHEMA)  # as in an ordinary run
    assert type(e).__name__ == "NoSuchColumnException" and "nope" in str(e)
    e = segments.unsupported_reason(dq.Mean("country"), SCHEMA)
    assert type(e).__name__ == "WrongColumnTypeException"


def _host_table():
    return dq.Table.from_pydict({"k": ("i32", [1, 2, 2, None]), "x": ("f64", [1.0, 2.0, 3.0, 4.0])}, device="cpu")


def test_unknown_segment_column_and_empty_column_list():
    t = _host_table()
    with pytest.raises(Exception, match="Input data does not include column nope!") as ei:
        dq.run_segmented(t, "nope", [dq.Size()])
    assert type(ei.value).__name__ == "NoSuchColumnException"
    with pytest.raises(ValueError, match="At least one column"):
        dq.AnalysisRunner.onData(t).segmentBy([]).addAnalyzer(dq.Size()).run()


def test_max_segments_is_refused_before_any_grouped_launch(monkeypatch):
    t = _host_table()
    before = (segments.order_calls, segments.scan_calls)
    monkeypatch.setattr(segments, "_key_set", lambda chunks, columns: (None, 12, True))
    check = dq.Check(dq.CheckLevel.Error, "c").isComplete("x")
    with pytest.raises(ValueError, match="13 segments of \\(k\\) found, more than maxSegments = 12"):
        dq.VerificationSuite().onData(t).segmentBy("k", maxSegments=12).addCheck(check).run()
    with pytest.raises(ValueError, match="13 segments"):
        dq.run_segmented(t, ["k"], [dq.Size()], maxSegments=5)
    assert (segments.order_calls, segments.scan_calls) == before


def test_builders_carry_their_analyzers_and_checks():
    t = _host_table()
    b = dq.AnalysisRunner.onData(t).addAnalyzer(dq.Size()).segmentBy(["k"]).addAnalyzers([dq.Mean("x")])
    assert isinstance(b, segments.SegmentedAnalysisRunBuilder) and b.analyzers == [dq.Size(), dq.Mean("x")]
    v = dq.VerificationSuite().onData(t).addRequiredAnalyzer(dq.Size()).segmentBy("k")
    assert isinstance(v, segments.SegmentedVerificationRunBuilder) and v.maxSegments == 10000 and v.required == [dq.Size()]
    assert segments.TILE % 64 == 0 and segments.MAX_SLOTS == 64
