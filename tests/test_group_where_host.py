"""`where` on the grouping, histogram and quantile analyzers: everything that needs no device -- identity and printing,
the repository JSON, the filterable checks, the failure metrics of a refused predicate and a missing column (both
raised before any launch: the tables here live on the CPU), and the argument checks of the _where entry points."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import pytest

import deequ_amd as dq
from deequ_amd import _lib as L
from deequ_amd.binning import Bins
from deequ_amd.repository import deserialize_analyzer, serialize_analyzer

W = "x > 1"
BINS = Bins.edges([0.0, 1.0, 2.0])

# (unfiltered analyzer, its str() and repository JSON on the parent commit, the filtered analyzer, its str())
CASES = [
    (lambda w: dq.Uniqueness(["a", "b"], w), "Uniqueness(List(a, b))",
     '{"analyzerName": "Uniqueness", "columns": ["a", "b"]}', "Uniqueness(List(a, b),Some(x > 1))"),
    (lambda w: dq.Distinctness(["a"], w), "Distinctness(List(a))",
     '{"analyzerName": "Distinctness", "columns": ["a"]}', "Distinctness(List(a),Some(x > 1))"),
    (lambda w: dq.CountDistinct("a", w), "CountDistinct(List(a))",
     '{"analyzerName": "CountDistinct", "columns": ["a"]}', "CountDistinct(List(a),Some(x > 1))"),
    (lambda w: dq.UniqueValueRatio(["a"], w), "UniqueValueRatio(List(a))",
     '{"analyzerName": "UniqueValueRatio", "columns": ["a"]}', "UniqueValueRatio(List(a),Some(x > 1))"),
    (lambda w: dq.Entropy("a", w), "Entropy(a)", '{"analyzerName": "Entropy", "column": "a"}', "Entropy(a,Some(x > 1))"),
    (lambda w: dq.MutualInformation("a", "b", w), "MutualInformation(List(a, b))",
     '{"analyzerName": "MutualInformation", "columns": ["a", "b"]}', "MutualInformation(List(a, b),Some(x > 1))"),
    (lambda w: dq.Histogram("a", where=w), "Histogram(a,None,1000)",
     '{"analyzerName": "Histogram", "column": "a", "maxDetailBins": 1000}', "Histogram(a,None,1000,Some(x > 1))"),
    (lambda w: dq.Histogram("a", None, 7, BINS, where=w), f"Histogram(a,None,7,{BINS})",
     '{"analyzerName": "Histogram", "column": "a", "maxDetailBins": 7, "binning": {"edges": [0.0, 1.0, 2.0], '
     '"labels": null}}', f"Histogram(a,None,7,{BINS},Some(x > 1))"),
    (lambda w: dq.ApproxQuantile("a", 0.5, 0.01, w), "ApproxQuantile(a,0.5,0.01)",
     '{"analyzerName": "ApproxQuantile", "column": "a", "quantile": 0.5, "relativeError": 0.01}',
     "ApproxQuantile(a,0.5,0.01,Some(x > 1))"),
    (lambda w: dq.ApproxQuantiles("a", [0.25, 0.75], 0.0, w), "ApproxQuantiles(a,List(0.25, 0.75),0.0)",
     '{"analyzerName": "ApproxQuantiles", "column": "a", "quantiles": "0.25,0.75", "relativeError": 0.0}',
     "ApproxQuantiles(a,List(0.25, 0.75),0.0,Some(x > 1))"),
]


@pytest.mark.parametrize("make,plain_str,plain_json,filtered_str", CASES, ids=[c[1] for c in CASES])
def test_identity_printing_and_repository_json(make, plain_str, plain_json, filtered_str):
    plain, filtered, other = make(None), make(W), make("x > 2")
    assert plain.where is None and filtered.where == W
    assert str(plain) == repr(plain) == plain_str  # today's analyzer, unchanged
    assert json.dumps(serialize_analyzer(plain)) == plain_json  # no new key without a filter
    assert str(filtered) == filtered_str
    assert plain == make(None) and hash(plain) == hash(make(None))
    assert filtered == make(W) and hash(filtered) == hash(make(W))
    assert len({plain, filtered, other, make(W)}) == 3  # two filters: two analyzers, neither the unfiltered one
    node = serialize_analyzer(filtered)
    assert node["where"] == W and {k: v for k, v in node.items() if k != "where"} == json.loads(plain_json)
    back = deserialize_analyzer(json.loads(json.dumps(node)))
    assert back == filtered and str(back) == filtered_str
    assert deserialize_analyzer(json.loads(plain_json)) == plain  # a result stored before filters loads as before
    # the persisted state's name derives from str(): two filters, two files
    from deequ_amd.state_provider import identifier

    assert len({identifier(plain), identifier(filtered), identifier(other)}) == 3


def test_where_is_the_last_parameter():
    assert dq.Uniqueness(["a"], W).where == dq.Uniqueness(["a"], where=W).where == W
    assert dq.Entropy("a", W).where == W and dq.MutualInformation("a", "b", W).where == W
    assert dq.ApproxQuantile("a", 0.5, 0.01, W).where == W and dq.ApproxQuantiles("a", [0.5], 0.01, W).where == W
    with pytest.raises(TypeError):  # keyword-only on Histogram, next to binning
        dq.Histogram("a", None, 1000, None, W)


def test_repository_round_trip_with_a_filter():
    from deequ_amd.metrics import DoubleMetric, Entity, Success
    from deequ_amd.repository import AnalysisResult, AnalysisResultSerde, ResultKey
    from deequ_amd.runner import AnalyzerContext

    a, b = dq.Uniqueness(["id"], "status != 'cancelled'"), dq.Uniqueness(["id"])
    ctx = AnalyzerContext({a: DoubleMetric(Entity.Column, "Uniqueness", "id", Success(1.0)),
                           b: DoubleMetric(Entity.Column, "Uniqueness", "id", Success(0.5))})
    text = AnalysisResultSerde.serialize([AnalysisResult(ResultKey(1), ctx)])
    assert text.count('"where"') == 1
    back = AnalysisResultSerde.deserialize(text)[0].analyzerContext
    assert back.metric(a).value.get() == 1.0 and back.metric(b).value.get() == 0.5


def test_the_ten_check_methods_are_filterable_and_where_replaces_the_last_constraint():
    from deequ_amd.checks import CheckWithLastConstraintFilterable

    base = dq.Check(dq.CheckLevel.Error, "c").isComplete("a")
    ok = lambda v: True  # noqa: E731
    made = [base.isUnique("a"), base.isPrimaryKey("a", "b"), base.hasUniqueness(["a"], ok), base.hasDistinctness(["a"], ok),
            base.hasUniqueValueRatio(["a"], ok), base.hasNumberOfDistinctValues("a", ok), base.hasHistogramValues("a", ok),
            base.hasEntropy("a", ok), base.hasMutualInformation("a", "b", ok), base.hasApproxQuantile("a", 0.5, ok)]
    for c in made:
        assert isinstance(c, CheckWithLastConstraintFilterable)
        assert len(c.constraints) == 2 and c.constraints[-1].inner.analyzer.where is None
        f = c.where(W)
        assert len(f.constraints) == 2 and str(f.constraints[0]) == str(base.constraints[0])
        assert f.constraints[-1].inner.analyzer.where == W
        assert type(f.constraints[-1].inner.analyzer) is type(c.constraints[-1].inner.analyzer)
    assert str(base.isUnique("a").constraints[-1]) == "UniquenessConstraint(Uniqueness(List(a)))"
    assert str(base.isUnique("a").where(W).constraints[-1]) == "UniquenessConstraint(Uniqueness(List(a),Some(x > 1)))"
    # UniqueValueRatio's constraint name keeps its open parenthesis
    assert str(base.hasUniqueValueRatio(["a"], ok).where(W).constraints[-1]) == \
        "UniqueValueRatioConstraint(UniqueValueRatio(List(a),Some(x > 1))"


def _cpu_table():
    from deequ_amd.table import Table, column_from_numpy

    return Table([column_from_numpy("a", "i64", np.arange(5), device="cpu"),
                  column_from_numpy("b", "i32", np.ones(5, np.int32), device="cpu")])


def _filtered(w):
    return [dq.Uniqueness(["a"], w), dq.Entropy("a", w), dq.Histogram("a", where=w), dq.Histogram("a", binning=BINS, where=w),
            dq.ApproxQuantile("a", 0.5, where=w), dq.ApproxQuantiles("a", [0.5], where=w),
            dq.MutualInformation("a", "b", where=w)]


def test_refused_predicate_and_missing_column_fail_before_any_launch():
    from deequ_amd import grouping
    from deequ_amd.metrics import UnsupportedOnGpuPathException

    t = _cpu_table()  # no device buffer anywhere: a launch over it could not succeed
    before = grouping.selection_builds
    for w in ("upper(a) = 'X'", "a LIKE '%x'"):
        scan = dq.Compliance("c", "a > 0", w).calculate(t).value.failed
        for a in _filtered(w):
            for m in (a.calculate(t), dq.AnalysisRunner.doAnalysisRun(t, [a]).metric(a)):
                e = m.value.failed
                assert isinstance(e, UnsupportedOnGpuPathException)
                assert str(e) == str(scan).replace(str(dq.Compliance("c", "a > 0", w)), str(a))
    w = "nope = 1"
    scan = dq.Compliance("c", "a > 0", w).calculate(t).value.failed
    for a in _filtered(w):
        for m in (a.calculate(t), dq.AnalysisRunner.doAnalysisRun(t, [a]).metric(a)):
            e = m.value.failed
            assert type(e) is type(scan) and str(e) == str(scan)
    assert grouping.selection_builds == before


def test_argument_checks_of_the_where_entry_points():
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    types = (i32 * 1)(L.TYPE_I64)
    views = (L.ColumnView * 1)()
    rows = (i64 * 1)(0)
    odd = (vp * 1)(4)  # not 8-byte aligned
    h = vp()
    assert L.lib.dq_freq_build_where(types, 1, views, rows, odd, 1, 0, None, ctypes.byref(h)) == L.DQ_E_INVALID
    assert b"8-byte aligned" in L.lib.dq_last_error()
    assert L.lib.dq_freq_build_where(types, 1, views, rows, None, -1, 0, None, ctypes.byref(h)) == L.DQ_E_INVALID
    rows[0] = -1
    assert L.lib.dq_freq_build_where(types, 1, views, rows, None, 1, 0, None, ctypes.byref(h)) == L.DQ_E_INVALID
    rows[0] = 0
    value, defined = ctypes.c_double(), i32()
    types2 = (i32 * 2)(L.TYPE_I64, L.TYPE_I64)
    views2 = (L.ColumnView * 2)()
    assert L.lib.dq_mutual_information_where(types2, views2, rows, odd, 1, 0, 0, None, ctypes.byref(value),
                                             ctypes.byref(defined)) == L.DQ_E_INVALID
    assert L.lib.dq_dict_count_where(views, 0, 4, None, 0, None) == L.DQ_E_INVALID
    assert L.lib.dq_dict_count_where(views, -1, None, None, 0, None) == L.DQ_E_INVALID
    assert L.lib.dq_bin_count_where(None, L.TYPE_F64, views, 0, 4, None, None, 0, None) == L.DQ_E_INVALID
    assert L.lib.dq_bin_count_where(None, L.TYPE_F64, views, 0, None, None, 4, 0, None) == L.DQ_E_INVALID
    q = (ctypes.c_double * 1)(0.5)
    out, cnt, ns = (ctypes.c_double * 1)(), i64(), i64()
    assert L.lib.dq_approx_quantiles_where(L.TYPE_I64, views, rows, odd, 1, q, 1, 0.0, 0, None, out,
                                           ctypes.byref(cnt)) == L.DQ_E_INVALID
    assert b"8-byte aligned" in L.lib.dq_last_error()
    assert L.lib.dq_quantile_digest_where(L.TYPE_I64, views, rows, odd, 1, 0.0, 0, None, None, None, 0, ctypes.byref(ns),
                                          ctypes.byref(cnt)) == L.DQ_E_INVALID
    assert b"8-byte aligned" in L.lib.dq_last_error()
    rows[0] = -1
    assert L.lib.dq_approx_quantiles_where(L.TYPE_I64, views, rows, None, 1, q, 1, 0.0, 0, None, out,
                                           ctypes.byref(cnt)) == L.DQ_E_INVALID
    assert L.lib.dq_freq_unique_rows_where(None, None, views, 0, None, None, None, None, None, None) == L.DQ_E_INVALID
