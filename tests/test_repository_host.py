"""deequ_amd.repository on the host: the serde, the result views, the loader's filters and both repositories.

Fixtures: tests/golden/repository_kats.json (what the reference's repository tests pin).  No GPU: metrics are built by
hand, the repositories never look at data.
"""
import json
import math
import os
import struct
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "repository_kats.json")) as f:
    K = json.load(f)


@pytest.fixture(scope="module")
def R():
    from deequ_amd import repository

    return repository


@pytest.fixture(scope="module")
def dq():
    import deequ_amd

    return deequ_amd


def _context(R, metric_map):
    from deequ_amd.runner import AnalyzerContext

    return AnalyzerContext({R.deserialize_analyzer(a): R.deserialize_metric(m) for a, m in metric_map})


def _bits(x):
    return struct.pack("<d", x)


def _double(dq, value, analyzer=None):
    analyzer = analyzer or dq.Mean("x")
    return analyzer, dq.DoubleMetric(dq.Entity.Column, analyzer.name, analyzer.instance, _S(value))


def _S(v):
    from deequ_amd.metrics import Success

    return Success(v)


def every_analyzer(dq):
    """One instance of every analyzer of analyzers.py, grouping.py and quantiles.py, with and without a where."""
    D = dq
    return [D.Size(), D.Size("a > 1"), D.Completeness("c"), D.Completeness("c", "a > 1"),
            D.Compliance("rule", "a > 3"), D.Compliance("rule", "a > 3", "b < 2"),
            D.PatternMatch("c", r"\d+<a>&'='"), D.PatternMatch("c", D.Patterns.EMAIL, "a > 1"),
            D.Sum("c"), D.Sum("c", "w"), D.Mean("c"), D.Mean("c", "w"), D.Minimum("c"), D.Minimum("c", "w"),
            D.Maximum("c"), D.Maximum("c", "w"), D.StandardDeviation("c"), D.StandardDeviation("c", "w"),
            D.ApproxCountDistinct("c"), D.ApproxCountDistinct("c", "w"), D.DataType("c"), D.DataType("c", "w"),
            D.Correlation("a", "b"), D.Correlation("a", "b", "w"),
            D.CountDistinct(["a", "b"]), D.Distinctness(["a", "b"]), D.Distinctness("a"), D.Uniqueness("a"),
            D.Uniqueness(["a", "b"]), D.UniqueValueRatio(["a", "b"]), D.Entropy("a"), D.MutualInformation("a", "b"),
            D.Histogram("a"), D.Histogram("a", None, 5),
            D.ApproxQuantile("a", 0.5), D.ApproxQuantile("a", 0.25, 0.2),
            D.ApproxQuantiles("a", [0.25, 0.5, 0.75]), D.ApproxQuantiles("a", [0.1], 1e-4)]


def metric_for(dq, analyzer, i):
    D = dq
    if isinstance(analyzer, (D.Histogram, D.DataType)):
        values = {"some": D.DistributionValue(10, 0.5), "<other>": D.DistributionValue(0, 0.0),
                  "": D.DistributionValue(3, 1.0 / 3.0)}
        return D.HistogramMetric(analyzer.instance, _S(D.Distribution(values, 10)))
    if isinstance(analyzer, D.ApproxQuantiles):
        return D.KeyedDoubleMetric(D.Entity.Column, "ApproxQuantiles", analyzer.instance,
                                   _S({str(q): 10.0 * q + i for q in analyzer.quantiles}))
    return D.DoubleMetric(analyzer.entity, analyzer.name, analyzer.instance, _S(0.1 * i + 1.0 / 3.0))


# ------------------------------------------------------------------------------------------------------- the serde
def test_round_trip_every_analyzer_and_metric_kind(R, dq):
    from deequ_amd.runner import AnalyzerContext

    analyzers = every_analyzer(dq)
    assert len(set(analyzers)) == len(analyzers)
    context = AnalyzerContext({a: metric_for(dq, a, i) for i, a in enumerate(analyzers)})
    results = [R.AnalysisResult(R.ResultKey(1507975810, {"Region": "EU"}), context),
               R.AnalysisResult(R.ResultKey(-5, {}), AnalyzerContext.empty())]
    text = R.AnalysisResultSerde.serialize(results)
    back = R.AnalysisResultSerde.deserialize(text)
    assert back == results
    assert list(back[0].analyzerContext.metricMap) == analyzers                   # order kept
    for a in analyzers:
        assert type(back[0].analyzerContext.metricMap[a]) is type(context.metricMap[a])
    assert R.AnalysisResultSerde.serialize(back) == text
    json.loads(text)  # finite values only: plain JSON


def test_every_analyzer_class_is_covered(dq):
    """The serde covers every public analyzer class of analyzers.py, grouping.py and quantiles.py."""
    import inspect

    from deequ_amd import analyzers, grouping, quantiles
    from deequ_amd.analyzers import Analyzer

    public = {c for m in (analyzers, grouping, quantiles) for _, c in inspect.getmembers(m, inspect.isclass)
              if issubclass(c, Analyzer) and c.__module__ == m.__name__ and not c.__name__.startswith("_")
              and c not in (Analyzer, grouping.FrequencyBasedAnalyzer)}
    assert public == {type(a) for a in every_analyzer(dq)}


def test_layout_of_one_result(R, dq):
    """Gson's pretty printing of the serializers' trees: field order, a None where left out, doubles as Double.toString."""
    from deequ_amd.runner import AnalyzerContext

    a, m = _double(dq, 1e10, dq.Completeness("c"))
    text = R.AnalysisResultSerde.serialize([R.AnalysisResult(R.ResultKey(7, {"t": "v"}), AnalyzerContext({a: m}))])
    assert text == """[
  {
    "resultKey": {
      "dataSetDate": 7,
      "tags": {
        "t": "v"
      }
    },
    "analyzerContext": {
      "metricMap": [
        {
          "analyzer": {
            "analyzerName": "Completeness",
            "column": "c"
          },
          "metric": {
            "metricName": "DoubleMetric",
            "entity": "Column",
            "instance": "c",
            "name": "Completeness",
            "value": 1.0E10
          }
        }
      ]
    }
  }
]"""
    assert R.AnalysisResultSerde.serialize([]) == "[]"
    assert R._gson_string("a<b>&c='d'\né") == '"a\\u003cb\\u003e\\u0026c\\u003d\\u0027d\\u0027\\né"'


def test_golden_layout_loads_and_reserializes(R):
    golden = K["serde_layout"]["results"]
    results = R.AnalysisResultSerde.deserialize(json.dumps(golden))
    assert len(results) == 4 and results[0].resultKey == R.ResultKey(K["DATE_ONE"], {"Region": "EU"})
    assert len(results[0].analyzerContext.metricMap) == 20
    assert json.loads(R.AnalysisResultSerde.serialize(results)) == golden
    assert R.AnalysisResultSerde.deserialize(R.AnalysisResultSerde.serialize(results)) == results


def test_pattern_match_round_trip(R, dq):
    from deequ_amd.runner import AnalyzerContext

    c = K["pattern_match_round_trip"]
    analyzer = dq.PatternMatch(c["column"], dq.Patterns.EMAIL)
    metric = R.deserialize_metric(c["metric"])
    result = R.AnalysisResult(R.ResultKey(K["DATE_ONE"], {"Region": "EU"}), AnalyzerContext({analyzer: metric}))
    (cloned, cloned_metric), = R.AnalysisResultSerde.deserialize(
        R.AnalysisResultSerde.serialize([result]))[0].analyzerContext.metricMap.items()
    assert (cloned.column, cloned.pattern, cloned.where) == (analyzer.column, analyzer.pattern, None)
    assert cloned_metric == metric


def test_refused_analyzers_and_metrics(R, dq):
    from deequ_amd.metrics import Failure
    from deequ_amd.runner import AnalyzerContext

    failed = dq.DoubleMetric(dq.Entity.Column, "Completeness", "ColumnA", Failure(ValueError("Some")))
    mixed = AnalyzerContext({dq.Size(): _double(dq, 5.0)[1], dq.Completeness("ColumnA"): failed})
    with pytest.raises(ValueError) as e:
        R.AnalysisResultSerde.serialize([R.AnalysisResult(R.ResultKey(0), mixed)])
    assert str(e.value) == K["failed_metric_refused"]["message"]
    with pytest.raises(ValueError) as e:
        R.serialize_analyzer(dq.Histogram("a", binningUdf=lambda v: v))
    assert str(e.value) == "Unable to serialize Histogram with binningUdf!"

    class Other(dq.Mean):
        pass

    with pytest.raises(ValueError) as e:
        R.serialize_analyzer(Other("a"))
    assert str(e.value) == "Unable to serialize analyzer Other(a,None)."
    with pytest.raises(ValueError) as e:
        R.deserialize_analyzer({"analyzerName": "KLLSketch"})
    assert str(e.value) == "Unable to deserialize analyzer KLLSketch."
    with pytest.raises(ValueError) as e:
        R.deserialize_metric({"metricName": "Other"})
    assert str(e.value) == "Unable to deserialize analyzer Other."


DOUBLES = [0.1, 1.0 / 3.0, 5e-324, 1.7976931348623157e308, -0.0, 0.0, 123456789.12345679, 1e7, 9999999.999999998, 1e-3,
           9.999999999999998e-4, 2.0 ** 53 + 2, -6.02214076e23, 4.35, 0.30000000000000004, 100.0]


def test_doubles_round_trip_bit_for_bit(R, dq):
    from deequ_amd.runner import AnalyzerContext

    context = AnalyzerContext(dict(_double(dq, v, dq.Mean(f"c{i}")) for i, v in enumerate(DOUBLES)))
    text = R.AnalysisResultSerde.serialize([R.AnalysisResult(R.ResultKey(0), context)])
    back = R.AnalysisResultSerde.deserialize(text)[0].analyzerContext
    for i, v in enumerate(DOUBLES):
        assert _bits(back.metricMap[dq.Mean(f"c{i}")].value.get()) == _bits(v), v


def test_non_finite_values_round_trip(R, dq):
    from deequ_amd.runner import AnalyzerContext

    values = {"nan": float("nan"), "inf": float("inf"), "ninf": float("-inf")}
    context = AnalyzerContext(dict(_double(dq, v, dq.Mean(k)) for k, v in values.items()))
    context.metricMap[dq.Histogram("h")] = dq.HistogramMetric(
        "h", _S(dq.Distribution({"k": dq.DistributionValue(0, float("nan"))}, 1)))
    context.metricMap[dq.ApproxQuantiles("q", [0.5])] = dq.KeyedDoubleMetric(
        dq.Entity.Column, "ApproxQuantiles", "q", _S({"0.5": float("inf")}))
    text = R.AnalysisResultSerde.serialize([R.AnalysisResult(R.ResultKey(0), context)])
    assert '"value": NaN' in text and '"value": Infinity' in text and '"value": -Infinity' in text  # Gson's lenient writer
    back = R.AnalysisResultSerde.deserialize(text)[0].analyzerContext.metricMap
    assert math.isnan(back[dq.Mean("nan")].value.get())
    assert back[dq.Mean("inf")].value.get() == float("inf") and back[dq.Mean("ninf")].value.get() == float("-inf")
    assert math.isnan(back[dq.Histogram("h")].value.get()["k"].ratio)
    assert back[dq.ApproxQuantiles("q", [0.5])].value.get() == {"0.5": float("inf")}


# ------------------------------------------------------------------------------------------- the views of a result
@pytest.mark.parametrize("case", K["analysis_result_cases"], ids=lambda c: c["name"].replace(" ", "_"))
def test_success_metrics_of_a_result(R, case):
    from deequ_amd.runner import AnalyzerContext

    context = AnalyzerContext.empty() if case.get("empty_context") else _context(R, K["context_dfFull"]["metricMap"])
    result = R.AnalysisResult(R.ResultKey(K["DATE_ONE"], case["tags"]), context)
    for_analyzers = [R.deserialize_analyzer(a) for a in case["forAnalyzers"]]
    rows = R.AnalysisResult.getSuccessMetricsAsDataFrame(result, for_analyzers, case["withTags"])
    key = lambda row: sorted(row.items())
    assert sorted(rows, key=key) == sorted(case["rows"], key=key)                  # assertSameRows: as sets
    for row in rows:
        assert list(row)[:5] == ["entity", "instance", "name", "value", "dataset_date"]
    got = json.loads(R.AnalysisResult.getSuccessMetricsAsJson(result, for_analyzers, case["withTags"]))
    assert sorted(got, key=key) == sorted(json.loads(case["json"]), key=key)       # assertSameJson


def test_simple_result_serde(R):
    c = K["simple_result_serde"]
    result = R.AnalysisResult(R.ResultKey(c["dataSetDate"], c["tags"]), _context(R, c["context"]))
    text = R.AnalysisResult.getSuccessMetricsAsJson(result)
    assert R.SimpleResultSerde.deserialize(text) == R.SimpleResultSerde.deserialize(c["json"])
    assert '"value":0.5623351446188083' in text and '"value":4.0' in text


def test_histogram_and_keyed_metrics_are_flattened_in_the_views(R, dq):
    from deequ_amd.runner import AnalyzerContext

    context = AnalyzerContext({dq.Histogram("h"): metric_for(dq, dq.Histogram("h"), 0),
                               dq.ApproxQuantiles("q", [0.5]): metric_for(dq, dq.ApproxQuantiles("q", [0.5]), 0)})
    rows = R.AnalysisResult.getSuccessMetricsAsDataFrame(R.AnalysisResult(R.ResultKey(1), context))
    assert [r["name"] for r in rows] == ["Histogram.bins", "Histogram.abs.some", "Histogram.ratio.some",
                                         "Histogram.abs.<other>", "Histogram.ratio.<other>", "Histogram.abs.",
                                         "Histogram.ratio.", "name-0.5"]


# ------------------------------------------------------------------------------------------------ the repositories
DATE_ONE, DATE_TWO, DATE_THREE = 1507975810, 1508062210, 1508148610
EU, NA = {"Region": "EU"}, {"Region": "NA"}


def both(tmp_path, R):
    return [R.InMemoryMetricsRepository(), R.FileSystemMetricsRepository(str(tmp_path / "metrics.json"))]


def fill(R, dq, repo):
    from deequ_amd.runner import AnalyzerContext

    def context(scale):
        return AnalyzerContext({dq.Size(): dq.DoubleMetric(dq.Entity.Dataset, "Size", "*", _S(4.0 * scale)),
                                dq.Completeness("att1"): _double(dq, 1.0 / scale, dq.Completeness("att1"))[1],
                                dq.Histogram("att2"): metric_for(dq, dq.Histogram("att2"), 0)})
    repo.save(R.ResultKey(DATE_ONE, EU), context(1))
    repo.save(R.ResultKey(DATE_TWO, NA), context(2))
    repo.save(R.ResultKey(DATE_THREE, dict(EU, run="nightly")), context(3))
    return context


def dates(results):
    return sorted(r.resultKey.dataSetDate for r in results)


def test_repositories_behave_alike(tmp_path, R, dq):
    observed = []
    for repo in both(tmp_path, R):
        context = fill(R, dq, repo)
        assert isinstance(repo, R.MetricsRepository)
        assert repo.loadByKey(R.ResultKey(DATE_ONE, EU)).metricMap == context(1).metricMap
        assert repo.loadByKey(R.ResultKey(DATE_ONE, NA)) is None and repo.loadByKey(R.ResultKey(1, EU)) is None
        load = repo.load
        # after and before are inclusive on both sides
        assert dates(load().get()) == [DATE_ONE, DATE_TWO, DATE_THREE]
        assert dates(load().after(DATE_TWO).get()) == [DATE_TWO, DATE_THREE]
        assert dates(load().after(DATE_TWO + 1).get()) == [DATE_THREE]
        assert dates(load().before(DATE_TWO).get()) == [DATE_ONE, DATE_TWO]
        assert dates(load().before(DATE_TWO - 1).get()) == [DATE_ONE]
        assert dates(load().after(DATE_TWO).before(DATE_TWO).get()) == [DATE_TWO]
        assert load().after(DATE_THREE + 1).get() == []
        # tags: every given pair has to be among the result's tags
        assert dates(load().withTagValues(EU).get()) == [DATE_ONE, DATE_THREE]
        assert dates(load().withTagValues({"Region": "EU", "run": "nightly"}).get()) == [DATE_THREE]
        assert load().withTagValues({"Region": "XX"}).get() == [] and load().withTagValues({"other": "EU"}).get() == []
        assert dates(load().withTagValues({}).get()) == [DATE_ONE, DATE_TWO, DATE_THREE]
        # forAnalyzers keeps the results and narrows their metrics
        only = load().forAnalyzers([dq.Completeness("att1"), dq.Mean("nope")]).get()
        assert dates(only) == [DATE_ONE, DATE_TWO, DATE_THREE]
        assert all(list(r.analyzerContext.metricMap) == [dq.Completeness("att1")] for r in only)
        assert all(r.analyzerContext.metricMap == {} for r in load().forAnalyzers([]).get())
        combined = load().withTagValues(EU).after(DATE_TWO).forAnalyzers([dq.Size()]).get()
        assert [(r.resultKey, r.analyzerContext.metricMap[dq.Size()].value.get()) for r in combined] == [
            (R.ResultKey(DATE_THREE, dict(EU, run="nightly")), 12.0)]
        # the views over several results: every tag column, None where a result lacks the tag
        rows = load().forAnalyzers([dq.Size()]).getSuccessMetricsAsDataFrame()
        assert sorted((r["dataset_date"], r["value"], r["region"], r["run"]) for r in rows) == [
            (DATE_ONE, 4.0, "EU", None), (DATE_TWO, 8.0, "NA", None), (DATE_THREE, 12.0, "EU", "nightly")]
        as_json = json.loads(load().forAnalyzers([dq.Size()]).getSuccessMetricsAsJson())
        assert sorted((r["dataset_date"], r["value"], r["region"], r.get("run")) for r in as_json) == sorted(
            (r["dataset_date"], r["value"], r["region"], r["run"]) for r in rows)
        assert all(set(r) == {"entity", "instance", "name", "value", "dataset_date", "region", "run"} for r in as_json)
        assert [r["region"] for r in load().withTagValues(NA).getSuccessMetricsAsDataFrame(withTags=["Region"])] == ["NA"] * 9
        assert load().after(DATE_THREE + 1).getSuccessMetricsAsJson() == "[]"
        assert load().after(DATE_THREE + 1).getSuccessMetricsAsDataFrame() == []
        observed.append(sorted(R.AnalysisResultSerde.serialize([r]) for r in load().get()))
    assert observed[0] == observed[1]


def test_saving_under_an_existing_key_replaces_the_result(tmp_path, R, dq):
    from deequ_amd.runner import AnalyzerContext

    for repo in both(tmp_path, R):
        fill(R, dq, repo)
        key = R.ResultKey(DATE_TWO, NA)
        repo.save(key, AnalyzerContext(dict([_double(dq, 42.0, dq.Mean("sales"))])))
        assert list(repo.loadByKey(key).metricMap) == [dq.Mean("sales")]            # replaced, not merged
        assert repo.loadByKey(key).metricMap[dq.Mean("sales")].value.get() == 42.0
        assert dates(repo.load().get()) == [DATE_ONE, DATE_TWO, DATE_THREE]          # the others stay, no duplicate
        assert len(repo.loadByKey(R.ResultKey(DATE_ONE, EU)).metricMap) == 3


def test_a_failed_metric_is_not_stored(tmp_path, R, dq):
    from deequ_amd.metrics import Failure
    from deequ_amd.runner import AnalyzerContext

    for repo in both(tmp_path, R):
        failed = dq.Completeness("att1").toFailureMetric(ValueError("boom"))
        failed_histogram = dq.HistogramMetric("h", Failure(ValueError("boom")))
        context = AnalyzerContext({dq.Size(): _double(dq, 4.0, dq.Size())[1], dq.Completeness("att1"): failed,
                                   dq.Histogram("h"): failed_histogram})
        repo.save(R.ResultKey(1, EU), context)
        assert list(repo.loadByKey(R.ResultKey(1, EU)).metricMap) == [dq.Size()]
        repo.save(R.ResultKey(2, EU), AnalyzerContext({dq.Completeness("att1"): failed}))
        assert repo.loadByKey(R.ResultKey(2, EU)).metricMap == {}                   # the key exists, empty


def test_file_system_repository_file(tmp_path, R, dq):
    path = tmp_path / "sub" / "metrics.json"
    path.parent.mkdir()
    repo = R.FileSystemMetricsRepository(str(path))
    assert repo.load().get() == [] and repo.loadByKey(R.ResultKey(1)) is None and not path.exists()
    fill(R, dq, repo)
    assert sorted(os.listdir(path.parent)) == ["metrics.json"]                     # no temporary file stays
    whole = json.loads(path.read_text(encoding="utf-8"))
    assert [r["resultKey"]["dataSetDate"] for r in whole] == [DATE_ONE, DATE_TWO, DATE_THREE]   # one file, all results
    assert R.AnalysisResultSerde.deserialize(path.read_text(encoding="utf-8")) == R.FileSystemMetricsRepository(
        str(path)).load().get()
    # a file in the reference's layout, written by hand, loads
    other = tmp_path / "golden.json"
    other.write_text(json.dumps(K["serde_layout"]["results"]), encoding="utf-8")
    loaded = R.FileSystemMetricsRepository(str(other))
    assert len(loaded.load().get()) == 4
    assert len(loaded.loadByKey(R.ResultKey(K["DATE_ONE"], {"Region": "NA"})).metricMap) == 20


def test_in_memory_repository_is_thread_safe(R, dq):
    from deequ_amd.runner import AnalyzerContext

    repo = R.InMemoryMetricsRepository()
    errors = []

    def work(t):
        try:
            for i in range(200):
                repo.save(R.ResultKey(i, {"t": str(t)}), AnalyzerContext(dict([_double(dq, float(i))])))
                repo.load().withTagValues({"t": str(t)}).get()
        except Exception as e:  # e.g. a dict changing size under an iteration
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == [] and len(repo.load().get()) == 1600


def test_result_key(R):
    assert R.ResultKey(1, {"a": "b", "c": "d"}) == R.ResultKey(1, {"c": "d", "a": "b"})
    assert hash(R.ResultKey(1, {"a": "b", "c": "d"})) == hash(R.ResultKey(1, {"c": "d", "a": "b"}))
    assert R.ResultKey(1) != R.ResultKey(2) and R.ResultKey(1, {"a": "b"}) != R.ResultKey(1)


# ------------------------------------------------------------------- the wiring that needs no data (no scan is run)
def test_new_check_methods(dq):
    check = dq.Check(dq.CheckLevel.Error, "c")
    names = [str(c) for c in check.hasApproxQuantile("a", 0.5, lambda v: v > 0).containsCreditCardNumber("s")
             .containsEmail("s").containsURL("s").containsSocialSecurityNumber("s").constraints]
    assert names == ["ApproxQuantileConstraint(ApproxQuantile(a,0.5,0.01))", "containsCreditCardNumber(s)",
                     "containsEmail(s)", "containsURL(s)", "containsSocialSecurityNumber(s)"]
    required = check.containsEmail("s").where("a > 1").containsURL("s").requiredAnalyzers()
    assert required == [dq.PatternMatch("s", dq.Patterns.EMAIL, "a > 1"), dq.PatternMatch("s", dq.Patterns.URL)]


def test_anomaly_check_against_a_stored_history(R, dq):
    """Check.isNewestPointNonAnomalous evaluated on a hand-made context: filters, the default config, a missing history."""
    from deequ_amd.runner import AnalyzerContext

    repo = R.InMemoryMetricsRepository()
    for day in range(1, 11):
        for tags, value in ((EU, float(day)), (NA, 100.0 * day)):
            repo.save(R.ResultKey(day, tags), AnalyzerContext({dq.Size(): dq.DoubleMetric(
                dq.Entity.Dataset, "Size", "*", _S(value))}))
    strategy = dq.RateOfChangeStrategy(maxRateIncrease=2.0)

    def status(value, **config):
        builder = dq.VerificationSuite().onData(None).useRepository(repo)
        cfg = dq.AnomalyCheckConfig(dq.CheckLevel.Error, "growth", **config) if config else None
        check = builder.addAnomalyCheck(strategy, dq.Size(), cfg).checks[-1]
        context = AnalyzerContext({dq.Size(): dq.DoubleMetric(dq.Entity.Dataset, "Size", "*", _S(value))})
        return check, check.evaluate(context)

    check, result = status(11.0, withTagValues=EU)
    assert result.status == dq.CheckStatus.Success and str(check.constraints[0]) == "AnomalyConstraint(Size(None))"
    assert status(13.5, withTagValues=EU)[1].status == dq.CheckStatus.Error
    assert status(1001.0, withTagValues=NA)[1].status == dq.CheckStatus.Success
    # before is inclusive: with day 10 left out the newest stored point is 9.0 and 11.5 grows by more than 2
    assert status(11.5, withTagValues=EU, beforeDate=10)[1].status == dq.CheckStatus.Success
    assert status(11.5, withTagValues=EU, beforeDate=9)[1].status == dq.CheckStatus.Error
    assert status(11.5, withTagValues=EU, afterDate=10)[1].status == dq.CheckStatus.Success
    # the default: level Warning, the reference's description; both regions interleave by date, so the rate breaks
    check, result = status(11.0)
    assert (check.level, check.description) == (dq.CheckLevel.Warning, "Anomaly check for Size(None)")
    # no history: the assertion's require fails inside the constraint
    check, result = status(1.0, withTagValues={"Region": "XX"})
    assert result.status == dq.CheckStatus.Error
    assert result.constraintResults[0].message == ("Can't execute the assertion: requirement failed: There have to be "
                                                   "previous results in the MetricsRepository!!")
    with pytest.raises(ValueError, match="useRepository"):
        dq.VerificationSuite().onData(None).addAnomalyCheck(strategy, dq.Size())


def test_run_on_aggregated_states_saves(R, dq):
    from deequ_amd.state_provider import InMemoryStateProvider
    from deequ_amd.states import NumMatches

    states = InMemoryStateProvider()
    states.persist(dq.Size(), NumMatches(5))
    repo, key = R.InMemoryMetricsRepository(), R.ResultKey(3, EU)
    repo.save(key, dq.AnalyzerContext(dict([_double(dq, 2.5, dq.Mean("kept"))])))
    schema = [("a", "i64", True)]
    got = dq.AnalysisRunner.runOnAggregatedStates(schema, [dq.Size(), dq.Mean("missing")], [states],
                                                  metricsRepository=repo, saveOrAppendResultsWithKey=key)
    assert got.metric(dq.Size()).value.get() == 5.0 and got.metric(dq.Mean("missing")).value.isFailure
    stored = repo.loadByKey(key).metricMap
    assert set(stored) == {dq.Mean("kept"), dq.Size()} and stored[dq.Size()].value.get() == 5.0   # existing ++ new
