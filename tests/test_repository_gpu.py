"""The metrics repository and the anomaly checks driven by the GPU scan: the reference's
MetricsRepositoryAnomalyDetectionIntegrationTest over a device table, device metrics through a store and the JSON
round trip bit for bit, and which analyzers still reach a plan once stored results are reused.  Tables of 8 and 64 rows.
"""
import datetime
import struct

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd

    return deequ_amd


def create_date(year, month, day):  # LocalDate.of(..).atTime(0, 0, 0).toEpochSecond(ZoneOffset.UTC)
    return int(datetime.datetime(year, month, day, tzinfo=datetime.timezone.utc).timestamp())


def repositories(dq, tmp_path):
    return [dq.InMemoryMetricsRepository(), dq.FileSystemMetricsRepository(str(tmp_path / "repository-test.json"))]


# ---------------------------------------------------- MetricsRepositoryAnomalyDetectionIntegrationTest.scala:59-212
@pytest.fixture(scope="module")
def sales(dq):  # getTestData (:81-102)
    return dq.Table.from_pydict({
        "item": ("utf8", ["item1", "item1", "item1", "item2", "item2", "item3", "item4", "item5"]),
        "origin": ("utf8", ["US", "US", "US", "DE", "DE", None, None, None]),
        "sales": ("i32", [100, 1000, 20, 20, 333, 12, 45, 123]),
        "marketplace": ("utf8", ["EU"] * 8)}, nullable={"item": False, "origin": True, "sales": False,
                                                        "marketplace": False})


def fill_with_previous_results(dq, repository):  # fillRepositoryWithPreviousResults (:104-126), name and instance
    from deequ_amd.metrics import Success             # in the order the reference passes them

    for past_day in range(1, 31):
        eu = dq.AnalyzerContext({
            dq.Size(): dq.DoubleMetric(dq.Entity.Dataset, "*", "Size", Success(float(past_day // 3))),
            dq.Mean("sales"): dq.DoubleMetric(dq.Entity.Column, "sales", "Mean", Success(float(past_day * 7)))})
        na = dq.AnalyzerContext({
            dq.Size(): dq.DoubleMetric(dq.Entity.Dataset, "*", "Size", Success(float(past_day))),
            dq.Mean("sales"): dq.DoubleMetric(dq.Entity.Column, "sales", "Mean", Success(float(past_day * 9)))})
        date = create_date(2018, 7, past_day)
        repository.save(dq.ResultKey(date, {"marketplace": "EU"}), eu)
        repository.save(dq.ResultKey(date, {"marketplace": "NA"}), na)


def test_anomaly_detection_integration(dq, sales, tmp_path):
    for repository in repositories(dq, tmp_path):
        fill_with_previous_results(dq, repository)
        other = (dq.Check(dq.CheckLevel.Error, "check").isComplete("item").isComplete("origin")
                 .isContainedIn("marketplace", ["EU"]).isNonNegative("sales"))
        eu = {"marketplace": "EU"}
        after, before = create_date(2018, 1, 1), create_date(2018, 8, 1)
        size_config = dq.AnomalyCheckConfig(dq.CheckLevel.Error, "Size only increases", eu, after, before)
        mean_config = dq.AnomalyCheckConfig(dq.CheckLevel.Warning, "Sales mean within 2 standard deviations", eu,
                                            after, before)
        key = dq.ResultKey(create_date(2018, 8, 1), eu)
        result = (dq.VerificationSuite().onData(sales).addCheck(other)
                  .addRequiredAnalyzers([dq.Maximum("sales"), dq.Minimum("sales")])
                  .useRepository(repository)
                  .addAnomalyCheck(dq.RateOfChangeStrategy(0.0), dq.Size(), size_config)
                  .addAnomalyCheck(dq.OnlineNormalStrategy(upperDeviationFactor=2.0, ignoreAnomalies=False),
                                   dq.Mean("sales"), mean_config)
                  .saveOrAppendResult(key).run())
        by_description = {c.description: r for c, r in result.checkResults.items()}
        # the new size 8 is below the last stored value 10: an anomaly
        assert by_description["Size only increases"].status == dq.CheckStatus.Error
        # the new mean 206.625 is within 2 standard deviations of (1 to 30) * 7
        assert by_description["Sales mean within 2 standard deviations"].status == dq.CheckStatus.Success
        assert by_description["check"].status == dq.CheckStatus.Error          # origin has NULLs
        assert result.metrics[dq.Size()].value.get() == 8.0 and result.metrics[dq.Mean("sales")].value.get() == 206.625
        # the run is stored after the checks were evaluated, under its own key, failures left out
        stored = repository.loadByKey(key).metricMap
        assert stored == {a: m for a, m in result.metrics.items() if m.value.isSuccess}
        assert {dq.Size(), dq.Mean("sales"), dq.Maximum("sales"), dq.Minimum("sales")} <= set(stored)
        assert len(repository.load().withTagValues(eu).get()) == 31


# ------------------------------------------------------------------------ device metrics through the repository
N = 64


@pytest.fixture(scope="module")
def table(dq):
    x = [0.1 * i + 1.0 / 3.0 for i in range(N)]
    x[5] = None
    y = [(-1.0) ** i * 1e-3 * i * i + 7.7 for i in range(N)]
    return dq.Table.from_pydict({
        "x": ("f64", x), "y": ("f64", y), "k": ("i64", [i * 37 % 23 for i in range(N)]),
        "s": ("utf8", [None if i % 11 == 0 else "v%d" % (i % 7) for i in range(N)])})


def analyzers(dq):
    return [dq.Size(), dq.Mean("x"), dq.StandardDeviation("x"), dq.Mean("y"), dq.StandardDeviation("y"),
            dq.ApproxCountDistinct("k"), dq.ApproxCountDistinct("s"), dq.Histogram("s"), dq.ApproxQuantile("x", 0.5),
            dq.ApproxQuantiles("y", [0.25, 0.5, 0.75]), dq.Correlation("x", "y"), dq.Completeness("s"),
            dq.DataType("s"), dq.Entropy("s"), dq.Uniqueness(["k", "s"])]


def bits(v):
    return struct.pack("<d", v)


def assert_same_metric(got, want):
    assert type(got) is type(want) and (got.entity, got.name, got.instance) == (want.entity, want.name, want.instance)
    a, b = got.value.get(), want.value.get()
    if isinstance(b, float):
        assert bits(a) == bits(b)
    elif isinstance(b, dict):
        assert list(a) == list(b) and all(bits(a[k]) == bits(b[k]) for k in b)
    else:  # Distribution
        assert a.numberOfBins == b.numberOfBins and list(a.values) == list(b.values)
        for k, v in b.values.items():
            assert a.values[k].absolute == v.absolute and bits(a.values[k].ratio) == bits(v.ratio)


@pytest.fixture(scope="module")
def full_run(dq, table):
    """The run every test below compares against: computed once, left unchanged."""
    context = dq.AnalysisRunner.onData(table).addAnalyzers(analyzers(dq)).run()
    assert all(m.value.isSuccess for m in context.allMetrics), context.metricMap
    return context


def test_save_then_load_by_key_is_bit_exact(dq, table, full_run, tmp_path):
    for repository in repositories(dq, tmp_path):
        key = dq.ResultKey(20, {"set": "t"})
        context = (dq.AnalysisRunner.onData(table).addAnalyzers(analyzers(dq)).useRepository(repository)
                   .saveOrAppendResult(key).run())
        loaded = repository.loadByKey(key)
        assert set(loaded.metricMap) == set(analyzers(dq)) and len(loaded.metricMap) == len(analyzers(dq))
        for a in analyzers(dq):
            assert_same_metric(loaded.metricMap[a], context.metricMap[a])
            assert_same_metric(loaded.metricMap[a], full_run.metricMap[a])
        # and the stored history answers an anomaly check on the device metric
        check = dq.Check(dq.CheckLevel.Error, "same size").isNewestPointNonAnomalous(
            repository, dq.RateOfChangeStrategy(0.0, 0.0), dq.Size(), {"set": "t"}, None, None)
        assert check.evaluate(context).status == dq.CheckStatus.Success


class Launches:
    """Counts what reaches the device: every ScanPlan (dq_plan_create_opts) with its analyzers and columns, and the
    passes of the grouping and quantile analyzers."""

    def __init__(self, monkeypatch):
        from deequ_amd import grouping, quantiles, runner

        self.plans, self.other = [], []
        launches = self

        class Recording(runner.ScanPlan):
            def __init__(self, analyzers, schema, *args, **kwargs):
                super().__init__(analyzers, schema, *args, **kwargs)
                launches.plans.append((list(analyzers), list(self.columns)))

        monkeypatch.setattr(runner, "ScanPlan", Recording)
        for module, name in ((grouping, "build_frequencies"), (quantiles, "device_quantiles"),
                             (quantiles, "device_digest")):
            monkeypatch.setattr(module, name, self._counted(name, getattr(module, name)))

    def _counted(self, name, f):
        def call(*args, **kwargs):
            self.other.append(name)
            return f(*args, **kwargs)
        return call


def test_reuse_with_all_metrics_stored_creates_no_plan(dq, table, full_run, monkeypatch):
    repository, key = dq.InMemoryMetricsRepository(), dq.ResultKey(1)
    repository.save(key, full_run)
    launches = Launches(monkeypatch)
    context = (dq.AnalysisRunner.onData(table).addAnalyzers(analyzers(dq)).useRepository(repository)
               .reuseExistingResultsForKey(key, failIfResultsMissing=True).run())
    assert launches.plans == [] and launches.other == []
    assert context.metricMap == full_run.metricMap
    # the same through a verification run: the constraints are evaluated on the stored metrics
    check = dq.Check(dq.CheckLevel.Error, "stored").hasSize(lambda n: n == N).hasMean("x", lambda m: m > 0)
    result = (dq.VerificationSuite().onData(table).addCheck(check).addRequiredAnalyzers(analyzers(dq))
              .useRepository(repository).reuseExistingResultsForKey(key).run())
    assert result.status == dq.CheckStatus.Success and launches.plans == [] and launches.other == []
    # without the reuse key the plan is built
    dq.AnalysisRunner.onData(table).addAnalyzers([dq.Size(), dq.Mean("x")]).useRepository(repository).run()
    assert [(a, c) for a, c in launches.plans] == [([dq.Size(), dq.Mean("x")], ["x"])]


def test_reuse_with_some_metrics_stored_plans_only_the_missing(dq, table, full_run, monkeypatch):
    missing = [dq.Mean("y"), dq.StandardDeviation("y"), dq.Histogram("s")]
    repository, key = dq.InMemoryMetricsRepository(), dq.ResultKey(1)
    repository.save(key, dq.AnalyzerContext({a: m for a, m in full_run.metricMap.items() if a not in missing}))
    launches = Launches(monkeypatch)
    context = (dq.AnalysisRunner.onData(table).addAnalyzers(analyzers(dq)).useRepository(repository)
               .reuseExistingResultsForKey(key).run())
    assert launches.plans == [([dq.Mean("y"), dq.StandardDeviation("y")], ["y"])]   # x, k and s never enter the plan
    assert launches.other == ["build_frequencies"]                                 # Histogram(s) alone
    assert set(context.metricMap) == set(full_run.metricMap)
    for a in analyzers(dq):
        assert_same_metric(context.metricMap[a], full_run.metricMap[a])
    assert repository.loadByKey(key).metric(dq.Mean("y")) is None                  # reuse alone stores nothing


def test_fail_if_results_missing(dq, table, full_run, monkeypatch):
    repository, key = dq.InMemoryMetricsRepository(), dq.ResultKey(1)
    repository.save(key, dq.AnalyzerContext({a: m for a, m in full_run.metricMap.items()
                                             if a not in (dq.Mean("y"), dq.Histogram("s"))}))
    launches = Launches(monkeypatch)
    builder = (dq.AnalysisRunner.onData(table).addAnalyzers(analyzers(dq)).useRepository(repository)
               .reuseExistingResultsForKey(key, failIfResultsMissing=True))
    with pytest.raises(dq.ReusingNotPossibleResultsMissingException) as e:
        builder.run()
    assert str(e.value) == ("Could not find all necessary results in the MetricsRepository, the calculation of "
                            "the metrics for these analyzers would be needed: Mean(y,None), Histogram(s,None,1000)")
    assert launches.plans == [] and launches.other == []
    with pytest.raises(dq.ReusingNotPossibleResultsMissingException):
        (dq.VerificationSuite().onData(table).addRequiredAnalyzers(analyzers(dq)).useRepository(repository)
         .reuseExistingResultsForKey(key, True).run())
    assert launches.plans == [] and launches.other == []


def test_two_runs_under_one_key_leave_the_union(dq, table, full_run, tmp_path):
    first = [dq.Size(), dq.Mean("x"), dq.Histogram("s")]
    second = [dq.StandardDeviation("y"), dq.Correlation("x", "y"), dq.ApproxQuantile("x", 0.5)]
    for repository in repositories(dq, tmp_path):
        key = dq.ResultKey(5, {"set": "t"})
        dq.AnalysisRunner.onData(table).addAnalyzers(first).useRepository(repository).saveOrAppendResult(key).run()
        assert set(repository.loadByKey(key).metricMap) == set(first)
        (dq.VerificationSuite().onData(table).addRequiredAnalyzers(second).useRepository(repository)
         .saveOrAppendResult(key).run())
        stored = repository.loadByKey(key).metricMap
        assert set(stored) == set(first + second) and len(stored) == 6              # existing ++ new
        for a in first + second:
            assert_same_metric(stored[a], full_run.metricMap[a])
        # a metric computed again replaces the stored one of the same analyzer, a failed one is not stored
        rerun = [dq.Mean("x"), dq.Mean("s")]
        context = (dq.AnalysisRunner.onData(table).addAnalyzers(rerun).useRepository(repository)
                   .saveOrAppendResult(key).run())
        assert context.metric(dq.Mean("s")).value.isFailure
        assert set(repository.loadByKey(key).metricMap) == set(first + second)
        assert len(repository.load().get()) == 1
