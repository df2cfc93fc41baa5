"""deequ_amd.anomaly against tests/golden/anomaly_kats.json: every case of the reference's anomaly detection tests.

Host only.  Anomaly indices are compared exactly, and the doubles the reference pins for OnlineNormalStrategy's running
statistics with ==.
"""
import json
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "anomaly_kats.json")) as f:
    K = json.load(f)


@pytest.fixture(scope="module")
def A():
    from deequ_amd import anomaly

    return anomaly


def _strategy(A, case):
    return getattr(A, case["strategy"])(**case["params"])


def _detect(A, case):
    series = K["series"][case["series"]]
    strategy = _strategy(A, case)
    return series, (strategy.detect(series) if case["interval"] is None else
                    strategy.detect(series, tuple(case["interval"])))


def _id(case):
    return f"{case.get('strategy', '')}-{case.get('name', case['source'])}".replace(" ", "_")


def test_fixture_covers_every_strategy():
    assert {c["strategy"] for c in K["detect_cases"]} == {"SimpleThresholdStrategy", "RateOfChangeStrategy",
                                                          "BatchNormalStrategy", "OnlineNormalStrategy"}
    assert len(K["series"]["online"]) == 51 and len(K["series"]["batch"]) == 50
    assert len(K["series"]["online_variance"]) == 1000


@pytest.mark.parametrize("case", K["detect_cases"], ids=_id)
def test_detect(A, case):
    series, got = _detect(A, case)
    assert [i for i, _ in got] == case["expected_indices"]
    # Seq[(Int, Anomaly)] equality: the value of the point, confidence 1.0 (the detail is not compared)
    assert got == [(i, A.Anomaly(series[i], 1.0)) for i in case["expected_indices"]]


@pytest.mark.parametrize("case", K["detail_cases"], ids=_id)
def test_detail_states_value_and_bounds(A, case):
    number = re.compile(K["test_utils"]["regex"])
    _, got = _detect(A, case)
    assert got
    for _, anomaly in got:
        value, lower, upper = [float(m[0]) for m in number.findall(anomaly.detail)][:3]
        if case["value_is_first"]:
            assert anomaly.value is not None and value == anomaly.value
        assert value < lower or value > upper


def test_detail_number_regex():
    u = K["test_utils"]
    number = re.compile(u["regex"])
    assert number.search(u["no_number"]) is None
    assert float(number.search(u["first"][0])[0]) == u["first"][1]
    assert [float(m[0]) for m in number.findall(u["first_three"][0])][:3] == u["first_three"][1]


def test_detail_texts(A):
    """The texts as the reference builds them, doubles as java.lang.Double.toString prints them."""
    got = A.SimpleThresholdStrategy(upperBound=1.0).detect([-1.0, 2.0])
    assert got[0][1].detail == ("[SimpleThresholdStrategy]: Value 2.0 is not in bounds "
                                "[-1.7976931348623157E308, 1.0]")
    got = A.RateOfChangeStrategy(maxRateIncrease=8.0, order=2).detect([0.0, 1.0, 3.0, 6.0, 18.0, 72.0], (5, 6))
    assert got[0][1].detail == ("[RateOfChangeStrategy]: Change of 42.0 is not in bounds "
                                "[-1.7976931348623157E308, 8.0]. Order=2")
    got = A.BatchNormalStrategy(3.0, 3.0).detect([1.0, 1.0, 1.0, 1000.0, 500.0, 1.0], (3, 5))
    assert got[0][1].detail == "[BatchNormalStrategy]: Value 1000.0 is not in bounds [1.0, 1.0]."
    got = A.OnlineNormalStrategy(1.5, 1.5, 0.2).detect([1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0])
    assert [i for i, _ in got] == [3]
    assert got[0][1].detail.startswith("[OnlineNormalStrategy]: Value 2.0 is not in bounds [")


@pytest.mark.parametrize("case", K["online_stats_cases"], ids=_id)
def test_online_running_statistics(A, case):
    strategy = A.OnlineNormalStrategy(**case["params"])
    results = strategy.computeStatsAndAnomalies(K["series"][case["series"]])
    assert len(results) == len(K["series"][case["series"]])
    last = results[-1]
    for field, expected in case["last_point"].items():
        assert getattr(last, field) == expected, field  # == on doubles: to the last bit
    if "stdDev_close_to" in case:
        assert abs(last.stdDev - case["stdDev_close_to"]) < case["stdDev_close_to"] * case["stdDev_relative_tolerance"]


def test_online_statistics_keep_the_order_of_operations(A):
    """mean_k = mean + (1.0 / k) * (x - mean), Sn += (x - lastMean) * (x - mean), variance = Sn / k, written out for a
    series on which another association of the same formula rounds differently."""
    series = [0.1, 0.7, 0.3, 1e-3, 12.5, 0.30000000000000004]
    strategy = A.OnlineNormalStrategy(None, 1e6, 0.0, ignoreAnomalies=False)
    mean = sn = 0.0
    for k, (x, got) in enumerate(zip(series, strategy.computeStatsAndAnomalies(series)), start=1):
        last = mean
        mean = x if k == 1 else last + (1.0 / k) * (x - last)
        sn += (x - last) * (x - mean)
        assert (got.mean, got.stdDev, got.isAnomaly) == (mean, math.sqrt(sn / k), False)


def test_online_ignore_start_and_ignore_anomalies(A):
    series = [1.0, 1.0, 1.0, 50.0, 1.0, 1.0, 1.0, 1.0, 1.0, 50.0]
    flagged = lambda s: [i for i, r in enumerate(s.computeStatsAndAnomalies(series)) if r.isAnomaly]
    assert flagged(A.OnlineNormalStrategy(1.5, 1.5, 0.2)) == [3, 9]
    assert flagged(A.OnlineNormalStrategy(1.5, 1.5, 0.4)) == [9]        # index 3 < 10 * 0.4: never flagged
    kept = A.OnlineNormalStrategy(1.5, 1.5, 0.2, ignoreAnomalies=True).computeStatsAndAnomalies(series)
    assert kept[3].mean == 1.0 and kept[3].stdDev > 0.0 and kept[4].mean == 1.0 and kept[4].stdDev == 0.0
    moved = A.OnlineNormalStrategy(1.5, 1.5, 0.2, ignoreAnomalies=False).computeStatsAndAnomalies(series)
    assert moved[3].mean == 1.0 + (1.0 / 4) * 49.0 and moved[4].mean > 1.0
    # the search interval is half open and limits the flags, not the statistics
    assert [i for i, _ in A.OnlineNormalStrategy(1.5, 1.5, 0.2).detect(series, (3, 9))] == [3]
    assert [i for i, _ in A.OnlineNormalStrategy(1.5, 1.5, 0.2).detect(series, (4, 10))] == [9]


def test_batch_normal_include_interval_and_half_open_interval(A):
    series = [1.0, 1.0, 1.0, 1000.0, 500.0, 1.0]
    # [3, 4): 500.0 joins the statistics, mean 100.8, sample stdDev 223.2, upper bound 770.3
    assert [i for i, _ in A.BatchNormalStrategy(3.0, 3.0).detect(series, (3, 4))] == [3]
    # [4, 5): 1000.0 joins them, mean 200.8, stdDev 446.8, upper bound 1541.1: 500.0 is inside
    assert [i for i, _ in A.BatchNormalStrategy(3.0, 3.0).detect(series, (4, 5))] == []
    assert [i for i, _ in A.BatchNormalStrategy(3.0, 3.0).detect(series, (3, 5))] == [3, 4]
    assert [i for i, _ in A.BatchNormalStrategy(1.0, 1.0, includeInterval=True).detect(series)] == [3]
    mean, variance, n = A.mean_and_variance([2.0, 4.0, 4.0, 4.0, 5.0, 5.0, 7.0, 9.0])
    assert (mean, n) == (5.0, 8) and abs(variance - 32.0 / 7.0) < 1e-15
    assert A.mean_and_variance([3.0]) == (3.0, 0.0, 1)


@pytest.mark.parametrize("case", K["diff_cases"], ids=_id)
def test_rate_of_change_diff(A, case):
    got = A.RateOfChangeStrategy(-2.0, 2.0).diff(case["data"], case["order"])
    assert got == case["expected"]


@pytest.mark.parametrize("case", K["require_cases"], ids=_id)
def test_require_messages(A, case):
    with pytest.raises(ValueError) as e:
        strategy = _strategy(A, case)
        assert "series" in case, "the constructor was expected to fail"
        series = K["series"][case["series"]]
        strategy.detect(series) if case["interval"] is None else strategy.detect(series, tuple(case["interval"]))
    assert str(e.value) == case["message"]


class _Stub:
    """The stubbed strategy of AnomalyDetectorTest: answers the one call it expects."""

    def __init__(self, A, sees, returns):
        self.A, self.sees, self.returns, self.calls = A, sees, returns, []

    def detect(self, dataSeries, searchInterval):
        self.calls.append([list(dataSeries), list(searchInterval)])
        return [(i, self.A.Anomaly(v, 1.0)) for i, v in self.returns]


@pytest.mark.parametrize("case", K["detector_cases"], ids=_id)
def test_detector_preprocessing(A, case):
    stub = _Stub(A, case["strategy_sees"], case["strategy_returns"])
    data = [A.DataPoint(t, v) for t, v in case["data"]]
    detector = A.AnomalyDetector(stub)
    got = (detector.detectAnomaliesInHistory(data) if case["interval"] is None else
           detector.detectAnomaliesInHistory(data, tuple(case["interval"])))
    assert stub.calls == [case["strategy_sees"]]
    assert got == A.DetectionResult([(t, A.Anomaly(v, 1.0)) for t, v in case["expected"]])


@pytest.mark.parametrize("case", K["detector_require_cases"], ids=_id)
def test_detector_require_messages(A, case):
    detector = A.AnomalyDetector(A.SimpleThresholdStrategy(upperBound=1.0))
    data = [A.DataPoint(t, v) for t, v in case["data"]]
    with pytest.raises(ValueError) as e:
        if case["call"] == "isNewPointAnomalous":
            detector.isNewPointAnomalous(data, A.DataPoint(*case["newPoint"]))
        else:
            detector.detectAnomaliesInHistory(data, tuple(case["interval"]))
    assert str(e.value) == case["message"]


def test_is_new_point_anomalous(A):
    detector = A.AnomalyDetector(A.SimpleThresholdStrategy(upperBound=1.0))
    history = [A.DataPoint(3, 5.0), A.DataPoint(1, 0.5), A.DataPoint(2, None)]  # unsorted, one missing, one anomaly
    assert detector.isNewPointAnomalous(history, A.DataPoint(4, 0.9)).anomalies == []  # only the new point counts
    assert detector.isNewPointAnomalous(history, A.DataPoint(4, 1.5)) == A.DetectionResult([(4, A.Anomaly(1.5, 1.0))])
    # a missing new value is removed with the other missing values: nothing to flag
    assert detector.isNewPointAnomalous(history, A.DataPoint(4, None)).anomalies == []
    rate = A.AnomalyDetector(A.RateOfChangeStrategy(maxRateIncrease=1.0))
    assert rate.isNewPointAnomalous([A.DataPoint(2, 1.0), A.DataPoint(1, 9.0)], A.DataPoint(3, 2.5)).anomalies != []
    assert rate.isNewPointAnomalous([A.DataPoint(2, 2.0), A.DataPoint(1, 9.0)], A.DataPoint(3, 2.5)).anomalies == []


def test_history_utils(A):
    from deequ_amd.metrics import DoubleMetric, Entity, Failure, Success

    h = K["history_utils"]
    make = {None: None, "failure": DoubleMetric(Entity.Column, "metric-name", "instance-name", Failure(ValueError()))}
    metrics = [(t, make[m] if not isinstance(m, float) else
                DoubleMetric(Entity.Column, "metric-name", "instance-name", Success(m))) for t, m in h["metrics"]]
    assert [A.HistoryUtils.extractMetricValue(m) for _, m in metrics] == [v for _, v in h["expected"]]
    assert A.HistoryUtils.extractMetricValues(metrics) == [A.DataPoint(t, v) for t, v in h["expected"]]


def test_holt_winters_is_not_carried_over(A):
    with pytest.raises(NotImplementedError, match="L-BFGS-B"):
        A.HoltWinters()
