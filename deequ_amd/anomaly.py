"""Anomaly detection over a history of metric values.

Mirrors (paths relative to src/main/scala/com/amazon/deequ/anomalydetection/):
  DetectionResult.scala:19-56          Anomaly (equal by value and confidence, not by detail), DetectionResult
  AnomalyDetector.scala:21-102         DataPoint, AnomalyDetector
  AnomalyDetectionStrategy.scala       detect(dataSeries, searchInterval = (0, Int.MaxValue))
  HistoryUtils.scala:24-48             HistoryUtils
  SimpleThresholdStrategy.scala:25-58, RateOfChangeStrategy.scala:35-104, BatchNormalStrategy.scala:33-95,
  OnlineNormalStrategy.scala:39-155

A Scala `require(cond, msg)` is a ValueError("requirement failed: msg") here, an Option is a value or None, and a
double inside a detail text is printed as java.lang.Double.toString prints it.  The arithmetic keeps the reference's
order of operations: OnlineNormalStrategy's running mean and variance are equal to the last bit.
seasonal/HoltWinters.scala is not carried over (see HoltWinters below).
"""
from __future__ import annotations

import bisect
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from .grouping import _java_double_to_string as _d

DOUBLE_MAX = 1.7976931348623157e308  # Double.MaxValue; Double.MinValue is its negation
INT_MAX = 2 ** 31 - 1
LONG_MIN, LONG_MAX = -2 ** 63, 2 ** 63 - 1


def _require(condition: bool, message: str) -> None:
    if not condition:
        raise ValueError(f"requirement failed: {message}")


def _or(option: Optional[float], default: float) -> float:
    return default if option is None else option


def _sqrt(x: float) -> float:  # scala.math.sqrt: NaN below zero
    return math.sqrt(x) if x >= 0.0 else float("nan")


class Anomaly:  # DetectionResult.scala:19-54
    __slots__ = ("value", "confidence", "detail")

    def __init__(self, value: Optional[float], confidence: float, detail: Optional[str] = None):
        self.value, self.confidence, self.detail = value, confidence, detail

    def __eq__(self, other):  # the detail is ignored (:34-39)
        return isinstance(other, Anomaly) and other.value == self.value and other.confidence == self.confidence

    def __hash__(self):
        return hash((self.value, self.confidence))

    def __repr__(self):
        return f"Anomaly({self.value}, {self.confidence}, {self.detail!r})"


@dataclass(eq=True)
class DetectionResult:  # DetectionResult.scala:56
    anomalies: Sequence[Tuple[int, Anomaly]] = ()

    def __post_init__(self):
        self.anomalies = list(self.anomalies)


@dataclass(frozen=True)
class DataPoint:  # AnomalyDetector.scala:21
    time: int
    metricValue: Optional[float]


class HistoryUtils:  # HistoryUtils.scala:24-48
    @staticmethod
    def extractMetricValues(metrics: Sequence[Tuple[int, Optional[object]]]) -> List[DataPoint]:
        return [DataPoint(date, HistoryUtils.extractMetricValue(metric)) for date, metric in metrics]

    @staticmethod
    def extractMetricValue(metric) -> Optional[float]:
        """None for a missing metric and for a failed one (metric.flatMap(_.value.toOption))."""
        if metric is None or metric.value.isFailure:
            return None
        return metric.value.get()


class AnomalyDetectionStrategy:  # AnomalyDetectionStrategy.scala
    def detect(self, dataSeries: Sequence[float], searchInterval: Tuple[int, int] = (0, INT_MAX)) -> List[Tuple[int, Anomaly]]:
        raise NotImplementedError


class AnomalyDetector:  # AnomalyDetector.scala:29-102
    def __init__(self, strategy: AnomalyDetectionStrategy):
        self.strategy = strategy

    def isNewPointAnomalous(self, historicalDataPoints: Sequence[DataPoint], newPoint: DataPoint) -> DetectionResult:
        _require(len(historicalDataPoints) > 0, "historicalDataPoints must not be empty!")
        points = sorted(historicalDataPoints, key=lambda p: p.time)
        first, last = points[0].time, points[-1].time
        _require(last < newPoint.time,
                 "Can't decide which range to use for anomaly detection. New data point with time "
                 f"{newPoint.time} is in history range ({first} - {last})!")
        return DetectionResult(self.detectAnomaliesInHistory(points + [newPoint], (newPoint.time, LONG_MAX)).anomalies)

    def detectAnomaliesInHistory(self, dataSeries: Sequence[DataPoint],
                                 searchInterval: Tuple[int, int] = (LONG_MIN, LONG_MAX)) -> DetectionResult:
        """Anomalies with a time in [searchStart, searchEnd): missing values removed, the rest ordered by time (a
        stable sort, as sortBy), the bounds turned into indices of that series."""
        searchStart, searchEnd = searchInterval
        _require(searchStart <= searchEnd, "The first interval element has to be smaller or equal to the last.")
        series = sorted((p for p in dataSeries if p.metricValue is not None), key=lambda p: p.time)
        timestamps = [p.time for p in series]
        lower = bisect.bisect_left(timestamps, searchStart)
        upper = bisect.bisect_left(timestamps, searchEnd)
        anomalies = self.strategy.detect([p.metricValue for p in series], (lower, upper))
        return DetectionResult([(timestamps[index], anomaly) for index, anomaly in anomalies])


class SimpleThresholdStrategy(AnomalyDetectionStrategy):  # SimpleThresholdStrategy.scala:25-58
    def __init__(self, lowerBound: float = -DOUBLE_MAX, upperBound: Optional[float] = None):
        if upperBound is None:
            raise TypeError("SimpleThresholdStrategy: upperBound has no default")
        self.lowerBound, self.upperBound = float(lowerBound), float(upperBound)
        _require(self.lowerBound <= self.upperBound, "The lower bound must be smaller or equal to the upper bound.")

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        searchStart, searchEnd = searchInterval
        _require(searchStart <= searchEnd, "The start of the interval can't be larger than the end.")
        out = []
        for index in range(max(searchStart, 0), min(searchEnd, len(dataSeries))):
            value = dataSeries[index]
            if value < self.lowerBound or value > self.upperBound:
                detail = (f"[SimpleThresholdStrategy]: Value {_d(value)} is not in "
                          f"bounds [{_d(self.lowerBound)}, {_d(self.upperBound)}]")
                out.append((index, Anomaly(value, 1.0, detail)))
        return out


class RateOfChangeStrategy(AnomalyDetectionStrategy):  # RateOfChangeStrategy.scala:35-104
    def __init__(self, maxRateDecrease: Optional[float] = None, maxRateIncrease: Optional[float] = None,
                 order: int = 1):
        self.maxRateDecrease = None if maxRateDecrease is None else float(maxRateDecrease)
        self.maxRateIncrease = None if maxRateIncrease is None else float(maxRateIncrease)
        self.order = order
        _require(self.maxRateDecrease is not None or self.maxRateIncrease is not None,
                 "At least one of the two limits (maxRateDecrease or maxRateIncrease) has to be specified.")
        _require(_or(self.maxRateDecrease, -DOUBLE_MAX) <= _or(self.maxRateIncrease, DOUBLE_MAX),
                 "The maximal rate of increase has to be bigger than the maximal rate of decrease.")
        _require(order >= 0, "Order of derivative cannot be negative.")

    def diff(self, dataSeries: Sequence[float], order: int) -> List[float]:
        """The order-th discrete difference (:61-70): one element shorter per order."""
        _require(order >= 0, "Order of diff cannot be negative")
        data = list(dataSeries)
        while order > 0 and data:
            data = [right - left for left, right in zip(data[:-1], data[1:])]
            order -= 1
        return data

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        _require(searchInterval[0] <= searchInterval[1], "The start of the interval cannot be larger than the end.")
        startPoint = max(searchInterval[0] - self.order, 0)
        data = self.diff(list(dataSeries)[startPoint:max(searchInterval[1], 0)], self.order)
        low, high = _or(self.maxRateDecrease, -DOUBLE_MAX), _or(self.maxRateIncrease, DOUBLE_MAX)
        out = []
        for index, change in enumerate(data):
            if change < low or change > high:
                at = index + startPoint + self.order
                detail = (f"[RateOfChangeStrategy]: Change of {_d(change)} is not in bounds ["
                          f"{_d(low)}, {_d(high)}]. Order={self.order}")
                out.append((at, Anomaly(dataSeries[at], 1.0, detail)))
        return out


def mean_and_variance(values: Sequence[float]) -> Tuple[float, float, int]:
    """breeze.stats.meanAndVariance as BatchNormalStrategy uses it: one pass, mu += 1/n * d and
    s += (n - 1) * d / n * d with d = y - mu, the sample variance s / (n - 1), and 0 for fewer than two values.
    (Restated from breeze's published source; no breeze build was available to compare the last bit.)"""
    mu, s, n = 0.0, 0.0, 0
    for y in values:
        n += 1
        d = y - mu
        mu = mu + 1.0 / n * d
        s = s + (n - 1) * d / n * d
    return mu, (s / (n - 1) if n > 1 else 0.0), n


def _factor_checks(lowerDeviationFactor, upperDeviationFactor) -> None:
    _require(lowerDeviationFactor is not None or upperDeviationFactor is not None,
             "At least one factor has to be specified.")
    _require(_or(lowerDeviationFactor, 1.0) >= 0 and _or(upperDeviationFactor, 1.0) >= 0,
             "Factors cannot be smaller than zero.")


class BatchNormalStrategy(AnomalyDetectionStrategy):  # BatchNormalStrategy.scala:33-95
    def __init__(self, lowerDeviationFactor: Optional[float] = 3.0, upperDeviationFactor: Optional[float] = 3.0,
                 includeInterval: bool = False):
        self.lowerDeviationFactor = None if lowerDeviationFactor is None else float(lowerDeviationFactor)
        self.upperDeviationFactor = None if upperDeviationFactor is None else float(upperDeviationFactor)
        self.includeInterval = includeInterval
        _factor_checks(self.lowerDeviationFactor, self.upperDeviationFactor)

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        searchStart, searchEnd = searchInterval
        _require(searchStart <= searchEnd, "The start of the interval can't be larger than the end.")
        _require(len(dataSeries) > 0, "Data series is empty. Can't calculate mean/ stdDev.")
        _require(self.includeInterval or searchEnd - searchStart < len(dataSeries),
                 "Excluding values in searchInterval from calculation but not enough values remain to "
                 "calculate mean and stdDev.")
        data = list(dataSeries)
        lo, hi = max(searchStart, 0), max(searchEnd, 0)
        mean, variance, _ = mean_and_variance(data if self.includeInterval else data[:lo] + data[hi:])
        stdDev = _sqrt(variance)
        upperBound = mean + _or(self.upperDeviationFactor, DOUBLE_MAX) * stdDev
        lowerBound = mean - _or(self.lowerDeviationFactor, DOUBLE_MAX) * stdDev
        out = []
        for index in range(lo, min(hi, len(data))):
            value = data[index]
            if value > upperBound or value < lowerBound:
                detail = (f"[BatchNormalStrategy]: Value {_d(value)} is not in "
                          f"bounds [{_d(lowerBound)}, {_d(upperBound)}].")
                out.append((index, Anomaly(value, 1.0, detail)))
        return out


@dataclass(frozen=True)
class OnlineCalculationResult:  # OnlineNormalStrategy.scala:58
    mean: float
    stdDev: float
    isAnomaly: bool


class OnlineNormalStrategy(AnomalyDetectionStrategy):  # OnlineNormalStrategy.scala:39-155
    def __init__(self, lowerDeviationFactor: Optional[float] = 3.0, upperDeviationFactor: Optional[float] = 3.0,
                 ignoreStartPercentage: float = 0.1, ignoreAnomalies: bool = True):
        self.lowerDeviationFactor = None if lowerDeviationFactor is None else float(lowerDeviationFactor)
        self.upperDeviationFactor = None if upperDeviationFactor is None else float(upperDeviationFactor)
        self.ignoreStartPercentage = float(ignoreStartPercentage)
        self.ignoreAnomalies = ignoreAnomalies
        _factor_checks(self.lowerDeviationFactor, self.upperDeviationFactor)
        _require(0 <= self.ignoreStartPercentage <= 1.0,
                 "Percentage of start values to ignore must be in interval [0, 1].")

    def computeStatsAndAnomalies(self, dataSeries: Sequence[float],
                                 searchInterval: Tuple[int, int] = (0, INT_MAX)) -> List[OnlineCalculationResult]:
        """The running mean and standard deviation after every value and whether the value is an anomaly against
        them (:70-120); the statements are in the reference's order, so the doubles are the reference's."""
        ret: List[OnlineCalculationResult] = []
        currentMean = 0.0
        currentVariance = 0.0
        Sn = 0.0
        numValuesToSkip = len(dataSeries) * self.ignoreStartPercentage
        upperFactor = _or(self.upperDeviationFactor, DOUBLE_MAX)
        lowerFactor = _or(self.lowerDeviationFactor, DOUBLE_MAX)
        searchStart, searchEnd = searchInterval
        for currentIndex, currentValue in enumerate(dataSeries):
            lastMean, lastVariance, lastSn = currentMean, currentVariance, Sn
            if currentIndex == 0:
                currentMean = currentValue
            else:
                currentMean = lastMean + (1.0 / (currentIndex + 1)) * (currentValue - lastMean)
            Sn += (currentValue - lastMean) * (currentValue - currentMean)
            currentVariance = Sn / (currentIndex + 1)
            stdDev = _sqrt(currentVariance)
            upperBound = currentMean + upperFactor * stdDev
            lowerBound = currentMean - lowerFactor * stdDev
            if (currentIndex < numValuesToSkip or currentIndex < searchStart or currentIndex >= searchEnd
                    or (currentValue <= upperBound and currentValue >= lowerBound)):
                ret.append(OnlineCalculationResult(currentMean, stdDev, False))
            else:
                if self.ignoreAnomalies:  # the anomaly leaves mean and variance as they were
                    currentMean, currentVariance, Sn = lastMean, lastVariance, lastSn
                ret.append(OnlineCalculationResult(currentMean, stdDev, True))
        return ret

    def detect(self, dataSeries, searchInterval=(0, INT_MAX)):
        searchStart, searchEnd = searchInterval
        _require(searchStart <= searchEnd, "The start of the interval can't be larger than the end.")
        results = self.computeStatsAndAnomalies(dataSeries, searchInterval)
        out = []
        for index in range(max(searchStart, 0), min(searchEnd, len(results))):
            r = results[index]
            if not r.isAnomaly:
                continue
            lowerBound = r.mean - _or(self.lowerDeviationFactor, DOUBLE_MAX) * r.stdDev
            upperBound = r.mean + _or(self.upperDeviationFactor, DOUBLE_MAX) * r.stdDev
            detail = (f"[OnlineNormalStrategy]: Value {_d(dataSeries[index])} is not in "
                      f"bounds [{_d(lowerBound)}, {_d(upperBound)}].")
            out.append((index, Anomaly(dataSeries[index], 1.0, detail)))
        return out


class HoltWinters(AnomalyDetectionStrategy):  # seasonal/HoltWinters.scala
    """Not carried over.  The reference fits the smoothing parameters with breeze's L-BFGS-B and its forecast, and
    with it every anomaly it reports, depends on that optimiser's iterates; without breeze they cannot be restated
    exactly, and an approximate fit would report other anomalies under the same name."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(
            "HoltWinters is not available: the reference fits it through breeze's L-BFGS-B, whose iterates its "
            "results depend on and which cannot be restated exactly here")
