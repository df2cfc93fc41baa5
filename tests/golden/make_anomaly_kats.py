"""Write anomaly_kats.json: the inputs and outcomes of the reference's anomaly detection tests, as data.

Paths are relative to src/test/scala/com/amazon/deequ/anomalydetection/.  Every case states its source lines.

Seeded series.  OnlineNormalStrategyTest (:31-40, :100-102) and BatchNormalStrategyTest (:30-39) draw their series
from scala.util.Random(1).nextGaussian().  java.util.Random is restated below from its published specification (the
48-bit LCG, nextDouble, the polar method of nextGaussian with its cached second value) and the generated numbers are
committed, so no seeded case is left out.  The one difference a JVM could show is the last bit of a gaussian:
nextGaussian takes StrictMath.log and StrictMath.sqrt (fdlibm), this generator math.log and math.sqrt; sqrt is exact
in both and log is within an ulp in both.  The expected anomaly indices are the reference's own (20..30 etc.) and do
not hang on that bit: the planted anomalies are tens of standard deviations out.

Doubles the reference pins for OnlineNormalStrategy.computeStatsAndAnomalies are held as `last_point` (mean, stdDev):
literal ones (:117-118), and where it asserts equality with breeze's meanAndVariance (:109, :131) the value of that
algorithm, restated here from breeze's published source as breeze_mean_and_variance.
"""
import json
import math
import os


class JavaRandom:
    """java.util.Random: seed scrambled with 0x5DEECE66D, next(bits) of the 48-bit LCG."""

    def __init__(self, seed):
        self.seed = (seed ^ 0x5DEECE66D) & ((1 << 48) - 1)
        self.next_next_gaussian = None

    def next(self, bits):
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        return self.seed >> (48 - bits)

    def next_double(self):
        return ((self.next(26) << 27) + self.next(27)) * (1.0 / (1 << 53))

    def next_gaussian(self):
        if self.next_next_gaussian is not None:
            g, self.next_next_gaussian = self.next_next_gaussian, None
            return g
        while True:
            v1 = 2 * self.next_double() - 1
            v2 = 2 * self.next_double() - 1
            s = v1 * v1 + v2 * v2
            if 0 < s < 1:
                break
        multiplier = math.sqrt(-2 * math.log(s) / s)
        self.next_next_gaussian = v2 * multiplier
        return v1 * multiplier


def breeze_mean_and_variance(values):
    mu, s, n = 0.0, 0.0, 0
    for y in values:
        n += 1
        d = y - mu
        mu = mu + 1.0 / n * d
        s = s + (n - 1) * d / n * d
    return mu, (s / (n - 1) if n > 1 else 0.0)


def planted(n):  # dist(i) += i + (i % 2 * -2 * i) for i in 20..30 over n gaussians of Random(1)
    r = JavaRandom(1)
    dist = [r.next_gaussian() for _ in range(n)]
    for i in range(20, 31):
        dist[i] += i + (i % 2 * -2 * i)
    return r, dist


def span(a, b, step=1):
    return list(range(a, b + 1, step))


MAX = 1.7976931348623157e308
online_r, online_data = planted(51)        # OnlineNormalStrategyTest.scala:31-40 (0 to 50)
variance_data = [online_r.next_gaussian() * (5000.0 / i) for i in range(1, 1001)]  # :100-102, the same Random
_, batch_data = planted(50)                # BatchNormalStrategyTest.scala:30-39 (0 to 49)
rate_data = [1.0 if (i < 20 or i > 30) else float(i if i % 2 == 0 else -i) for i in range(51)]  # RateOfChange :27-33
ONES = [1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0]
ON = {"lowerDeviationFactor": 1.5, "upperDeviationFactor": 1.5, "ignoreStartPercentage": 0.2}  # Online :29-30
BN = {"lowerDeviationFactor": 1.0, "upperDeviationFactor": 1.0}                                 # Batch :27-28
RC = {"maxRateDecrease": -2.0, "maxRateIncrease": 2.0}                                          # Rate :26
ST = {"upperBound": 1.0}                                                                        # Simple :25
SIMPLE_DATA = [-1.0, 2.0, 3.0, 0.5]

series = {"online": online_data, "online_variance": variance_data, "batch": batch_data, "rate": rate_data,
          "simple": SIMPLE_DATA, "ones": ONES, "empty": [], "rate_orders": [0.0, 1.0, 3.0, 6.0, 18.0, 72.0],
          "rate_small": [1.0, -1.0, 4.0, -7.0], "batch_small": [1.0, 1.0, 1.0, 1000.0, 500.0, 1.0]}


def detect(strategy, params, data, interval, expected, source, name):
    return {"name": name, "source": source, "strategy": strategy, "params": params, "series": data,
            "interval": interval, "expected_indices": expected}


detect_cases = [
    # SimpleThresholdStrategyTest.scala
    detect("SimpleThresholdStrategy", ST, "simple", [0, 4], [1, 2], "SimpleThresholdStrategyTest.scala:29-33", "above threshold"),
    detect("SimpleThresholdStrategy", ST, "simple", None, [1, 2], "SimpleThresholdStrategyTest.scala:35-39", "no range"),
    detect("SimpleThresholdStrategy", ST, "empty", None, [], "SimpleThresholdStrategyTest.scala:41-46", "empty input"),
    detect("SimpleThresholdStrategy", {"lowerBound": -0.5, "upperBound": 1.0}, "simple", None, [0, 1, 2],
           "SimpleThresholdStrategyTest.scala:48-54", "upper and lower threshold"),
    # RateOfChangeStrategyTest.scala
    detect("RateOfChangeStrategy", RC, "rate", None, span(20, 31), "RateOfChangeStrategyTest.scala:35-41", "no interval"),
    detect("RateOfChangeStrategy", RC, "rate", [25, 50], span(25, 31), "RateOfChangeStrategyTest.scala:43-49", "in interval"),
    detect("RateOfChangeStrategy", {"maxRateDecrease": None, "maxRateIncrease": 1.0}, "rate", None, span(20, 30, 2),
           "RateOfChangeStrategyTest.scala:51-60", "no min rate"),
    detect("RateOfChangeStrategy", {"maxRateDecrease": -1.0, "maxRateIncrease": None}, "rate", None, span(21, 31, 2),
           "RateOfChangeStrategyTest.scala:62-71", "no max rate"),
    detect("RateOfChangeStrategy", {"maxRateDecrease": -MAX, "maxRateIncrease": MAX}, "rate", None, [],
           "RateOfChangeStrategyTest.scala:73-79", "min / max value"),
    detect("RateOfChangeStrategy", {"maxRateDecrease": None, "maxRateIncrease": 8.0, "order": 2}, "rate_orders", None,
           [4, 5], "RateOfChangeStrategyTest.scala:104-111", "higher order, no interval"),
    detect("RateOfChangeStrategy", {"maxRateDecrease": None, "maxRateIncrease": 8.0, "order": 2}, "rate_orders", [5, 6],
           [5], "RateOfChangeStrategyTest.scala:113-120", "higher order, interval"),
    detect("RateOfChangeStrategy", RC, "rate_small", None, [2, 3], "RateOfChangeStrategyTest.scala:122-128",
           "threshold-like (the test's strategy has order 1)"),
    detect("RateOfChangeStrategy", RC, "empty", None, [], "RateOfChangeStrategyTest.scala:142-147", "empty input"),
    # BatchNormalStrategyTest.scala
    detect("BatchNormalStrategy", BN, "batch", [25, 50], span(25, 30), "BatchNormalStrategyTest.scala:41-47", "in interval"),
    detect("BatchNormalStrategy", {"lowerDeviationFactor": None, "upperDeviationFactor": 1.0}, "batch", [20, 31],
           span(20, 30, 2), "BatchNormalStrategyTest.scala:49-58", "no lower factor"),
    detect("BatchNormalStrategy", {"lowerDeviationFactor": 1.0, "upperDeviationFactor": None}, "batch", [10, 30],
           span(21, 29, 2), "BatchNormalStrategyTest.scala:60-69", "no upper factor"),
    detect("BatchNormalStrategy", {"lowerDeviationFactor": 3.0, "upperDeviationFactor": 3.0}, "batch_small", [3, 5],
           [3, 4], "BatchNormalStrategyTest.scala:71-78", "interval left out of mean / stdDev"),
    detect("BatchNormalStrategy", {"lowerDeviationFactor": MAX, "upperDeviationFactor": MAX}, "batch", [30, 51], [],
           "BatchNormalStrategyTest.scala:88-94", "max value factors"),
    # OnlineNormalStrategyTest.scala
    detect("OnlineNormalStrategy", {"lowerDeviationFactor": 3.5, "upperDeviationFactor": 3.5, "ignoreStartPercentage": 0.2},
           "online", None, span(20, 30), "OnlineNormalStrategyTest.scala:42-50", "no interval"),
    detect("OnlineNormalStrategy", ON, "online", [25, 31], span(25, 30), "OnlineNormalStrategyTest.scala:52-58", "in interval"),
    detect("OnlineNormalStrategy", {"lowerDeviationFactor": None, "upperDeviationFactor": 1.5}, "online", None,
           span(20, 30, 2), "OnlineNormalStrategyTest.scala:60-70", "no lower factor"),
    detect("OnlineNormalStrategy", {"lowerDeviationFactor": 1.5, "upperDeviationFactor": None}, "online", None,
           span(21, 29, 2), "OnlineNormalStrategyTest.scala:72-82", "no upper factor"),
    detect("OnlineNormalStrategy", ON, "empty", None, [], "OnlineNormalStrategyTest.scala:84-89", "empty input"),
    detect("OnlineNormalStrategy", {"lowerDeviationFactor": MAX, "upperDeviationFactor": MAX}, "online", None, [],
           "OnlineNormalStrategyTest.scala:91-97", "max value factors"),
]

# detail texts: (value, lowerBound, upperBound) are the first three numbers, the value outside the bounds
detail_cases = [
    {"source": "SimpleThresholdStrategyTest.scala:62-72", "strategy": "SimpleThresholdStrategy", "params": ST,
     "series": "simple", "interval": None, "value_is_first": True},
    {"source": "RateOfChangeStrategyTest.scala:149-158", "strategy": "RateOfChangeStrategy", "params": RC,
     "series": "rate", "interval": None, "value_is_first": False},
    {"source": "BatchNormalStrategyTest.scala:111-121", "strategy": "BatchNormalStrategy", "params": BN,
     "series": "batch", "interval": [25, 50], "value_is_first": True},
    {"source": "OnlineNormalStrategyTest.scala:159-169", "strategy": "OnlineNormalStrategy", "params": ON,
     "series": "online", "interval": None, "value_is_first": True},
]

var_mean, var_variance = breeze_mean_and_variance(variance_data)
ones_mean, ones_variance = breeze_mean_and_variance(ONES)
online_stats_cases = [
    {"name": "calculate variance correctly", "source": "OnlineNormalStrategyTest.scala:99-111", "params": ON,
     "series": "online_variance", "last_point": {"mean": var_mean}, "stdDev_close_to": math.sqrt(var_variance),
     "stdDev_relative_tolerance": 0.001},
    {"name": "ignores anomalies in calculation if wanted", "source": "OnlineNormalStrategyTest.scala:113-119",
     "params": ON, "series": "ones", "last_point": {"mean": 1.0, "stdDev": 0.0, "isAnomaly": False}},
    {"name": "doesn't ignore anomalies in calculation if not wanted", "source": "OnlineNormalStrategyTest.scala:121-133",
     "params": dict(ON, ignoreAnomalies=False), "series": "ones", "last_point": {"mean": ones_mean},
     "stdDev_close_to": math.sqrt(ones_variance), "stdDev_relative_tolerance": 0.1},
]

diff_cases = [
    {"source": "RateOfChangeStrategyTest.scala:81-87", "data": [1.0, 2.0, 4.0, 1.0, 2.0, 8.0], "order": 1,
     "expected": [1.0, 2.0, -3.0, 1.0, 6.0], "tolerance": 0.0},
    {"source": "RateOfChangeStrategyTest.scala:89-95", "data": [1.0, 2.0, 4.0, 1.0, 2.0, 8.0], "order": 2,
     "expected": [1.0, -5.0, 4.0, 5.0], "tolerance": 0.0},
    # scalatest's === on Array[Double] against Array(47, 56, -280.99, 296.9765) is exact equality
    {"source": "RateOfChangeStrategyTest.scala:96-102", "data": [1.0, 5.0, -10.0, 3.0, 100.0, 0.01, 0.0065], "order": 3,
     "expected": [47.0, 56.0, -280.99, 296.9765], "tolerance": 0.0},
]

R = "requirement failed: "
require_cases = [  # the constructor or detect call that must fail, with the message of the require in src/main
    {"source": "SimpleThresholdStrategyTest.scala:56-60", "strategy": "SimpleThresholdStrategy",
     "params": {"lowerBound": 2.0, "upperBound": 1.0},
     "message": R + "The lower bound must be smaller or equal to the upper bound."},
    {"source": "RateOfChangeStrategyTest.scala:130-134", "strategy": "RateOfChangeStrategy",
     "params": {"maxRateDecrease": -2.0, "maxRateIncrease": -3.0},
     "message": R + "The maximal rate of increase has to be bigger than the maximal rate of decrease."},
    {"source": "RateOfChangeStrategyTest.scala:136-140", "strategy": "RateOfChangeStrategy",
     "params": {"maxRateDecrease": None, "maxRateIncrease": None},
     "message": R + "At least one of the two limits (maxRateDecrease or maxRateIncrease) has to be specified."},
    {"source": "RateOfChangeStrategy.scala:47", "strategy": "RateOfChangeStrategy",
     "params": {"maxRateDecrease": -1.0, "maxRateIncrease": 1.0, "order": -1},
     "message": R + "Order of derivative cannot be negative."},
    {"source": "BatchNormalStrategyTest.scala:96-103", "strategy": "BatchNormalStrategy",
     "params": {"lowerDeviationFactor": None, "upperDeviationFactor": -3.0},
     "message": R + "Factors cannot be smaller than zero."},
    {"source": "BatchNormalStrategyTest.scala:96-103", "strategy": "BatchNormalStrategy",
     "params": {"lowerDeviationFactor": -3.0, "upperDeviationFactor": None},
     "message": R + "Factors cannot be smaller than zero."},
    {"source": "BatchNormalStrategyTest.scala:105-109", "strategy": "BatchNormalStrategy",
     "params": {"lowerDeviationFactor": None, "upperDeviationFactor": None},
     "message": R + "At least one factor has to be specified."},
    {"source": "BatchNormalStrategyTest.scala:80-85", "strategy": "BatchNormalStrategy", "params": {},
     "series": "batch", "interval": None,
     "message": R + "Excluding values in searchInterval from calculation but not enough values remain to "
                    "calculate mean and stdDev."},
    {"source": "BatchNormalStrategy.scala:60", "strategy": "BatchNormalStrategy", "params": {"includeInterval": True},
     "series": "empty", "interval": None, "message": R + "Data series is empty. Can't calculate mean/ stdDev."},
    {"source": "OnlineNormalStrategyTest.scala:135-139", "strategy": "OnlineNormalStrategy",
     "params": {"lowerDeviationFactor": None, "upperDeviationFactor": None},
     "message": R + "At least one factor has to be specified."},
    {"source": "OnlineNormalStrategyTest.scala:141-148", "strategy": "OnlineNormalStrategy",
     "params": {"lowerDeviationFactor": None, "upperDeviationFactor": -3.0},
     "message": R + "Factors cannot be smaller than zero."},
    {"source": "OnlineNormalStrategyTest.scala:141-148", "strategy": "OnlineNormalStrategy",
     "params": {"lowerDeviationFactor": -3.0, "upperDeviationFactor": None},
     "message": R + "Factors cannot be smaller than zero."},
    {"source": "OnlineNormalStrategyTest.scala:150-157", "strategy": "OnlineNormalStrategy",
     "params": {"ignoreStartPercentage": 1.5},
     "message": R + "Percentage of start values to ignore must be in interval [0, 1]."},
    {"source": "OnlineNormalStrategyTest.scala:150-157", "strategy": "OnlineNormalStrategy",
     "params": {"ignoreStartPercentage": -1.0},
     "message": R + "Percentage of start values to ignore must be in interval [0, 1]."},
] + [{"source": src, "strategy": s, "params": p, "series": "simple", "interval": [3, 2], "message": R + m} for s, p, src, m in [
    ("SimpleThresholdStrategy", ST, "SimpleThresholdStrategy.scala:45", "The start of the interval can't be larger than the end."),
    ("RateOfChangeStrategy", RC, "RateOfChangeStrategy.scala:88-89", "The start of the interval cannot be larger than the end."),
    ("BatchNormalStrategy", BN, "BatchNormalStrategy.scala:58", "The start of the interval can't be larger than the end."),
    ("OnlineNormalStrategy", ON, "OnlineNormalStrategy.scala:137", "The start of the interval can't be larger than the end."),
]]


def pts(pairs):
    return [[t, v] for t, v in pairs]


DET = [[0, -1.0], [1, 2.0], [2, 3.0], [3, 0.5]]  # AnomalyDetectorTest.scala:27-29
# AnomalyDetectorTest stubs the strategy: `strategy_sees` is the (series, index interval) the stub expects, `strategy_
# returns` the (index, value) pairs it answers, `expected` the (time, value) pairs of the DetectionResult
detector_cases = [
    {"name": "ignore missing values", "source": "AnomalyDetectorTest.scala:33-43",
     "data": [[0, 1.0], [1, 2.0], [2, None], [3, 1.0]], "interval": [0, 4],
     "strategy_sees": [[1.0, 2.0, 1.0], [0, 3]], "strategy_returns": [[1, 2.0]], "expected": [[1, 2.0]]},
    {"name": "only detect values in range", "source": "AnomalyDetectorTest.scala:45-52", "data": DET, "interval": [2, 4],
     "strategy_sees": [[-1.0, 2.0, 3.0, 0.5], [2, 4]], "strategy_returns": [[2, 3.0]], "expected": [[2, 3.0]]},
    {"name": "ordered values with time gaps", "source": "AnomalyDetectorTest.scala:60-74",
     "data": pts((i * 200, 5.0) for i in range(1, 11)), "interval": [200, 401],
     "strategy_sees": [[5.0] * 10, [0, 2]], "strategy_returns": [[0, 5.0], [1, 5.0]],
     "expected": [[200, 5.0], [400, 5.0]]},
    {"name": "unordered values with time gaps", "source": "AnomalyDetectorTest.scala:76-90",
     "data": [[10, -1.0], [25, 2.0], [11, 3.0], [0, 0.5]], "interval": None,
     "strategy_sees": [[0.5, -1.0, 3.0, 2.0], [0, 4]], "strategy_returns": [[1, -1.0], [2, 3.0], [3, 2.0]],
     "expected": [[10, -1.0], [11, 3.0], [25, 2.0]]},
    {"name": "unordered values without time gaps", "source": "AnomalyDetectorTest.scala:92-105",
     "data": [[1, -1.0], [3, 2.0], [2, 3.0], [0, 0.5]], "interval": None,
     "strategy_sees": [[0.5, -1.0, 3.0, 2.0], [0, 4]], "strategy_returns": [[1, -1.0], [2, 3.0], [3, 2.0]],
     "expected": [[1, -1.0], [2, 3.0], [3, 2.0]]},
]
detector_require_cases = [
    {"source": "AnomalyDetectorTest.scala:54-58, AnomalyDetector.scala:85-86", "call": "detectAnomaliesInHistory",
     "data": DET, "interval": [4, 2],
     "message": R + "The first interval element has to be smaller or equal to the last."},
    {"source": "AnomalyDetector.scala:44", "call": "isNewPointAnomalous", "data": [], "newPoint": [5, 1.0],
     "message": R + "historicalDataPoints must not be empty!"},
    {"source": "AnomalyDetector.scala:53-55", "call": "isNewPointAnomalous", "data": DET, "newPoint": [3, 1.0],
     "message": R + "Can't decide which range to use for anomaly detection. New data point with time "
                    "3 is in history range (0 - 3)!"},
]

history_utils = {  # HistoryUtilsTest.scala:27-45: a missing metric, a failed one, Success(50)
    "source": "HistoryUtilsTest.scala:27-45",
    "metrics": [[0, None], [1, "failure"], [2, 50.0]],
    "expected": [[0, None], [1, None], [2, 50.0]],
}

test_utils = {  # AnomalyDetectionTestUtils.scala:26 and AnomalyDetectionTestUtilsTest.scala:25-47
    "source": "AnomalyDetectionTestUtils.scala:26-56, AnomalyDetectionTestUtilsTest.scala:25-47",
    "regex": "([+-]?([0-9]*[.])?[0-9]+([Ee][0-9]+)?)",
    "no_number": "noNumber",
    "first": ["xx3.141yyu4.2", 3.141],
    "first_three": ["In this 1 string are 3.000 values, not 42.01", [1.0, 3.0, 42.01]],
}

out = {
    "_comment": "generated by make_anomaly_kats.py; data only, see its docstring for the sources and the seeded series",
    "series": series, "detect_cases": detect_cases, "detail_cases": detail_cases,
    "online_stats_cases": online_stats_cases, "diff_cases": diff_cases, "require_cases": require_cases,
    "detector_cases": detector_cases, "detector_require_cases": detector_require_cases,
    "history_utils": history_utils, "test_utils": test_utils,
}

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "anomaly_kats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path)
