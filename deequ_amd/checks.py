"""Check DSL + VerificationSuite over the GPU scan -- the callers of the hot path.

The reference's user entry point for config C1 is VerificationSuite().onData(df).addCheck(check).run()
(VerificationSuite.scala:42-130, VerificationRunBuilder.scala:28-149): the checks' analyzers are unioned
with the required ones, run through AnalysisRunner.doAnalysisRun (ONE fused scan: here dq_plan / dq_scan),
and every constraint's assertion is evaluated on the metrics (Check.scala:878-890,
AnalysisBasedConstraint.scala:42-122).  This module mirrors the constraint methods whose analyzers are on
the GPU path, with the reference's predicate strings (Check.scala:670-871), constraint names
(Constraint.scala:83-536) and failure messages, so a check runs unchanged on the MI355X path.  The grouping
constraints (isUnique, hasUniqueness, hasEntropy, ...) and hasDataType are constraint factories over the analyzers of
grouping.py and the DataType analyzer; they are what the suggested constraints of suggestions.py resolve to.
"""
from __future__ import annotations

from enum import IntEnum
from typing import Callable, Dict, List, Optional, Sequence

from .analyzers import (Analyzer, ApproxCountDistinct, Completeness, Compliance, Correlation, MaxLength, Maximum, Mean,
                        MinLength, Minimum, PatternMatch, Size, StandardDeviation, Sum)
from .analyzers import DataType, DataTypeInstances
from .grouping import (Distinctness, Entropy, Histogram, MutualInformation, Uniqueness, UniqueValueRatio,
                       _java_double_to_string)
from .matching import DatasetMatch, ReferentialIntegrity
from .drift import DistributionDistance
from .quantiles import ApproxQuantile
from .runner import AnalysisRunner, AnalyzerContext, arrow_data


class CheckLevel(IntEnum):  # Check.scala:30-32
    Error = 0
    Warning = 1


class CheckStatus(IntEnum):  # Check.scala:34-36 (Enumeration order: Success < Warning < Error)
    Success = 0
    Warning = 1
    Error = 2


class ConstraintStatus(IntEnum):  # Constraint.scala:25-27
    Success = 0
    Failure = 1


class ConstrainableDataTypes(IntEnum):  # ConstrainableDataTypes.scala:19-26
    Null = 0
    Fractional = 1
    Integral = 2
    Boolean = 3
    String = 4
    Numeric = 5  # union of integral and fractional


MISSING_ANALYSIS = "Missing Analysis, can't run the constraint!"          # AnalysisBasedConstraint.scala:117
PROBLEMATIC_METRIC_PICKER = "Can't retrieve the value to assert on"       # :118
ASSERTION_EXCEPTION = "Can't execute the assertion"                       # :119


class ConstraintResult:  # Constraint.scala:29-33
    def __init__(self, constraint, status: ConstraintStatus, message: Optional[str] = None, metric=None):
        self.constraint, self.status, self.message, self.metric = constraint, status, message, metric

    def __repr__(self):
        return f"ConstraintResult({self.constraint}, {self.status.name}, {self.message!r})"


class AnalysisBasedConstraint:  # AnalysisBasedConstraint.scala:42-111
    def __init__(self, analyzer: Analyzer, assertion: Callable, value_picker: Optional[Callable] = None,
                 hint: Optional[str] = None):
        self.analyzer, self.assertion, self.value_picker, self.hint = analyzer, assertion, value_picker, hint

    def evaluate(self, metric_map: Dict) -> ConstraintResult:
        metric = metric_map.get(self.analyzer)
        if metric is None:
            return ConstraintResult(self, ConstraintStatus.Failure, MISSING_ANALYSIS, None)
        if metric.value.isFailure:
            return ConstraintResult(self, ConstraintStatus.Failure, str(metric.value.failed), metric)
        value = metric.value.get()
        try:
            assert_on = self.value_picker(value) if self.value_picker else value
        except Exception as e:
            return ConstraintResult(self, ConstraintStatus.Failure, f"{PROBLEMATIC_METRIC_PICKER}: {e}!", metric)
        try:
            ok = bool(self.assertion(assert_on))
        except Exception as e:
            return ConstraintResult(self, ConstraintStatus.Failure, f"{ASSERTION_EXCEPTION}: {e}!", metric)
        if ok:
            return ConstraintResult(self, ConstraintStatus.Success, None, metric)
        shown = _java_double_to_string(assert_on) if isinstance(assert_on, float) else str(assert_on)
        msg = f"Value: {shown} does not meet the constraint requirement!"
        if self.hint:
            msg += f" {self.hint}"
        return ConstraintResult(self, ConstraintStatus.Failure, msg, metric)

    def __str__(self):  # the case class's toString (functions print as <function1>, Options as Some(..) / None)
        picker = "Some(<function1>)" if self.value_picker else "None"
        hint = f"Some({self.hint})" if self.hint is not None else "None"
        return f"AnalysisBasedConstraint({self.analyzer},<function1>,{picker},{hint})"


class NamedConstraint:  # Constraint.scala:40-69 (ConstraintDecorator keeps the name in the result)
    def __init__(self, inner: AnalysisBasedConstraint, name: str):
        self.inner, self.name = inner, name

    def evaluate(self, metric_map: Dict) -> ConstraintResult:
        r = self.inner.evaluate(metric_map)
        r.constraint = self
        return r

    def __str__(self):
        return self.name

    __repr__ = __str__


def _named(analyzer, assertion, kind: str, picker=None, hint=None) -> NamedConstraint:
    return NamedConstraint(AnalysisBasedConstraint(analyzer, assertion, picker, hint), f"{kind}({analyzer})")


def _is_one(v) -> bool:  # Check.IsOne
    return v == 1.0


def ratio_types(ignore_unknown: bool, key_type: str, distribution) -> float:
    """ratioTypes (Constraint.scala:589-613): the key type's share of the distribution's values, of the values that
    are not Unknown when ignore_unknown; 0.0 when the key type has no values."""
    entry = distribution.values.get(key_type)
    if not ignore_unknown:
        return 0.0 if entry is None else entry.ratio
    absolute = 0 if entry is None else entry.absolute
    if absolute == 0:
        return 0.0
    num_values = sum(v.absolute for v in distribution.values.values())
    unknown = distribution.values.get(DataTypeInstances.Unknown)
    return float(absolute) / float(num_values - (0 if unknown is None else unknown.absolute))


def data_type_value_picker(dataType: ConstrainableDataTypes) -> Callable:
    """dataTypeConstraint's valuePicker (Constraint.scala:556-567)."""
    I, T = DataTypeInstances, ConstrainableDataTypes
    if dataType == T.Null:
        return lambda d: ratio_types(False, I.Unknown, d)
    if dataType == T.Numeric:
        return lambda d: ratio_types(True, I.Fractional, d) + ratio_types(True, I.Integral, d)
    key = {T.Fractional: I.Fractional, T.Integral: I.Integral, T.Boolean: I.Boolean, T.String: I.String}[T(dataType)]
    return lambda d: ratio_types(True, key, d)


def data_type_constraint(column, dataType, assertion=_is_one, hint=None) -> AnalysisBasedConstraint:
    """Constraint.dataTypeConstraint (Constraint.scala:548-571): the one factory that returns the bare
    AnalysisBasedConstraint, so its name is that case class's toString."""
    return AnalysisBasedConstraint(DataType(column), assertion, data_type_value_picker(dataType), hint)


def is_newest_point_non_anomalous(metricsRepository, anomalyDetectionStrategy, analyzer, withTagValues,
                                  afterDate: Optional[int], beforeDate: Optional[int],
                                  currentMetricValue: float) -> bool:
    """Check.isNewestPointNonAnomalous of the companion object (Check.scala:926-983): the history of the analyzer's
    metric from the repository (tag filter, before and after both inclusive), the current value appended one tick
    after the newest stored result, and the strategy asked about that last point only."""
    from .anomaly import AnomalyDetector, DataPoint, HistoryUtils

    loader = metricsRepository.load().withTagValues(withTagValues)
    if beforeDate is not None:
        loader = loader.before(beforeDate)
    if afterDate is not None:
        loader = loader.after(afterDate)
    results = loader.forAnalyzers([analyzer]).get()
    if not results:
        raise ValueError("requirement failed: There have to be previous results in the MetricsRepository!")
    # results of one dateTime are ordered by their tag values first (the sort is stable)
    historical = []
    for r in sorted(results, key=lambda r: list(r.resultKey.tags.values())):
        metrics = list(r.analyzerContext.metricMap.values())
        historical.append((r.resultKey.dataSetDate, metrics[0] if metrics else None))
    testDateTime = max(r.resultKey.dataSetDate for r in results) + 1
    if testDateTime == 2 ** 63 - 1:
        raise ValueError("requirement failed: Test DateTime cannot be Long.MaxValue, otherwise the"
                         "Anomaly Detection, which works with an open upper interval bound, won't test anything")
    detected = AnomalyDetector(anomalyDetectionStrategy).isNewPointAnomalous(
        HistoryUtils.extractMetricValues(historical), DataPoint(testDateTime, currentMetricValue))
    return not detected.anomalies


class CheckResult:  # Check.scala:39-42
    def __init__(self, check: "Check", status: CheckStatus, constraintResults: List[ConstraintResult]):
        self.check, self.status, self.constraintResults = check, status, constraintResults


class Check:  # Check.scala:59-902
    def __init__(self, level: CheckLevel, description: str, constraints: Sequence = ()):
        self.level, self.description, self.constraints = level, description, list(constraints)

    def addConstraint(self, constraint) -> "Check":
        return Check(self.level, self.description, self.constraints + [constraint])

    def _filterable(self, create: Callable[[Optional[str]], NamedConstraint]) -> "CheckWithLastConstraintFilterable":
        return CheckWithLastConstraintFilterable(self.level, self.description, self.constraints + [create(None)], create)

    # ---- constraints on GPU-path analyzers (Constraint.scala factories) ----------------------------
    def hasSize(self, assertion, hint=None):
        return self._filterable(lambda w: _named(Size(w), assertion, "SizeConstraint", lambda v: int(v), hint))

    def isComplete(self, column, hint=None):
        return self._filterable(lambda w: _named(Completeness(column, w), _is_one, "CompletenessConstraint", None, hint))

    def hasCompleteness(self, column, assertion, hint=None):
        return self._filterable(lambda w: _named(Completeness(column, w), assertion, "CompletenessConstraint", None, hint))

    def hasMin(self, column, assertion, hint=None):
        return self._filterable(lambda w: _named(Minimum(column, w), assertion, "MinimumConstraint", None, hint))

    def hasMax(self, column, assertion, hint=None):
        return self._filterable(lambda w: _named(Maximum(column, w), assertion, "MaximumConstraint", None, hint))

    def hasMinLength(self, column, assertion, hint=None):  # (Deequ 1.0.3 Check.hasMinLength)
        return self._filterable(lambda w: _named(MinLength(column, w), assertion, "MinLengthConstraint", None, hint))

    def hasMaxLength(self, column, assertion, hint=None):
        return self._filterable(lambda w: _named(MaxLength(column, w), assertion, "MaxLengthConstraint", None, hint))

    def hasMean(self, column, assertion, hint=None):
        return self._filterable(lambda w: _named(Mean(column, w), assertion, "MeanConstraint", None, hint))

    def hasSum(self, column, assertion, hint=None):
        return self._filterable(lambda w: _named(Sum(column, w), assertion, "SumConstraint", None, hint))

    def hasStandardDeviation(self, column, assertion, hint=None):
        return self._filterable(
            lambda w: _named(StandardDeviation(column, w), assertion, "StandardDeviationConstraint", None, hint))

    def hasApproxCountDistinct(self, column, assertion, hint=None):
        return self._filterable(
            lambda w: _named(ApproxCountDistinct(column, w), assertion, "ApproxCountDistinctConstraint", None, hint))

    def hasCorrelation(self, columnA, columnB, assertion, hint=None):
        return self._filterable(
            lambda w: _named(Correlation(columnA, columnB, w), assertion, "CorrelationConstraint", None, hint))

    def hasPattern(self, column, pattern, assertion=_is_one, name=None, hint=None):  # Check.scala:560-575
        text = pattern if isinstance(pattern, str) else pattern.pattern

        def create(w):  # Constraint.patternMatchConstraint (Constraint.scala:290-312)
            c = AnalysisBasedConstraint(PatternMatch(column, pattern, w), assertion, None, hint)
            return NamedConstraint(c, name or f"PatternMatchConstraint({column}, {text})")
        return self._filterable(create)

    def satisfies(self, columnCondition, constraintName, assertion=_is_one, hint=None):  # Check.scala:538-548
        return self._filterable(lambda w: _named(Compliance(constraintName, columnCondition, w), assertion,
                                                 "ComplianceConstraint", None, hint))

    def isNonNegative(self, column, hint=None):  # Check.scala:670-677
        return self.satisfies(f"COALESCE({column}, 0.0) >= 0", f"{column} is non-negative", hint=hint)

    def isPositive(self, column):  # Check.scala:685-688
        return self.satisfies(f"COALESCE({column}, 1.0) > 0", f"{column} is positive")

    def isLessThan(self, columnA, columnB, hint=None):  # Check.scala:699-707
        return self.satisfies(f"{columnA} < {columnB}", f"{columnA} is less than {columnB}", hint=hint)

    def isLessThanOrEqualTo(self, columnA, columnB, hint=None):
        return self.satisfies(f"{columnA} <= {columnB}", f"{columnA} is less than or equal to {columnB}", hint=hint)

    def isGreaterThan(self, columnA, columnB, hint=None):
        return self.satisfies(f"{columnA} > {columnB}", f"{columnA} is greater than {columnB}", hint=hint)

    def isGreaterThanOrEqualTo(self, columnA, columnB, hint=None):
        return self.satisfies(f"{columnA} >= {columnB}", f"{columnA} is greater than or equal to {columnB}",
                              hint=hint)

    def isContainedIn(self, column, *args, **kw):
        """isContainedIn(column, allowedValues[, assertion][, hint]) (Check.scala:772-842) or
        isContainedIn(column, lowerBound, upperBound, includeLowerBound, includeUpperBound, hint) (:855-871)."""
        if args and isinstance(args[0], (list, tuple)):
            allowed = list(args[0])
            rest = list(args[1:])
            assertion = rest.pop(0) if rest and callable(rest[0]) else kw.get("assertion", _is_one)
            hint = rest.pop(0) if rest else kw.get("hint")
            values = ",".join("'" + v.replace("'", "''") + "'" for v in allowed)
            predicate = f"`{column}` IS NULL OR `{column}` IN ({values})"
            return self.satisfies(predicate, f"{column} contained in {','.join(allowed)}", assertion, hint)
        names = ["lowerBound", "upperBound", "includeLowerBound", "includeUpperBound", "hint"]
        vals = dict(zip(names, args))
        vals.update(kw)
        lo, hi = float(vals["lowerBound"]), float(vals["upperBound"])
        left = ">=" if vals.get("includeLowerBound", True) else ">"
        right = "<=" if vals.get("includeUpperBound", True) else "<"
        los, his = _java_double_to_string(lo), _java_double_to_string(hi)
        predicate = f"`{column}` IS NULL OR (`{column}` {left} {los} AND `{column}` {right} {his})"
        return self.satisfies(predicate, f"{column} between {los} and {his}", hint=vals.get("hint"))

    def hasReferentialIntegrity(self, columns, reference, assertion=_is_one, hint=None):
        """The fraction of rows whose `columns` tuple is a key of `reference` (a matching.KeySet) meets the assertion;
        a NULL in a key column is not contained.  (Upstream: Check.doesDatasetMatch / ReferentialIntegrity.)"""
        return self._filterable(lambda w: _named(ReferentialIntegrity(columns, reference, w), assertion,
                                                 "ReferentialIntegrityConstraint", None, hint))

    def doesDatasetMatch(self, keyColumns, compareColumns, reference, assertion=_is_one, hint=None):
        """The fraction of rows that equal `reference`'s row with the same key (a matching.KeyedRows) meets the
        assertion: key column k against key k of the reference, compareColumns (names on both sides, a dict
        {column: reference column}, or None for every payload column) null-safe equal.  (Upstream:
        Check.doesDatasetMatch with matchColumnMappings.)"""
        return self._filterable(lambda w: _named(DatasetMatch(keyColumns, compareColumns, reference, w), assertion,
                                                 "DatasetMatchConstraint", None, hint))

    def hasDistributionDistance(self, columns, reference, assertion, method="linf", binning=None, hint=None):
        """The distance between the distribution of `columns` and `reference`'s (a drift.ReferenceDistribution) meets
        the assertion; method: "linf" (upstream's Distance.categoricalDistance), "tv", "js" or "ks"; binning: a
        binning.Bins the reference was built with.  NULL rows are part of neither distribution."""
        return self._filterable(lambda w: _named(DistributionDistance(columns, reference, method, binning, w),
                                                 assertion, "DistributionDistanceConstraint", None, hint))

    # ---- constraints on the grouping, histogram and quantile analyzers: filterable, the `where` is the analyzer's ----
    def isUnique(self, column, hint=None):  # Check.scala:139-141
        return self._filterable(lambda w: _named(Uniqueness([column], w), _is_one, "UniquenessConstraint", None, hint))

    def isPrimaryKey(self, column, *columns):  # Check.scala:151-153
        return self._filterable(lambda w: _named(Uniqueness([column, *columns], w), _is_one, "UniquenessConstraint"))

    def hasUniqueness(self, columns, assertion, hint=None):  # Check.scala:176-221
        return self._filterable(lambda w: _named(Uniqueness(columns, w), assertion, "UniquenessConstraint", None, hint))

    def hasDistinctness(self, columns, assertion, hint=None):  # Check.scala:232-238
        return self._filterable(lambda w: _named(Distinctness(columns, w), assertion, "DistinctnessConstraint", None,
                                                 hint))

    def hasUniqueValueRatio(self, columns, assertion, hint=None):  # Check.scala:249-256
        def create(w):
            a = UniqueValueRatio(columns, w)
            # (Constraint.scala:254 leaves the name's parenthesis open)
            return NamedConstraint(AnalysisBasedConstraint(a, assertion, None, hint), f"UniqueValueRatioConstraint({a}")
        return self._filterable(create)

    def hasNumberOfDistinctValues(self, column, assertion, binningUdf=None, maxBins=Histogram.MaximumAllowedDetailBins,
                                  hint=None, *, binning=None):
        # Check.scala:269-278, histogramBinConstraint (Constraint.scala:133-147); binning: a binning.Bins
        return self._filterable(lambda w: _named(Histogram(column, binningUdf, maxBins, binning, where=w), assertion,
                                                 "HistogramBinConstraint", lambda d: d.numberOfBins, hint))

    def hasHistogramValues(self, column, assertion, binningUdf=None, maxBins=Histogram.MaximumAllowedDetailBins,
                           hint=None, *, binning=None):  # Check.scala:295-304; binning: a binning.Bins
        return self._filterable(lambda w: _named(Histogram(column, binningUdf, maxBins, binning, where=w), assertion,
                                                 "HistogramConstraint", None, hint))

    def hasEntropy(self, column, assertion, hint=None):  # Check.scala:353-360
        return self._filterable(lambda w: _named(Entropy(column, w), assertion, "EntropyConstraint", None, hint))

    def hasMutualInformation(self, columnA, columnB, assertion, hint=None):  # Check.scala:371-379
        return self._filterable(lambda w: _named(MutualInformation(columnA, columnB, w), assertion,
                                                 "MutualInformationConstraint", None, hint))

    # ---- DataType (plain addConstraint: no .where) -------------------------------------------------
    def hasDataType(self, column, dataType, assertion=_is_one, hint=None):  # Check.scala:653-661
        return self.addConstraint(data_type_constraint(column, dataType, assertion, hint))

    def hasApproxQuantile(self, column, quantile, assertion, hint=None):  # Check.scala:391-398
        return self._filterable(lambda w: _named(ApproxQuantile(column, quantile, where=w), assertion,
                                                 "ApproxQuantileConstraint", None, hint))

    # the pattern checks of Check.scala:581-642; a pattern outside the GPU regex subset (the credit card and social
    # security number patterns) gives the failure metric PatternMatch gives for it
    def containsCreditCardNumber(self, column, assertion=_is_one, hint=None):
        from .analyzers import Patterns

        return self.hasPattern(column, Patterns.CREDITCARD, assertion, f"containsCreditCardNumber({column})", hint)

    def containsEmail(self, column, assertion=_is_one, hint=None):
        from .analyzers import Patterns

        return self.hasPattern(column, Patterns.EMAIL, assertion, f"containsEmail({column})", hint)

    def containsURL(self, column, assertion=_is_one, hint=None):
        from .analyzers import Patterns

        return self.hasPattern(column, Patterns.URL, assertion, f"containsURL({column})", hint)

    def containsSocialSecurityNumber(self, column, assertion=_is_one, hint=None):
        from .analyzers import Patterns

        return self.hasPattern(column, Patterns.SOCIAL_SECURITY_NUMBER_US, assertion,
                               f"containsSocialSecurityNumber({column})", hint)

    def isNewestPointNonAnomalous(self, metricsRepository, anomalyDetectionStrategy, analyzer, withTagValues=None,
                                  afterDate=None, beforeDate=None, hint=None):  # Check.scala:322-342
        def assertion(currentMetricValue):
            return is_newest_point_non_anomalous(metricsRepository, anomalyDetectionStrategy, analyzer,
                                                 dict(withTagValues or {}), afterDate, beforeDate, currentMetricValue)
        # Constraint.anomalyConstraint (Constraint.scala:180-190)
        return self.addConstraint(_named(analyzer, assertion, "AnomalyConstraint", None, hint))

    # ---- evaluation --------------------------------------------------------------------------------
    def evaluate(self, context: AnalyzerContext) -> CheckResult:  # Check.scala:878-890
        results = [c.evaluate(context.metricMap) for c in self.constraints]
        failed = any(r.status == ConstraintStatus.Failure for r in results)
        status = CheckStatus.Success
        if failed:
            status = CheckStatus.Error if self.level == CheckLevel.Error else CheckStatus.Warning
        return CheckResult(self, status, results)

    def requiredAnalyzers(self) -> List[Analyzer]:  # Check.scala:892-901
        out = []
        for c in self.constraints:
            inner = c.inner if isinstance(c, NamedConstraint) else c
            if isinstance(inner, AnalysisBasedConstraint) and inner.analyzer not in out:
                out.append(inner.analyzer)
        return out


class CheckWithLastConstraintFilterable(Check):  # CheckWithLastConstraintFilterable.scala:20-40
    def __init__(self, level, description, constraints, create):
        super().__init__(level, description, constraints)
        self._create = create

    def where(self, filter: str) -> Check:
        return Check(self.level, self.description, self.constraints[:-1] + [self._create(filter)])


class VerificationResult:  # VerificationResult.scala:33-36
    def __init__(self, status: CheckStatus, checkResults: Dict, metrics: Dict):
        self.status, self.checkResults, self.metrics = status, checkResults, metrics

    def successMetricsAsJson(self) -> str:
        return AnalyzerContext(self.metrics).successMetricsAsJson()

    def rowLevelResults(self, data, filteredRow: str = "TRUE"):
        """Which rows of `data` (a Table or a list of chunks) pass each check and each constraint of this run
        (VerificationResult.rowLevelResultsAsDataFrame): rowlevel.row_level_results over the run's checks."""
        from .rowlevel import row_level_results

        return row_level_results(list(self.checkResults), data, filteredRow)


class VerificationSuite:  # VerificationSuite.scala:42-282
    def onData(self, data) -> "VerificationRunBuilder":
        return VerificationRunBuilder(data)

    @staticmethod
    def doVerificationRun(data, checks: Sequence[Check], requiredAnalyzers: Sequence[Analyzer] = (),
                          aggregateWith=None, saveStatesWith=None, metricsRepository=None,
                          reuseExistingResultsForKey=None, failIfResultsForReusingMissing: bool = False,
                          saveOrAppendResultsWithKey=None) -> VerificationResult:
        data = arrow_data(data)
        analyzers = list(requiredAnalyzers) + [a for c in checks for a in c.requiredAnalyzers()]
        # the analysis run reuses but does not save (VerificationSuite.scala:121-130): the checks, the anomaly checks
        # among them, are evaluated against the repository as it was, and the metrics are stored after that (:132-139)
        context = AnalysisRunner.doAnalysisRun(data, analyzers, aggregateWith, saveStatesWith, metricsRepository,
                                               reuseExistingResultsForKey, failIfResultsForReusingMissing, None)
        result = VerificationSuite._evaluate(checks, context)
        if metricsRepository is not None and saveOrAppendResultsWithKey is not None:
            from .repository import save_or_append_result

            save_or_append_result(AnalyzerContext(result.metrics), metricsRepository, saveOrAppendResultsWithKey)
        return result

    @staticmethod
    def _evaluate(checks, context: AnalyzerContext) -> VerificationResult:  # VerificationSuite.scala:263-281
        results = {c: c.evaluate(context) for c in checks}
        status = max((r.status for r in results.values()), default=CheckStatus.Success)
        return VerificationResult(CheckStatus(status), results, context.metricMap)


class AnomalyCheckConfig:  # VerificationRunBuilder.scala:303-308
    def __init__(self, level: CheckLevel, description: str, withTagValues: Optional[Dict[str, str]] = None,
                 afterDate: Optional[int] = None, beforeDate: Optional[int] = None):
        self.level, self.description = level, description
        self.withTagValues: Dict[str, str] = dict(withTagValues or {})
        self.afterDate, self.beforeDate = afterDate, beforeDate


def getAnomalyCheck(metricsRepository, anomalyDetectionStrategy, analyzer,
                    anomalyCheckConfig: AnomalyCheckConfig) -> Check:
    """VerificationRunBuilderHelper.getAnomalyCheck (VerificationRunBuilder.scala:269-285)."""
    return Check(anomalyCheckConfig.level, anomalyCheckConfig.description).isNewestPointNonAnomalous(
        metricsRepository, anomalyDetectionStrategy, analyzer, anomalyCheckConfig.withTagValues,
        anomalyCheckConfig.afterDate, anomalyCheckConfig.beforeDate)


class VerificationRunBuilder:  # VerificationRunBuilder.scala:28-149
    def __init__(self, data):
        self.data = arrow_data(data)
        self.checks: List[Check] = []
        self.required: List[Analyzer] = []
        self._aggregateWith = None
        self._saveStatesWith = None
        self._metricsRepository = None
        self._reuseExistingResultsKey = None
        self._failIfResultsForReusingMissing = False
        self._saveOrAppendResultsKey = None

    def addCheck(self, check: Check) -> "VerificationRunBuilder":
        self.checks.append(check)
        return self

    def addChecks(self, checks: Sequence[Check]) -> "VerificationRunBuilder":
        self.checks.extend(checks)
        return self

    def addRequiredAnalyzer(self, a: Analyzer) -> "VerificationRunBuilder":
        self.required.append(a)
        return self

    def addRequiredAnalyzers(self, analyzers: Sequence[Analyzer]) -> "VerificationRunBuilder":
        self.required.extend(analyzers)
        return self

    def aggregateWith(self, loader) -> "VerificationRunBuilder":
        self._aggregateWith = loader
        return self

    def saveStatesWith(self, persister) -> "VerificationRunBuilder":
        self._saveStatesWith = persister
        return self

    # VerificationRunBuilderWithRepository (VerificationRunBuilder.scala:151-211): one builder class here
    def useRepository(self, metricsRepository) -> "VerificationRunBuilder":
        self._metricsRepository = metricsRepository
        return self

    def reuseExistingResultsForKey(self, resultKey, failIfResultsMissing: bool = False) -> "VerificationRunBuilder":
        self._reuseExistingResultsKey = resultKey
        self._failIfResultsForReusingMissing = failIfResultsMissing
        return self

    def saveOrAppendResult(self, resultKey) -> "VerificationRunBuilder":
        self._saveOrAppendResultsKey = resultKey
        return self

    def addAnomalyCheck(self, anomalyDetectionStrategy, analyzer,
                        anomalyCheckConfig: Optional[AnomalyCheckConfig] = None) -> "VerificationRunBuilder":
        """A check that the analyzer's new metric is no anomaly against its history in the repository (:194-210);
        without a config: level Warning, description "Anomaly check for <analyzer>"."""
        if self._metricsRepository is None:
            raise ValueError("addAnomalyCheck needs a metrics repository: call useRepository first")
        config = anomalyCheckConfig or AnomalyCheckConfig(CheckLevel.Warning, f"Anomaly check for {analyzer}")
        self.checks.append(getAnomalyCheck(self._metricsRepository, anomalyDetectionStrategy, analyzer, config))
        return self

    def segmentBy(self, columns, maxSegments: int = 10000):
        """The checks once per distinct tuple of `columns` (segments.run_segmented): a new builder whose run() gives a
        SegmentedVerificationResult; more than maxSegments segments is a ValueError before any grouped launch."""
        from .segments import SegmentedVerificationRunBuilder

        return SegmentedVerificationRunBuilder(self.data, columns, maxSegments, self.checks, self.required)

    def run(self) -> VerificationResult:
        return VerificationSuite.doVerificationRun(self.data, self.checks, self.required, self._aggregateWith,
                                                   self._saveStatesWith, self._metricsRepository,
                                                   self._reuseExistingResultsKey, self._failIfResultsForReusingMissing,
                                                   self._saveOrAppendResultsKey)
