"""Constraint suggestion (suggestions/**): rules over column profiles, an optional device train / test split, and the
evaluation of the suggested check on the test side.

  rules                    suggestions/rules/*.scala -- shouldBeApplied / candidate / ruleDescription, restated with
                           the reference's descriptions and code strings (doubles printed as Scala's s"..." does)
  ConstraintSuggestion(s)  suggestions/ConstraintSuggestion.scala:27-114
  ConstraintSuggestionResult   suggestions/ConstraintSuggestionResult.scala:30-58 (plus numRecords and splitSeed)
  ConstraintSuggestionRunner / ConstraintSuggestionRunBuilder
                           suggestions/ConstraintSuggestionRunner.scala:56-315, ConstraintSuggestionRunBuilder.scala

Everything that touches data runs on the device: the split (split.py, dq_split_rows + the take compaction),
ColumnProfiler.profile on the training side and VerificationSuite on the test side.  The rules are host arithmetic
over a handful of numbers per column.  The metrics repository is out of scope.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from decimal import ROUND_DOWN, Decimal
from typing import Dict, List, Optional, Sequence

from .analyzers import Completeness, Compliance, DataTypeInstances
from .checks import (Check, CheckLevel, ConstrainableDataTypes, VerificationResult, VerificationSuite, _is_one, _named,
                     data_type_constraint)
from .grouping import Uniqueness, _java_double_to_string
from .profiles import NULL_FIELD_REPLACEMENT, ColumnProfile, ColumnProfiler, ColumnProfiles, NumericColumnProfile
from .runner import _chunks, arrow_data
from .split import check_ratio, random_split
from .table import Table

_d2s = _java_double_to_string  # Double.toString: how s"$x" and "..." + x print a Double


def round_down_2(x: float) -> float:
    """BigDecimal(x).setScale(2, RoundingMode.DOWN).toDouble.  Scala's BigDecimal(Double) goes through Double.toString
    (the shortest digits, not the exact binary value: 0.29 stays 0.29), and DOWN rounds toward zero."""
    return float(Decimal(_d2s(x)).quantize(Decimal("0.01"), rounding=ROUND_DOWN))


def round_target(p: float, n: int) -> float:
    """The lower end of the binomial confidence interval, rounded as the rules round it
    (RetainCompletenessRule.scala:36-37, FractionalCategoricalRangeRule.scala:72-73)."""
    return round_down_2(p - 1.96 * math.sqrt(p * (1 - p) / n))


def escape_java(s: str) -> str:
    """StringEscapeUtils.escapeJava: backslash, double quote and the control characters escaped, everything outside
    printable ASCII as \\uXXXX (upper-case hex, UTF-16 code units); the single quote stays."""
    named = {"\\": "\\\\", '"': '\\"', "\b": "\\b", "\n": "\\n", "\t": "\\t", "\f": "\\f", "\r": "\\r"}
    out = []
    for ch in s:
        if ch in named:
            out.append(named[ch])
        elif 32 <= ord(ch) <= 0x7F:
            out.append(ch)
        else:
            units = ch.encode("utf-16-be")
            out += [f"\\u{int.from_bytes(units[i:i + 2], 'big'):04X}" for i in range(0, len(units), 2)]
    return "".join(out)


def _by_popularity(items, key):
    """sortBy(key).reverse over a Scala Map's entries.  Ties unpinned: among equal keys the reference keeps the map's
    iteration order, which nothing pins; here ties are ordered by category descending."""
    return sorted(items, key=lambda kv: (key(kv[1]), kv[0]), reverse=True)


def _categories(values_by_popularity):
    sql = "'" + "', '".join(k.replace("'", "''") for k, _ in values_by_popularity) + "'"
    code = '"' + '", "'.join(escape_java(k) for k, _ in values_by_popularity) + '"'
    return sql, code


@dataclass(frozen=True)
class ConstraintRule:  # rules/ConstraintRule.scala:23-43
    ruleDescription = ""

    def shouldBeApplied(self, profile: ColumnProfile, numRecords: int) -> bool:
        raise NotImplementedError

    def candidate(self, profile: ColumnProfile, numRecords: int) -> "ConstraintSuggestion":
        raise NotImplementedError

    def __str__(self):  # the case class's toString
        return f"{type(self).__name__}()"


class CompleteIfCompleteRule(ConstraintRule):  # rules/CompleteIfCompleteRule.scala:25-46
    ruleDescription = "If a column is complete in the sample, we suggest a NOT NULL constraint"

    def shouldBeApplied(self, profile, numRecords):
        return profile.completeness == 1.0

    def candidate(self, profile, numRecords):
        constraint = _named(Completeness(profile.column), _is_one, "CompletenessConstraint")
        return ConstraintSuggestion(constraint, profile.column, "Completeness: " + _d2s(float(profile.completeness)),
                                    f"'{profile.column}' is not null", self, f'.isComplete("{profile.column}")')


class RetainCompletenessRule(ConstraintRule):  # rules/RetainCompletenessRule.scala:28-64
    ruleDescription = ("If a column is incomplete in the sample, we model its completeness as a binomial variable, "
                       "estimate a confidence interval and use this to define a lower bound for the completeness")

    def shouldBeApplied(self, profile, numRecords):
        return 0.2 < profile.completeness < 1.0

    def candidate(self, profile, numRecords):
        target = round_target(float(profile.completeness), numRecords)
        constraint = _named(Completeness(profile.column), lambda v: v >= target, "CompletenessConstraint")
        bound = int((1.0 - target) * 100)  # .toInt: toward zero
        return ConstraintSuggestion(
            constraint, profile.column, "Completeness: " + _d2s(float(profile.completeness)),
            f"'{profile.column}' has less than {bound}% missing values", self,
            f'.hasCompleteness("{profile.column}", _ >= {_d2s(target)}, Some("It should be above {_d2s(target)}!"))')


class RetainTypeRule(ConstraintRule):  # rules/RetainTypeRule.scala:26-60
    ruleDescription = "If we detect a non-string type, we suggest a type constraint"
    _TESTABLE = {DataTypeInstances.Fractional: ConstrainableDataTypes.Fractional,
                 DataTypeInstances.Integral: ConstrainableDataTypes.Integral,
                 DataTypeInstances.Boolean: ConstrainableDataTypes.Boolean}

    def shouldBeApplied(self, profile, numRecords):
        return bool(profile.isDataTypeInferred) and profile.dataType in self._TESTABLE

    def candidate(self, profile, numRecords):
        constraint = data_type_constraint(profile.column, self._TESTABLE[profile.dataType], _is_one)
        return ConstraintSuggestion(
            constraint, profile.column, "DataType: " + profile.dataType, f"'{profile.column}' has type {profile.dataType}",
            self, f'.hasDataType("{profile.column}", ConstrainableDataTypes.{profile.dataType})')


def _unique_value_ratio(profile) -> Optional[float]:
    """The share of histogram entries seen once; None without a histogram of a String column.  An empty histogram
    gives NaN as 0.0 / 0 does, which no threshold admits."""
    if profile.histogram is None or profile.dataType != DataTypeInstances.String:
        return None
    entries = profile.histogram.values
    unique = sum(1 for v in entries.values() if v.absolute == 1)
    return unique / len(entries) if entries else float("nan")


class CategoricalRangeRule(ConstraintRule):  # rules/CategoricalRangeRule.scala:28-77
    ruleDescription = "If we see a categorical range for a column, we suggest an IS IN (...) constraint"

    def shouldBeApplied(self, profile, numRecords):
        ratio = _unique_value_ratio(profile)
        return ratio is not None and ratio <= 0.1  # (the reference's own threshold)

    def candidate(self, profile, numRecords):
        values = _by_popularity([kv for kv in profile.histogram.values.items() if kv[0] != NULL_FIELD_REPLACEMENT],
                                lambda v: v.absolute)
        sql, code = _categories(values)
        description = f"'{profile.column}' has value range {sql}"
        constraint = _named(Compliance(description, f"`{profile.column}` IN ({sql})"), _is_one, "ComplianceConstraint")
        return ConstraintSuggestion(constraint, profile.column, "Compliance: 1", description, self,
                                    f'.isContainedIn("{profile.column}", Array({code}))')


@dataclass(frozen=True)
class FractionalCategoricalRangeRule(ConstraintRule):  # rules/FractionalCategoricalRangeRule.scala:29-121
    targetDataCoverageFraction: float = 0.9
    ruleDescription = ("If we see a categorical range for most values in a column, we suggest an IS IN (...) "
                       "constraint that should hold for most values")

    def __str__(self):
        return f"FractionalCategoricalRangeRule({_d2s(float(self.targetDataCoverageFraction))})"

    def _top_categories(self, profile):
        """getTopCategoriesForFractionalDataCoverage (:98-116): by ratio descending (ties unpinned, see
        _by_popularity) until the coverage reaches the target."""
        coverage, out = 0.0, []
        for name, value in _by_popularity(profile.histogram.values.items(), lambda v: v.ratio):
            if coverage < self.targetDataCoverageFraction:
                coverage += value.ratio
                out.append((name, value))
        return out

    def shouldBeApplied(self, profile, numRecords):
        ratio = _unique_value_ratio(profile)
        if ratio is None:
            return False
        return ratio <= 0.4 and sum(v.ratio for _, v in self._top_categories(profile)) < 1

    def candidate(self, profile, numRecords):
        top = self._top_categories(profile)
        ratio_sums = float(sum(v.ratio for _, v in top))  # (NullValue's share included, as in the reference)
        values = _by_popularity([kv for kv in top if kv[0] != NULL_FIELD_REPLACEMENT], lambda v: v.absolute)
        sql, code = _categories(values)
        target = round_target(ratio_sums, numRecords)
        description = f"'{profile.column}' has value range {sql} for at least {_d2s(target * 100)}% of values"
        hint = f"It should be above {_d2s(target)}!"
        constraint = _named(Compliance(description, f"`{profile.column}` IN ({sql})"), lambda v: v >= target,
                            "ComplianceConstraint", None, hint)
        return ConstraintSuggestion(
            constraint, profile.column, "Compliance: " + _d2s(ratio_sums), description, self,
            f'.isContainedIn("{profile.column}", Array({code}), _ >= {_d2s(target)}, Some("{hint}"))')


class NonNegativeNumbersRule(ConstraintRule):  # rules/NonNegativeNumbersRule.scala:25-56
    ruleDescription = "If we see only non-negative numbers in a column, we suggest a corresponding constraint"

    def shouldBeApplied(self, profile, numRecords):
        return isinstance(profile, NumericColumnProfile) and profile.minimum is not None and profile.minimum >= 0.0

    def candidate(self, profile, numRecords):
        description = f"'{profile.column}' has no negative values"
        constraint = _named(Compliance(description, f"{profile.column} >= 0"), _is_one, "ComplianceConstraint")
        if isinstance(profile, NumericColumnProfile) and profile.minimum is not None:
            minimum = _d2s(float(profile.minimum))
        else:
            minimum = "Error while calculating minimum!"
        return ConstraintSuggestion(constraint, profile.column, "Minimum: " + minimum, description, self,
                                    f'.isNonNegative("{profile.column}")')


class UniqueIfApproximatelyUniqueRule(ConstraintRule):  # rules/UniqueIfApproximatelyUniqueRule.scala:29-55
    ruleDescription = ("If the ratio of approximate num distinct values in a column is close to the number of records "
                       "(within the error of the HLL sketch), we suggest a UNIQUE constraint")

    def shouldBeApplied(self, profile, numRecords):
        if numRecords == 0:  # (Long.toDouble / 0: NaN or Infinity, never within the bound)
            return False
        return profile.completeness == 1.0 and abs(1.0 - profile.approximateNumDistinctValues / numRecords) <= 0.08

    def candidate(self, profile, numRecords):
        constraint = _named(Uniqueness([profile.column]), _is_one, "UniquenessConstraint")
        distinctness = profile.approximateNumDistinctValues / numRecords
        return ConstraintSuggestion(constraint, profile.column, "ApproxDistinctness: " + _d2s(float(distinctness)),
                                    f"'{profile.column}' is unique", self, f'.isUnique("{profile.column}")')


class Rules:  # ConstraintSuggestionRunner.scala:29-35
    """DEFAULT is the reference's list (:31-34).  UniqueIfApproximatelyUniqueRule, the seventh rule, is not part of
    it there either: the reference's own runs add it with addConstraintRule."""
    DEFAULT: Sequence[ConstraintRule] = (CompleteIfCompleteRule(), RetainCompletenessRule(), RetainTypeRule(),
                                         CategoricalRangeRule(), FractionalCategoricalRangeRule(),
                                         NonNegativeNumbersRule())


@dataclass
class ConstraintSuggestion:  # ConstraintSuggestion.scala:27-34
    constraint: object
    columnName: str
    currentValue: str
    description: str
    suggestingRule: ConstraintRule
    codeForConstraint: str


class ConstraintSuggestions:  # ConstraintSuggestion.scala:36-114
    FIELD = "constraint_suggestions"

    @staticmethod
    def _shared(s: ConstraintSuggestion) -> Dict[str, str]:  # addSharedProperties (:98-112), in insertion order
        return {"constraint_name": str(s.constraint), "column_name": s.columnName, "current_value": s.currentValue,
                "description": s.description, "suggesting_rule": str(s.suggestingRule),
                "rule_description": s.suggestingRule.ruleDescription, "code_for_constraint": s.codeForConstraint}

    @staticmethod
    def toJson(constraintSuggestions: Sequence[ConstraintSuggestion]) -> str:  # :40-59
        return json.dumps({ConstraintSuggestions.FIELD: [ConstraintSuggestions._shared(s) for s in constraintSuggestions]},
                          indent=2)

    @staticmethod
    def evaluationResultsToJson(constraintSuggestions: Sequence[ConstraintSuggestion],
                                result: Optional[VerificationResult]) -> str:
        """:61-96: the first check's constraint results, in order, next to the suggestions; "Unknown" where there is
        no result (no train / test split)."""
        results = []
        if result is not None and result.checkResults:
            results = [r.status.name for r in next(iter(result.checkResults.values())).constraintResults]
        rows = []
        for i, s in enumerate(constraintSuggestions):
            row = ConstraintSuggestions._shared(s)
            row["constraint_result_on_test_set"] = results[i] if i < len(results) else "Unknown"
            rows.append(row)
        return json.dumps({ConstraintSuggestions.FIELD: rows}, indent=2)


column_profiles_to_json = ColumnProfiles.toJson  # profiles/ColumnProfile.scala:67-146


@dataclass
class ConstraintSuggestionResult:  # ConstraintSuggestionResult.scala:30-33
    columnProfiles: Dict[str, ColumnProfile]
    constraintSuggestions: Dict[str, List[ConstraintSuggestion]]
    verificationResult: Optional[VerificationResult] = None
    numRecords: int = 0               # the rows profiled (the training side when a split was used)
    splitSeed: Optional[int] = None   # the seed of the train / test split, None without one

    def _all(self) -> List[ConstraintSuggestion]:
        return [s for group in self.constraintSuggestions.values() for s in group]

    @staticmethod
    def getColumnProfilesAsJson(result: "ConstraintSuggestionResult") -> str:  # :37-40
        return column_profiles_to_json(list(result.columnProfiles.values()))

    @staticmethod
    def getConstraintSuggestionsAsJson(result: "ConstraintSuggestionResult") -> str:  # :42-46
        return ConstraintSuggestions.toJson(result._all())

    @staticmethod
    def getEvaluationResultsAsJson(result: "ConstraintSuggestionResult") -> str:  # :48-56
        return ConstraintSuggestions.evaluationResultsToJson(result._all(), result.verificationResult)


def _write_text(path: str, text: str, overwrite: bool) -> None:
    if os.path.exists(path) and not overwrite:
        raise FileExistsError(f"{path} exists and overwritePreviousFiles is not set")
    with open(path, "w", encoding="utf-8") as f:
        f.write(text + "\n")


_NO_REPOSITORY = "the metrics repository is not part of the GPU path"


class ConstraintSuggestionRunner:  # ConstraintSuggestionRunner.scala:56-315
    def onData(self, data) -> "ConstraintSuggestionRunBuilder":
        return ConstraintSuggestionRunBuilder(data)

    @staticmethod
    def applyRules(constraintRules: Sequence[ConstraintRule], profiles: ColumnProfiles,
                   columns: Sequence[str]) -> List[ConstraintSuggestion]:  # :193-208
        out = []
        for column in columns:
            profile = profiles.profiles[column]
            out += [r.candidate(profile, profiles.numRecords) for r in constraintRules
                    if r.shouldBeApplied(profile, profiles.numRecords)]
        return out

    @staticmethod
    def run(data, constraintRules, restrictToColumns=None,
            lowCardinalityHistogramThreshold=ColumnProfiler.DEFAULT_CARDINALITY_THRESHOLD, printStatusUpdates=False,
            testsetRatio=None, testsetSplitRandomSeed=None, saveColumnProfilesJsonToPath=None,
            saveConstraintSuggestionsJsonToPath=None, saveEvaluationResultsJsonToPath=None,
            overwriteResults=False) -> ConstraintSuggestionResult:  # :62-125
        if testsetRatio is not None:
            check_ratio(testsetRatio)
        data = arrow_data(data)
        if not isinstance(data, Table):
            data = list(data)
        training, test, seed = data, None, None
        if testsetRatio is not None:  # splitTrainTestSets (:127-148), on the device
            split = random_split(data, testsetRatio, testsetSplitRandomSeed)
            training, test, seed = split.train, split.test, split.seed

        # profileAndSuggest (:150-191)
        profiles = ColumnProfiler.profile(training, restrictToColumns=restrictToColumns,
                                          printStatusUpdates=printStatusUpdates,
                                          lowCardinalityHistogramThreshold=lowCardinalityHistogramThreshold)
        relevant = [name for name, _, _ in _chunks(training)[0].schema
                    if restrictToColumns is None or name in restrictToColumns]
        suggestions = ConstraintSuggestionRunner.applyRules(constraintRules, profiles, relevant)

        if saveColumnProfilesJsonToPath is not None:
            if printStatusUpdates:
                print(f"### WRITING COLUMN PROFILES TO {saveColumnProfilesJsonToPath}")
            _write_text(saveColumnProfilesJsonToPath, column_profiles_to_json(list(profiles.profiles.values())),
                        overwriteResults)
        if saveConstraintSuggestionsJsonToPath is not None:
            if printStatusUpdates:
                print(f"### WRITING CONSTRAINTS TO {saveConstraintSuggestionsJsonToPath}")
            _write_text(saveConstraintSuggestionsJsonToPath, ConstraintSuggestions.toJson(suggestions), overwriteResults)

        verification = None
        if test is not None:  # evaluateConstraintsIfNecessary (:283-313)
            if printStatusUpdates:
                print("### RUNNING EVALUATION")
            generated = Check(CheckLevel.Warning, "generated constraints", [s.constraint for s in suggestions])
            verification = VerificationSuite().onData(test).addCheck(generated).run()
            if saveEvaluationResultsJsonToPath is not None:
                if printStatusUpdates:
                    print(f"### WRITING EVALUATION RESULTS TO {saveEvaluationResultsJsonToPath}")
                _write_text(saveEvaluationResultsJsonToPath,
                            ConstraintSuggestions.evaluationResultsToJson(suggestions, verification), overwriteResults)

        by_column: Dict[str, List[ConstraintSuggestion]] = {}
        for s in suggestions:
            by_column.setdefault(s.columnName, []).append(s)
        return ConstraintSuggestionResult(profiles.profiles, by_column, verification, profiles.numRecords, seed)


class ConstraintSuggestionRunBuilder:  # ConstraintSuggestionRunBuilder.scala:27-293
    def __init__(self, data):
        self.data = arrow_data(data)
        self.constraintRules: List[ConstraintRule] = []
        self._printStatusUpdates = False
        self._testsetRatio: Optional[float] = None
        self._testsetSplitRandomSeed: Optional[int] = None
        self._restrictToColumns: Optional[List[str]] = None
        self._threshold = ColumnProfiler.DEFAULT_CARDINALITY_THRESHOLD
        self._profilesPath = self._suggestionsPath = self._evaluationPath = None
        self._overwrite = False

    def addConstraintRule(self, constraintRule: ConstraintRule) -> "ConstraintSuggestionRunBuilder":
        self.constraintRules.append(constraintRule)
        return self

    def addConstraintRules(self, constraintRules: Sequence[ConstraintRule]) -> "ConstraintSuggestionRunBuilder":
        self.constraintRules.extend(constraintRules)
        return self

    def printStatusUpdates(self, printStatusUpdates: bool) -> "ConstraintSuggestionRunBuilder":
        self._printStatusUpdates = printStatusUpdates
        return self

    def cacheInputs(self, cacheInputs: bool) -> "ConstraintSuggestionRunBuilder":
        return self  # (accepted and ignored: the data is already device-resident)

    def useTrainTestSplitWithTestsetRatio(self, testsetRatio: float,
                                          testsetSplitRandomSeed: Optional[int] = None) -> "ConstraintSuggestionRunBuilder":
        self._testsetRatio, self._testsetSplitRandomSeed = testsetRatio, testsetSplitRandomSeed
        return self

    def withLowCardinalityHistogramThreshold(self, lowCardinalityHistogramThreshold: int) -> "ConstraintSuggestionRunBuilder":
        self._threshold = lowCardinalityHistogramThreshold
        return self

    def restrictToColumns(self, restrictToColumns: Sequence[str]) -> "ConstraintSuggestionRunBuilder":
        self._restrictToColumns = list(restrictToColumns)
        return self

    def useRepository(self, metricsRepository):
        raise NotImplementedError(f"ConstraintSuggestionRunner: {_NO_REPOSITORY}")

    def reuseExistingResultsForKey(self, resultKey, failIfResultsMissing: bool = False):
        raise NotImplementedError(f"ConstraintSuggestionRunner: {_NO_REPOSITORY}")

    def saveOrAppendResult(self, resultKey):
        raise NotImplementedError(f"ConstraintSuggestionRunner: {_NO_REPOSITORY}")

    def useSparkSession(self, sparkSession) -> "ConstraintSuggestionRunBuilder":
        return self  # (the save options write to the local filesystem; no session is needed)

    def saveColumnProfilesJsonToPath(self, path: str) -> "ConstraintSuggestionRunBuilder":
        self._profilesPath = path
        return self

    def saveConstraintSuggestionsJsonToPath(self, path: str) -> "ConstraintSuggestionRunBuilder":
        self._suggestionsPath = path
        return self

    def saveEvaluationResultsJsonToPath(self, path: str) -> "ConstraintSuggestionRunBuilder":
        self._evaluationPath = path
        return self

    def overwritePreviousFiles(self, overwriteFiles: bool) -> "ConstraintSuggestionRunBuilder":
        self._overwrite = overwriteFiles
        return self

    def run(self) -> ConstraintSuggestionResult:
        return ConstraintSuggestionRunner.run(
            self.data, self.constraintRules, self._restrictToColumns, self._threshold, self._printStatusUpdates,
            self._testsetRatio, self._testsetSplitRandomSeed, self._profilesPath, self._suggestionsPath,
            self._evaluationPath, self._overwrite)
