"""Constraint suggestion on the CPU: the rules against the reference's known answers (tests/golden/suggestion_kats.json),
the target rounding, the JSON shapes, the split's draw (dq_split_rows_host) against the plain-Python restatement
(tests/split_ref.py), and the value pickers and names of the new Check methods on hand-built metrics."""
import json
import os
from decimal import ROUND_DOWN, Decimal

import numpy as np
import pytest

from tests import split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_kats():
    with open(os.path.join(ROOT, "tests", "golden", "suggestion_kats.json")) as f:
        return json.load(f)


KATS = load_kats()


@pytest.fixture(scope="module")
def S():
    from deequ_amd import suggestions

    return suggestions


def make_profile(spec, minimum=None):
    from deequ_amd.metrics import Distribution, DistributionValue
    from deequ_amd.profiles import NumericColumnProfile, StandardColumnProfile

    column, completeness, distinct, dtype, inferred, hist = spec
    dist = None
    if hist is not None:
        values = KATS["histograms"][hist]
        dist = Distribution({k: DistributionValue(a, r) for k, (a, r) in values.items()}, numberOfBins=len(values))
    if minimum is not None:  # ConstraintRulesTest.scala:586-589
        return NumericColumnProfile(column, completeness, distinct, dtype, inferred, {}, dist, 10.0, 100.0, minimum,
                                    10000.0, 1.0, None)
    return StandardColumnProfile(column, completeness, distinct, dtype, inferred, {}, dist)


@pytest.mark.parametrize("table", KATS["should_be_applied"], ids=lambda t: t["rule"])
def test_should_be_applied(S, table):
    rule = getattr(S, table["rule"])()
    for case in table["cases"]:
        profile = make_profile(case["profile"], case.get("minimum"))
        assert rule.shouldBeApplied(profile, case["numRecords"]) is case["expected"], (table["source"], case)


@pytest.mark.parametrize("kat", KATS["candidates"], ids=lambda k: k["rule"])
def test_candidate_code(S, kat):
    rule = getattr(S, kat["rule"])()
    s = rule.candidate(make_profile(kat["profile"]), kat["numRecords"])
    assert s.codeForConstraint == kat["code"], kat["source"]
    assert s.columnName == kat["profile"][0] and s.suggestingRule is rule


def test_candidates_kind_value_description(S):
    from deequ_amd.analyzers import Completeness, Compliance, DataType
    from deequ_amd.checks import AnalysisBasedConstraint, NamedConstraint
    from deequ_amd.grouping import Uniqueness

    s = S.CompleteIfCompleteRule().candidate(make_profile(["att1", 1.0, 0, "String", False, None]), 100)
    assert (s.currentValue, s.description) == ("Completeness: 1.0", "'att1' is not null")
    assert isinstance(s.constraint, NamedConstraint) and s.constraint.inner.analyzer == Completeness("att1")
    assert s.constraint.inner.assertion(1.0) and not s.constraint.inner.assertion(0.99)
    assert str(s.constraint) == "CompletenessConstraint(Completeness(att1,None))"

    s = S.RetainCompletenessRule().candidate(make_profile(["att1", 0.5, 0, "String", False, None]), 100)
    assert (s.currentValue, s.description) == ("Completeness: 0.5", "'att1' has less than 60% missing values")
    assert s.constraint.inner.assertion(0.4) and not s.constraint.inner.assertion(0.39)

    s = S.RetainTypeRule().candidate(make_profile(["item", 1.0, 0, "Integral", True, None]), 100)
    assert (s.currentValue, s.description) == ("DataType: Integral", "'item' has type Integral")
    assert isinstance(s.constraint, AnalysisBasedConstraint) and s.constraint.analyzer == DataType("item")
    assert str(s.constraint) == "AnalysisBasedConstraint(DataType(item,None),<function1>,Some(<function1>),None)"

    s = S.CategoricalRangeRule().candidate(make_profile(["c", 1.0, 0, "String", False, "problematic2"]), 100)
    assert s.currentValue == "Compliance: 1"
    assert s.description == "'c' has value range '_b%%__', '''_[a_[]}!@'''"
    assert s.constraint.inner.analyzer == Compliance(s.description, "`c` IN ('_b%%__', '''_[a_[]}!@''')")

    s = S.FractionalCategoricalRangeRule().candidate(make_profile(["c", 1.0, 0, "String", False, "problematic3"]), 100)
    ratio_sums = 0.65 + 0.3
    assert s.currentValue == "Compliance: " + repr(ratio_sums)
    assert s.description == "'c' has value range '_b%%__', '''_[a_[]}!@''' for at least 90.0% of values"
    assert s.constraint.inner.hint == "It should be above 0.9!"
    assert s.constraint.inner.assertion(0.9) and not s.constraint.inner.assertion(0.89)

    s = S.NonNegativeNumbersRule().candidate(make_profile(["item", 1.0, 0, "Integral", False, None]), 100)
    assert s.currentValue == "Minimum: Error while calculating minimum!"  # (a profile that is not numeric)
    s = S.NonNegativeNumbersRule().candidate(make_profile(["item", 1.0, 0, "Integral", False, None], minimum=1.0), 100)
    assert (s.currentValue, s.description) == ("Minimum: 1.0", "'item' has no negative values")
    assert str(s.constraint) == "ComplianceConstraint(Compliance('item' has no negative values,item >= 0,None))"

    s = S.UniqueIfApproximatelyUniqueRule().candidate(make_profile(["item", 1.0, 95, "String", False, None]), 100)
    assert (s.currentValue, s.description) == ("ApproxDistinctness: 0.95", "'item' is unique")
    assert s.constraint.inner.analyzer == Uniqueness(["item"])
    assert str(s.constraint) == "UniquenessConstraint(Uniqueness(List(item)))"


def test_category_order_and_null_replacement(S):
    from deequ_amd.metrics import Distribution, DistributionValue
    from deequ_amd.profiles import StandardColumnProfile

    dist = Distribution({"b": DistributionValue(10, 0.25), "NullValue": DistributionValue(12, 0.3),
                         "a": DistributionValue(4, 0.1), "d": DistributionValue(4, 0.1), "c": DistributionValue(4, 0.1),
                         "it's": DistributionValue(6, 0.15)}, numberOfBins=6)
    s = S.CategoricalRangeRule().candidate(StandardColumnProfile("k", 0.7, 6, "String", False, {}, dist), 40)
    cats = s.codeForConstraint[len('.isContainedIn("k", Array('):-2].split(", ")
    assert cats[:2] == ['"b"', '"it\'s"'] and set(cats[2:]) == {'"a"', '"c"', '"d"'}  # (ties unpinned: a set)
    assert "NullValue" not in s.description and "'it''s'" in s.description
    assert S.escape_java('a"b\\c\né') == 'a\\"b\\\\c\\n\\u00E9'


def test_default_rules(S):
    assert [str(r) for r in S.Rules.DEFAULT] == [
        "CompleteIfCompleteRule()", "RetainCompletenessRule()", "RetainTypeRule()", "CategoricalRangeRule()",
        "FractionalCategoricalRangeRule(0.9)", "NonNegativeNumbersRule()"]  # ConstraintSuggestionRunner.scala:31-34
    for r in list(S.Rules.DEFAULT) + [S.UniqueIfApproximatelyUniqueRule()]:
        assert r.ruleDescription


def test_target_rounding(S):
    assert S.round_target(0.5, 100) == 0.4
    # p - 1.96 sigma = 0.21 - 0.5645... is negative: DOWN is toward zero, not toward -infinity
    assert S.round_target(0.21, 2) == -0.35
    # the shortest string of the double 0.29 is "0.29"; its exact binary value 0.28999999999999998... would give 0.28
    assert float(Decimal(0.29).quantize(Decimal("0.01"), rounding=ROUND_DOWN)) == 0.28
    assert S.round_down_2(0.29) == 0.29
    assert S.round_down_2(0.999) == 0.99 and S.round_down_2(-0.001) == 0.0


def suggestions_of_json_kat(S):
    order = {"att2": 0, "att1": 1, "item": 2}
    profiles = {"item": make_profile(["item", 1.0, 4, "Integral", True, None], minimum=1.0),
                "att1": make_profile(["att1", 1.0, 2, "String", True, None]),
                "att2": make_profile(["att2", 1.0, 2, "String", True, None])}
    from deequ_amd.profiles import ColumnProfiles

    rules = list(S.Rules.DEFAULT) + [S.UniqueIfApproximatelyUniqueRule()]
    # (att1 / att2 carry no histogram here: with 4 rows the reference's categorical rules do not fire either)
    return S.ConstraintSuggestionRunner.applyRules(rules, ColumnProfiles(profiles, 4), sorted(profiles, key=order.get))


def test_to_json(S):
    kat = KATS["json"]
    got = json.loads(S.ConstraintSuggestions.toJson(suggestions_of_json_kat(S)))
    assert got == {"constraint_suggestions": kat["suggestions"]}, kat["source"]
    assert all(list(row) == kat["key_order"] for row in got["constraint_suggestions"])


def test_evaluation_results_to_json(S):
    from deequ_amd.checks import (Check, CheckLevel, CheckResult, CheckStatus, ConstraintResult, ConstraintStatus,
                                  VerificationResult)

    kat = KATS["json"]
    suggestions = suggestions_of_json_kat(S)
    got = json.loads(S.ConstraintSuggestions.evaluationResultsToJson(suggestions, None))
    want = [dict(row, **{kat["evaluation_key"]: kat["without_split"]}) for row in kat["suggestions"]]
    assert got == {"constraint_suggestions": want}
    assert all(list(row) == kat["key_order"] + [kat["evaluation_key"]] for row in got["constraint_suggestions"])
    check = Check(CheckLevel.Warning, "generated constraints", [s.constraint for s in suggestions])
    statuses = [ConstraintStatus.Failure if i % 2 else ConstraintStatus.Success for i in range(len(suggestions))]
    result = VerificationResult(CheckStatus.Warning, {check: CheckResult(check, CheckStatus.Warning, [
        ConstraintResult(c, st) for c, st in zip(check.constraints, statuses)])}, {})
    got = json.loads(S.ConstraintSuggestions.evaluationResultsToJson(suggestions, result))
    assert [r[kat["evaluation_key"]] for r in got["constraint_suggestions"]] == [st.name for st in statuses]


def test_column_profiles_to_json(S):
    from deequ_amd.profiles import ColumnProfiles

    profiles = [make_profile(["item", 1.0, 4, "Integral", True, None], minimum=1.0),
                make_profile(["att1", 1.0, 2, "String", False, "fracNonSkewedActual"])]
    got = json.loads(ColumnProfiles.toJson(profiles))["columns"]
    assert list(got[0]) == ["column", "dataType", "isDataTypeInferred", "completeness", "approximateNumDistinctValues",
                            "mean", "maximum", "minimum", "sum", "stdDev", "approxPercentiles"]
    assert got[0]["isDataTypeInferred"] == "true" and got[0]["approxPercentiles"] == [] and got[0]["minimum"] == 1.0
    assert got[1]["histogram"] == [{"value": "Y", "count": 5, "ratio": 0.4}, {"value": "N", "count": 10, "ratio": 0.6}]
    assert "typeCounts" not in got[1] and "mean" not in got[1]


def test_builder_options(S):
    b = S.ConstraintSuggestionRunner().onData(None)
    assert b.cacheInputs(True) is b and b.addConstraintRules(S.Rules.DEFAULT) is b
    for call in (lambda: b.useRepository(object()), lambda: b.reuseExistingResultsForKey(0, True),
                 lambda: b.saveOrAppendResult(0)):
        with pytest.raises(NotImplementedError, match="the metrics repository is not part of the GPU path"):
            call()
    for ratio in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"Testset ratio must be in \]0, 1\["):
            S.ConstraintSuggestionRunner().onData(None).useTrainTestSplitWithTestsetRatio(ratio, 0).run()


# ---------------------------------------------------------------------------------------------------------- the split
SPLIT_SHAPES = [(1, 0), (63, 0), (64, 0), (65, 0), (1000, 0), (1000, 2 ** 32 + 5)]
SPLIT_SEEDS = [0, 42, 2 ** 63 + 1]
SPLIT_RATIOS = [0.1, 0.5, 0.999]


def test_ref_hash_formulations_agree():
    import struct

    for g in (0, 1, 2 ** 32 + 5, 2 ** 63 + 7):
        for seed in SPLIT_SEEDS:
            assert R.hash_row(g, seed) == R.xxh64_of_8_bytes(struct.pack("<Q", g), seed)


@pytest.mark.parametrize("n_rows,row0", SPLIT_SHAPES)
def test_split_host_matches_reference(n_rows, row0):
    from deequ_amd.split import split_host

    for seed in SPLIT_SEEDS:
        for ratio in SPLIT_RATIOS:
            got = split_host(n_rows, row0, seed, ratio)
            assert got.tolist() == R.split(n_rows, row0, seed, ratio), (n_rows, row0, seed, ratio)


def test_reference_is_bernoulli():
    # 5 standard deviations of Binomial(1e5, 0.1) (sigma = 94.9): a guard against a broken mantissa mapping
    n_test = sum(R.split(100000, 0, 0, 0.1))
    assert abs(n_test - 10000) <= 475, n_test


def test_split_host_argument_checks():
    import ctypes

    from deequ_amd import _lib as L

    out = np.zeros(8, np.uint8)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    for ratio in (0.0, 1.0, float("nan"), -0.1, 1.5):
        assert L.lib.dq_split_rows_host(8, 0, 0, ratio, ptr) == L.DQ_E_INVALID
    assert L.lib.dq_split_rows_host(-1, 0, 0, 0.5, ptr) == L.DQ_E_INVALID
    assert L.lib.dq_split_rows_host(8, -1, 0, 0.5, ptr) == L.DQ_E_INVALID
    assert L.lib.dq_split_rows_host(0, 0, 0, 0.5, None) == L.DQ_OK
    assert L.lib.dq_split_rows_host(8, 0, 0, 0.5, ptr) == L.DQ_OK


# ------------------------------------------------------------------------------------------- the new Check methods
def dtype_distribution(counts):
    from deequ_amd.metrics import Distribution, DistributionValue

    total = sum(counts.values())
    return Distribution({k: DistributionValue(v, v / total) for k, v in counts.items()}, numberOfBins=5)


def test_data_type_value_picker():
    from deequ_amd.checks import ConstrainableDataTypes as T
    from deequ_amd.checks import data_type_value_picker as pick

    d = dtype_distribution({"Unknown": 2, "Fractional": 1, "Integral": 3, "Boolean": 0, "String": 2})
    assert pick(T.Null)(d) == 2 / 8           # ratioTypes(ignoreUnknown = false)(Unknown): the stored ratio
    assert pick(T.Integral)(d) == 3 / 6       # Unknown left out of the denominator
    assert pick(T.Fractional)(d) == 1 / 6
    assert pick(T.Numeric)(d) == 1 / 6 + 3 / 6
    assert pick(T.Boolean)(d) == 0.0 and pick(T.String)(d) == 2 / 6
    only_null = dtype_distribution({"Unknown": 4, "Fractional": 0, "Integral": 0, "Boolean": 0, "String": 0})
    assert pick(T.Integral)(only_null) == 0.0 and pick(T.Numeric)(only_null) == 0.0 and pick(T.Null)(only_null) == 1.0
    assert [t.value for t in T] == [0, 1, 2, 3, 4, 5] and T.Numeric.name == "Numeric"


def test_new_check_methods_on_hand_built_metrics():
    from deequ_amd.analyzers import DataType
    from deequ_amd.checks import Check, CheckLevel, CheckStatus, ConstrainableDataTypes, ConstraintStatus
    from deequ_amd.grouping import (Distinctness, Entropy, Histogram, MutualInformation, Uniqueness, UniqueValueRatio)
    from deequ_amd.metrics import DoubleMetric, Entity, HistogramMetric, Success
    from deequ_amd.runner import AnalyzerContext

    def dm(a, v):
        return DoubleMetric(a.entity, a.name, a.instance, Success(v))

    hist = dtype_distribution({"x": 3, "y": 1})
    metrics = {Uniqueness(["a"]): dm(Uniqueness(["a"]), 1.0), Uniqueness(["a", "b"]): dm(Uniqueness(["a", "b"]), 0.5),
               Distinctness(["a"]): dm(Distinctness(["a"]), 0.75), UniqueValueRatio(["a"]): dm(UniqueValueRatio(["a"]), 0.25),
               Entropy("a"): dm(Entropy("a"), 0.6), MutualInformation("a", "b"): dm(MutualInformation("a", "b"), 0.1),
               Histogram("a"): HistogramMetric("a", Success(hist)),
               DataType("s"): HistogramMetric("s", Success(dtype_distribution(
                   {"Unknown": 0, "Fractional": 1, "Integral": 1, "Boolean": 0, "String": 0})))}
    check = (Check(CheckLevel.Error, "new methods")
             .isUnique("a").hasUniqueness(["a", "b"], lambda v: v == 0.5).hasUniqueness("a", lambda v: v == 1.0)
             .hasDistinctness(["a"], lambda v: v == 0.75).hasUniqueValueRatio(["a"], lambda v: v == 0.25)
             .hasNumberOfDistinctValues("a", lambda v: v == 5).hasHistogramValues("a", lambda d: d.values["x"].ratio == 0.75)
             .hasEntropy("a", lambda v: v == 0.6).hasMutualInformation("a", "b", lambda v: v == 0.1)
             .hasDataType("s", ConstrainableDataTypes.Integral, lambda v: v == 0.5)
             .hasDataType("s", ConstrainableDataTypes.Numeric).isPrimaryKey("a", "b"))
    assert [str(c) for c in check.constraints] == [
        "UniquenessConstraint(Uniqueness(List(a)))", "UniquenessConstraint(Uniqueness(List(a, b)))",
        "UniquenessConstraint(Uniqueness(List(a)))", "DistinctnessConstraint(Distinctness(List(a)))",
        "UniqueValueRatioConstraint(UniqueValueRatio(List(a))",  # (Constraint.scala:254: the open parenthesis)
        "HistogramBinConstraint(Histogram(a,None,1000))", "HistogramConstraint(Histogram(a,None,1000))",
        "EntropyConstraint(Entropy(a))", "MutualInformationConstraint(MutualInformation(List(a, b)))",
        "AnalysisBasedConstraint(DataType(s,None),<function1>,Some(<function1>),None)",
        "AnalysisBasedConstraint(DataType(s,None),<function1>,Some(<function1>),None)",
        "UniquenessConstraint(Uniqueness(List(a, b)))"]
    assert set(check.requiredAnalyzers()) == set(metrics)
    result = check.evaluate(AnalyzerContext(metrics))
    statuses = [r.status for r in result.constraintResults]
    assert statuses[:-1] == [ConstraintStatus.Success] * 11 and statuses[-1] == ConstraintStatus.Failure
    assert result.status == CheckStatus.Error
    assert result.constraintResults[-1].message == "Value: 0.5 does not meet the constraint requirement!"
    hinted = Check(CheckLevel.Warning, "hint").isUnique("a", hint="keys repeat").evaluate(
        AnalyzerContext({Uniqueness(["a"]): dm(Uniqueness(["a"]), 0.5)}))
    assert hinted.status == CheckStatus.Warning
    assert hinted.constraintResults[0].message == "Value: 0.5 does not meet the constraint requirement! keys repeat"
    assert Check(CheckLevel.Error, "d", []).constraints == []
