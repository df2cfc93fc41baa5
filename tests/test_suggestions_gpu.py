"""Constraint suggestion on the device: dq_split_rows against its host twin bit for bit, chunk invariance of
random_split over every column layout, the reference's integration cases through the whole runner, a split run with
its evaluation, a constraint that fails on the test side, and the new Check methods through VerificationSuite."""
import json

import numpy as np
import pytest

from tests import split_ref as R
from tests.test_suggestions_host import KATS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd
    from deequ_amd import split, suggestions  # noqa: F401

    return deequ_amd


def bits_of(t, n):
    return np.unpackbits(t.cpu().numpy(), bitorder="little")[:n].astype(bool)


# 70001: several workgroups and a ragged last word; 524288 + 65: one row group past a full grid's stride of
# 2048 workgroups x 4 waves x 64 rows, so some waves take a second trip through the grid-stride loop
@pytest.mark.parametrize("row0", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 1000, 70001, 524288 + 65])
def test_split_rows_matches_host(dq, n_rows, row0):
    from deequ_amd.split import split_bitmaps, split_host

    seed, ratio = 42, 0.1
    b = split_bitmaps(n_rows, row0, seed, ratio)
    words = (n_rows + 63) // 64
    raw_train, raw_test = b.train.cpu().numpy(), b.test.cpu().numpy()
    assert len(raw_train) == len(raw_test) == (words + 1) * 8
    all_train = np.unpackbits(raw_train[:words * 8], bitorder="little").astype(bool)
    all_test = np.unpackbits(raw_test[:words * 8], bitorder="little").astype(bool)
    want = split_host(n_rows, row0, seed, ratio)
    assert np.array_equal(all_test[:n_rows], want)
    assert np.array_equal(all_train[:n_rows], ~want)             # complements over the rows
    assert not all_test[n_rows:].any() and not all_train[n_rows:].any()  # bits past n_rows are zero
    assert b.num_test == int(want.sum()) and b.num_train == n_rows - int(want.sum())
    assert b.num_test == int(all_test.sum()) and b.num_train == int(all_train.sum())


def test_split_rows_argument_checks(dq):
    import ctypes

    import torch

    from deequ_amd import _lib as L

    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    nt, ns = ctypes.c_int64(-1), ctypes.c_int64(-1)
    stream = torch.cuda.current_stream().cuda_stream

    def call(n, ratio, train=buf.data_ptr(), test=buf.data_ptr() + 32):
        return L.lib.dq_split_rows(n, 0, 0, ratio, train, test, torch.cuda.current_device(), stream, ctypes.byref(nt),
                                   ctypes.byref(ns))

    for ratio in (0.0, 1.0, float("nan")):
        assert call(8, ratio) == L.DQ_E_INVALID
    assert call(0, 0.5, None, None) == L.DQ_OK and (nt.value, ns.value) == (0, 0)
    assert call(8, 0.5, None, None) == L.DQ_E_INVALID
    assert not buf.cpu().numpy().any()  # nothing was written by any of these


def values_of(col):
    """A device column as Python values, None = NULL."""
    n = col.n_rows
    valid = np.ones(n, bool) if col.validity is None else bits_of(col.validity, n)
    raw = col.values.cpu().numpy()
    if col.dtype == "utf8":
        o = col.offsets.cpu().numpy().view(np.int32)[:n + 1]
        vals = [raw[o[i]:o[i + 1]].tobytes() for i in range(n)]
    elif col.dtype == "bool":
        vals = np.unpackbits(raw, bitorder="little")[:n].astype(bool).tolist()
    elif col.dtype == "f64":
        vals = raw[:8 * n].view(np.float64).tolist()
    elif col.dtype == "i64":
        vals = raw[:8 * n].view(np.int64).tolist()
    else:  # decimal: 16-byte unscaled values
        vals = [int.from_bytes(raw[16 * i:16 * i + 16].tobytes(), "little", signed=True) for i in range(n)]
    return [v if ok else None for v, ok in zip(vals, valid)]


def test_random_split_chunk_invariance(dq):
    from deequ_amd.split import random_split
    from deequ_amd.table import Table

    n, rng = 1000, np.random.default_rng(3)

    def rows(lo, hi):
        idx = range(lo, hi)
        return {"i": ("i64", [None if k % 11 == 0 else k * 7 - 300 for k in idx]),
                "f": ("f64", [None if k % 13 == 0 else k / 8.0 for k in idx]),
                "s": ("utf8", [None if k % 5 == 0 else "v" * (k % 9) + str(k) for k in idx]),
                "b": ("bool", [None if k % 17 == 0 else k % 3 == 0 for k in idx]),
                "d": ("decimal(20,2)", [None if k % 19 == 0 else (k - 500) * 10 ** 15 + k for k in idx])}

    whole = Table.from_pydict(rows(0, n))
    chunks = [Table.from_pydict(rows(0, 300)), Table.from_pydict(rows(300, 300)), Table.from_pydict(rows(300, n))]
    seed = int(rng.integers(0, 2 ** 62))
    one = random_split(whole, 0.3, seed)
    many = random_split(chunks, 0.3, seed)
    assert isinstance(one.train, Table) and [t.num_rows for t in many.train][1] == 0 and len(many.test) == 3
    want = np.array(R.split(n, 0, seed, 0.3))
    assert (one.numTrain, one.numTest) == (int((~want).sum()), int(want.sum())) == (many.numTrain, many.numTest)
    assert one.seed == many.seed == seed
    source = {name: values_of(c) for name, c in whole.columns.items()}
    for side, side_chunks, keep in (("train", many.train, ~want), ("test", many.test, want)):
        single = getattr(one, side)
        for name in whole.columns:
            got = values_of(single.columns[name])
            assert got == [v for v, k in zip(source[name], keep) if k], (side, name)
            assert got == [v for t in side_chunks for v in values_of(t.columns[name])], (side, name)
    train, test = random_split(whole, 0.3)  # no seed: one is drawn, and the result unpacks
    assert train.num_rows + test.num_rows == n


def integration_table(dq, n):
    rng = np.random.default_rng(0)
    cats = KATS["integration"]["categories"]
    m3 = rng.random(n)
    return dq.Table.from_pydict({
        "id": ("utf8", [f"id{i}" for i in range(n)]),
        "marketplace": ("utf8", [cats[k] for k in rng.integers(0, len(cats), n)]),
        "measurement": ("f64", rng.random(n).tolist()),
        "propertyA": ("utf8", ["true" if k else "false" for k in rng.integers(0, 2, n)]),
        "measurement2": ("utf8", [repr(float(k) - 0.5) for k in rng.integers(0, 100, n)]),
        "measurement3": ("utf8", [repr(float(v)) if v >= 0.5 else None for v in m3])})


def all_rules(S):
    return list(S.Rules.DEFAULT) + [S.UniqueIfApproximatelyUniqueRule()]


def test_integration_candidates(dq):
    from deequ_amd import suggestions as S

    kat = KATS["integration"]
    result = (S.ConstraintSuggestionRunner().onData(integration_table(dq, 1000)).addConstraintRules(S.Rules.DEFAULT)
              .addConstraintRule(S.UniqueIfApproximatelyUniqueRule()).run())
    assert result.verificationResult is None and result.splitSeed is None and result.numRecords == 1000
    assert list(result.columnProfiles) == ["id", "marketplace", "measurement", "propertyA", "measurement2", "measurement3"]
    for column, want in kat["expected"].items():
        got = result.constraintSuggestions.get(column, [])
        codes = [s.codeForConstraint for s in got]
        for code in want.get("present", []):
            assert code in codes, (column, code, codes)
        for prefix in want.get("present_prefixes", []):
            assert any(c.startswith(prefix) for c in codes), (column, prefix, codes)
        for prefix in want.get("absent_prefixes", []):
            assert not any(c.startswith(prefix) for c in codes), (column, prefix, codes)
        for prefix in want.get("description_prefixes", []):
            assert any(s.description.startswith(prefix) for s in got), (column, prefix)
        if "completeness_assertion" in want:
            (s,) = [s for s in got if s.codeForConstraint.startswith(".hasCompleteness(")]
            assert s.constraint.inner.assertion(want["completeness_assertion"]["holds_at"])
            assert not s.constraint.inner.assertion(want["completeness_assertion"]["fails_at"])
    (cat,) = [s for s in result.constraintSuggestions["marketplace"] if s.codeForConstraint.startswith(".isContainedIn(")]
    listed = cat.codeForConstraint[len('.isContainedIn("marketplace", Array('):-2].split(", ")
    assert set(listed) == {f'"{c}"' for c in kat["categories"]}  # (popularity order; ties unpinned)
    for case in kat["non_negativity"]:
        t = dq.Table.from_pydict({"some": (case["dtype"], case["values"])})
        r = S.ConstraintSuggestionRunner().onData(t).addConstraintRules([S.NonNegativeNumbersRule()]).run()
        assert len(r.constraintSuggestions) == case["num_suggestions"], case["source"]
        assert r.constraintSuggestions["some"][0].codeForConstraint == '.isNonNegative("some")'


def test_retain_type_with_completeness(dq):
    from deequ_amd import suggestions as S
    from deequ_amd.checks import Check, CheckLevel, CheckStatus, VerificationSuite

    kat = KATS["retain_type_with_completeness"]
    for values in (kat["complete"], kat["missing_at_least_one"]):
        t = dq.Table.from_pydict({kat["column"]: ("utf8", values)})
        r = S.ConstraintSuggestionRunner().onData(t).addConstraintRules(S.Rules.DEFAULT).run()
        (s,) = [s for s in r.constraintSuggestions[kat["column"]] if s.codeForConstraint.startswith(".hasDataType(")]
        assert s.codeForConstraint == kat["code"]
        v = VerificationSuite().onData(t).addCheck(Check(CheckLevel.Error, "retain type", [s.constraint])).run()
        assert v.status == CheckStatus.Success, kat["source"]


def split_table(dq, n, stray_rows=()):
    rng = np.random.default_rng(5)
    cats = ["DE", "NA", "IN", "EU"]
    cat = [cats[k] for k in rng.integers(0, 4, n)]
    for r in stray_rows:
        cat[r] = "ZZ"
    return dq.Table.from_pydict({
        "num": ("utf8", [str(i % 50 - 5) for i in range(n)]),  # (negatives: no non-negativity suggestion, see below)
        "cat": ("utf8", cat),
        "id": ("utf8", [f"id{i}" for i in range(n)]),
        "amount": ("f64", (rng.random(n) * 100).tolist())})


def test_split_run(dq, tmp_path):
    from deequ_amd import suggestions as S
    from deequ_amd.checks import CheckStatus

    n = 2000
    paths = [str(tmp_path / f"{k}.json") for k in ("profiles", "suggestions", "evaluation")]
    result = (S.ConstraintSuggestionRunner().onData(split_table(dq, n)).addConstraintRules(all_rules(S))
              .useTrainTestSplitWithTestsetRatio(0.1, 0).saveColumnProfilesJsonToPath(paths[0])
              .saveConstraintSuggestionsJsonToPath(paths[1]).saveEvaluationResultsJsonToPath(paths[2]).run())
    assert result.verificationResult is not None and result.splitSeed == 0
    (check_result,) = result.verificationResult.checkResults.values()
    for r in check_result.constraintResults:
        print(r)
    assert result.verificationResult.status == CheckStatus.Success
    assert check_result.status == CheckStatus.Success
    suggestions = [s for group in result.constraintSuggestions.values() for s in group]
    evaluation = json.loads(S.ConstraintSuggestionResult.getEvaluationResultsAsJson(result))["constraint_suggestions"]
    assert len(evaluation) == len(suggestions) == len(check_result.constraintResults) > 0
    assert [e["code_for_constraint"] for e in evaluation] == [s.codeForConstraint for s in suggestions]
    assert all(e["constraint_result_on_test_set"] == "Success" for e in evaluation)
    assert result.numRecords == n - sum(R.split(n, 0, 0, 0.1))
    codes = {s.codeForConstraint for s in suggestions}
    assert {'.isComplete("num")', '.hasDataType("num", ConstrainableDataTypes.Integral)', '.isComplete("cat")',
            '.isComplete("id")', '.isNonNegative("amount")'} <= codes
    assert any(c.startswith('.isContainedIn("cat", Array(') for c in codes)
    for p, key in zip(paths, ("columns", "constraint_suggestions", "constraint_suggestions")):
        with open(p) as f:
            assert json.load(f)[key]
    with pytest.raises(FileExistsError):  # overwritePreviousFiles is off
        (S.ConstraintSuggestionRunner().onData(split_table(dq, 100)).addConstraintRules(S.Rules.DEFAULT)
         .saveColumnProfilesJsonToPath(paths[0]).run())


def test_failure_on_test_side(dq):
    from deequ_amd import suggestions as S
    from deequ_amd.checks import CheckStatus, ConstraintStatus

    n = 2000
    is_test = R.split(n, 0, 0, 0.1)
    stray = [r for r in range(n) if is_test[r]][:5]  # a category only the test side sees
    result = (S.ConstraintSuggestionRunner().onData(split_table(dq, n, stray)).addConstraintRules(all_rules(S))
              .useTrainTestSplitWithTestsetRatio(0.1, 0).run())
    assert result.verificationResult.status == CheckStatus.Warning
    (check_result,) = result.verificationResult.checkResults.values()
    by_code = {s.codeForConstraint: r for s, r in zip(
        [s for group in result.constraintSuggestions.values() for s in group], check_result.constraintResults)}
    (code,) = [c for c in by_code if c.startswith('.isContainedIn("cat", Array(') and c.endswith("))") and "_ >=" not in c]
    assert '"ZZ"' not in code
    assert by_code[code].status == ConstraintStatus.Failure
    assert "does not meet the constraint requirement" in by_code[code].message
    assert by_code['.isComplete("cat")'].status == ConstraintStatus.Success
    evaluation = json.loads(S.ConstraintSuggestionResult.getEvaluationResultsAsJson(result))["constraint_suggestions"]
    assert {e["code_for_constraint"]: e["constraint_result_on_test_set"] for e in evaluation}[code] == "Failure"


def test_refused_condition_reports_failure(dq):
    """A category with a quote gives a condition with '' in it, and a non-negativity suggestion on a numeric string
    column compares a string column: the predicate compiler refuses both, and the evaluation reports those constraints
    as failures through the failure metric instead of raising."""
    from deequ_amd import suggestions as S
    from deequ_amd.checks import CheckStatus, ConstraintStatus

    n = 400
    t = dq.Table.from_pydict({"q": ("utf8", ["it's" if i % 2 else "plain" for i in range(n)]),
                              "num": ("utf8", [str(i % 7) for i in range(n)])})
    result = (S.ConstraintSuggestionRunner().onData(t).addConstraintRules(S.Rules.DEFAULT)
              .useTrainTestSplitWithTestsetRatio(0.5, 1).run())
    (check_result,) = result.verificationResult.checkResults.values()
    suggestions = [s for group in result.constraintSuggestions.values() for s in group]
    by_code = {s.codeForConstraint: r for s, r in zip(suggestions, check_result.constraintResults)}
    (code,) = [c for c in by_code if c.startswith('.isContainedIn("q", Array(') and "_ >=" not in c]
    assert '"it\'s"' in code and "'it''s'" in suggestions[[s.codeForConstraint for s in suggestions].index(code)].description
    quoted = by_code[code]
    assert quoted.status == ConstraintStatus.Failure and "outside the GPU-eligible set" in quoted.message
    assert by_code['.isNonNegative("num")'].status == ConstraintStatus.Failure
    assert by_code['.isComplete("q")'].status == ConstraintStatus.Success
    assert result.verificationResult.status == CheckStatus.Warning


def test_check_additions_through_verification_suite(dq):
    from deequ_amd.checks import (Check, CheckLevel, CheckStatus, ConstrainableDataTypes, ConstraintStatus,
                                  VerificationSuite)

    kat = KATS["check_additions"]
    table = dq.Table.from_pydict({k: ("utf8", v) for k, v in kat["unique_columns"].items() if k != "source"})
    ops = {"==": lambda x: (lambda v: v == x), "<": lambda x: (lambda v: v < x)}

    check = Check(CheckLevel.Error, "group-1")
    for c in kat["is_unique"]["columns"]:
        check = check.isUnique(c)
    result = VerificationSuite().onData(table).addCheck(check).run()
    assert result.status == CheckStatus[kat["is_unique"]["status"]]
    assert [r.status for r in result.checkResults[check].constraintResults] == \
        [ConstraintStatus[s] for s in kat["is_unique"]["constraint_statuses"]]

    check = Check(CheckLevel.Error, "group-1-u")
    for case in kat["has_uniqueness"]["cases"]:
        op, x = case["assertion"]
        cols = case["columns"]
        check = check.hasUniqueness(cols[0] if len(cols) == 1 else cols, ops[op](x))
    result = VerificationSuite().onData(table).addCheck(check).run()
    assert result.status == CheckStatus[kat["has_uniqueness"]["status"]]
    assert [r.status for r in result.checkResults[check].constraintResults] == \
        [ConstraintStatus[s] for s in kat["has_uniqueness"]["constraint_statuses"]]

    kt = kat["has_data_type"]
    t = dq.Table.from_pydict({kt["column"]: ("utf8", kt["values"])})
    op, x = kt["assertion"]
    check = Check(CheckLevel.Error, "some description").hasDataType(kt["column"], ConstrainableDataTypes[kt["dataType"]],
                                                                    ops[op](x))
    assert VerificationSuite().onData(t).addCheck(check).run().status == CheckStatus[kt["status"]]
    wrong = Check(CheckLevel.Error, "not all integral").hasDataType(kt["column"], ConstrainableDataTypes.Integral)
    assert VerificationSuite().onData(t).addCheck(wrong).run().status == CheckStatus.Error
