"""Referential integrity without a device: the check and its constraint (construction, printing, .where), the
analyzer's preconditions (their text names the column and both types), metric naming and entity, the
NumMatchesAndCount algebra the analyzer's states follow, the empty state, and what a metrics repository keeps of the
analyzer.  The key sets here are host stand-ins: a KeySet over a table handle that is never dereferenced."""
import pytest

from deequ_amd import _lib as L
from deequ_amd import (AnalysisRunner, Check, CheckLevel, Compliance, FileSystemMetricsRepository,
                       InMemoryMetricsRepository, InMemoryStateProvider, NumMatchesAndCount, ResultKey)
from deequ_amd.grouping import FreqTable
from deequ_amd.matching import KeySet, ReferentialIntegrity, StoredKeySet, types_match
from deequ_amd.metrics import DoubleMetric, Entity, Success
from deequ_amd.runner import AnalyzerContext


class HostKeySet(KeySet):
    """A key set of a given size over given type codes, without a device table."""

    def __init__(self, types, columns, num_keys):
        super().__init__(FreqTable(None, types), columns)
        self._n = num_keys

    @property
    def num_keys(self):
        return self._n


KS1 = HostKeySet([L.TYPE_I64], ["id"], 50)
KS2 = HostKeySet([L.TYPE_UTF8, L.decimal_type(10, 2)], ["country", "zip"], 1234)
SCHEMA = [("cid", "i64", True), ("cid32", "i32", True), ("country", "large_utf8", True), ("code", "dict_utf8", True),
          ("zip", "decimal(10,2)", True), ("zip3", "decimal(10,3)", True), ("amount", "f64", True)]


def test_key_set_describes_itself():
    assert (KS2.columns, KS2.dtypes, KS2.num_keys) == (("country", "zip"), ("utf8", "decimal(10,2)"), 1234)
    assert str(KS2) == "1234 keys"
    with pytest.raises(ValueError, match="2 columns, 1 names"):
        KeySet(FreqTable(None, [L.TYPE_I64, L.TYPE_I64]), ["a"])


def test_check_construction_and_printing():
    check = Check(CheckLevel.Error, "orders").hasReferentialIntegrity("cid", KS1)
    c = check.constraints[-1]
    assert str(c) == "ReferentialIntegrityConstraint(ReferentialIntegrity(cid,50 keys,None))"
    filtered = check.where("amount > 0")
    assert type(filtered) is Check and len(filtered.constraints) == 1
    assert str(filtered.constraints[-1]) == "ReferentialIntegrityConstraint(ReferentialIntegrity(cid,50 keys,Some(amount > 0)))"
    multi = Check(CheckLevel.Warning, "feed").hasReferentialIntegrity(["country", "zip"], KS2, lambda v: v > 0.9, hint="h")
    assert str(multi.constraints[-1]) == "ReferentialIntegrityConstraint(ReferentialIntegrity(country,zip,1234 keys,None))"
    assert multi.constraints[-1].inner.hint == "h"
    assert check.requiredAnalyzers() == [ReferentialIntegrity("cid", KS1)]
    assert filtered.requiredAnalyzers() == [ReferentialIntegrity(["cid"], KS1, "amount > 0")]
    # the default assertion is "== 1.0"
    a = ReferentialIntegrity("cid", KS1)
    ok = c.evaluate({a: DoubleMetric(Entity.Column, "ReferentialIntegrity", "cid", Success(1.0))})
    bad = c.evaluate({a: DoubleMetric(Entity.Column, "ReferentialIntegrity", "cid", Success(0.5))})
    assert ok.status.name == "Success" and bad.status.name == "Failure"
    assert bad.message == "Value: 0.5 does not meet the constraint requirement!"


def test_identity():
    a, b = ReferentialIntegrity("cid", KS1), ReferentialIntegrity(["cid"], KS1)
    assert a == b and hash(a) == hash(b)
    assert a != ReferentialIntegrity("cid", KS1, "amount > 0")
    assert a != ReferentialIntegrity("cid32", KS1)
    # another key set of the same size is another analyzer; a stored one of that size keys the same metrics
    assert a != ReferentialIntegrity("cid", HostKeySet([L.TYPE_I64], ["id"], 50))
    stored = ReferentialIntegrity("cid", StoredKeySet(50))
    assert a == stored and hash(a) == hash(stored)
    assert a != ReferentialIntegrity("cid", StoredKeySet(51))


def test_metric_naming_and_entity():
    one, two = ReferentialIntegrity("cid", KS1), ReferentialIntegrity(["country", "zip"], KS2)
    assert (one.name, one.instance, one.entity) == ("ReferentialIntegrity", "cid", Entity.Column)
    assert (two.name, two.instance, two.entity) == ("ReferentialIntegrity", "country,zip", Entity.Mutlicolumn)
    m = two.computeMetricFrom(NumMatchesAndCount(3, 4))
    assert (m.entity, m.name, m.instance, m.value.get()) == (Entity.Mutlicolumn, "ReferentialIntegrity", "country,zip", 0.75)
    f = one.toFailureMetric(ValueError("x"))
    assert (f.entity, f.name, f.instance, f.value.isFailure) == (Entity.Column, "ReferentialIntegrity", "cid", True)


def _failure(analyzer, schema=SCHEMA):
    from deequ_amd.analyzers import Preconditions

    return Preconditions.findFirstFailing(schema, analyzer.preconditions())


def test_types_match_rule():
    assert types_match("i64", "i64") and types_match("utf8", "large_utf8") and types_match("dict_utf8", "utf8")
    assert not types_match("i32", "i64") and not types_match("date32", "i32") and not types_match("timestamp", "i64")
    assert not types_match("decimal(10,3)", "decimal(10,2)") and not types_match("utf8", "i64")


def test_preconditions_name_column_and_types():
    assert _failure(ReferentialIntegrity("cid", KS1)) is None
    assert _failure(ReferentialIntegrity(["country", "zip"], KS2)) is None  # (the other offset width)
    assert _failure(ReferentialIntegrity(["code", "zip"], KS2)) is None     # (a dictionary-encoded column)
    e = _failure(ReferentialIntegrity("nope", KS1))
    assert type(e).__name__ == "NoSuchColumnException" and str(e) == "Input data does not include column nope!"
    e = _failure(ReferentialIntegrity("cid32", KS1))
    assert type(e).__name__ == "WrongColumnTypeException"
    assert str(e) == ("Expected type of column cid32 to be i64, the type of column id of the key set, but found i32 "
                      "instead! (no implicit widening: cast the column first)")
    e = _failure(ReferentialIntegrity(["country", "zip3"], KS2))
    assert "column zip3 to be decimal(10,2), the type of column zip of the key set, but found decimal(10,3)" in str(e)
    e = _failure(ReferentialIntegrity(["cid", "country"], KS1))
    assert str(e) == "2 columns (cid, country) cannot be matched with a key set over 1 (id)"
    e = _failure(ReferentialIntegrity([], KS1))
    assert str(e) == "At least one column needs to be specified!"
    # a precondition failure is a Failure metric, before anything is launched (no device in this process)
    from deequ_amd.table import Table

    class Schema(Table):  # the runner reads a table's schema before it touches a column
        def __init__(self):
            pass

        schema = SCHEMA

    a = ReferentialIntegrity("cid32", KS1)
    m = a.calculate(Schema())
    assert m.value.isFailure and "found i32 instead" in str(m.value.failed)
    assert (m.name, m.instance) == ("ReferentialIntegrity", "cid32")
    ctx = AnalysisRunner.runOnAggregatedStates(SCHEMA, [a], [InMemoryStateProvider()])
    assert ctx.metric(a).value.isFailure and "found i32 instead" in str(ctx.metric(a).value.failed)


def test_states_sum_as_compliance_does():
    a = ReferentialIntegrity("cid", KS1)
    like = Compliance("c", "cid >= 0")
    p1, p2 = InMemoryStateProvider(), InMemoryStateProvider()
    for an in (a, like):
        p1.persist(an, NumMatchesAndCount(3, 10))
        p2.persist(an, NumMatchesAndCount(4, 6))
    ctx = AnalysisRunner.runOnAggregatedStates(SCHEMA, [a, like], [p1, p2])
    assert ctx.metric(a).value.get() == ctx.metric(like).value.get() == 7 / 16
    assert NumMatchesAndCount(3, 10).sum(NumMatchesAndCount(4, 6)) == NumMatchesAndCount(7, 16)
    # calculateMetric: load, merge, persist, metric
    out = InMemoryStateProvider()
    m = a.calculateMetric(NumMatchesAndCount(1, 2), aggregateWith=p1, saveStatesWith=out)
    assert m.value.get() == 4 / 12 and out.load(a) == NumMatchesAndCount(4, 12)
    # the state's file image is Compliance's
    assert a._lower_op() == like._lower_op() == L.OP_COMPLIANCE


def test_state_files_round_trip(tmp_path):
    from deequ_amd import HdfsStateProvider

    a = ReferentialIntegrity(["country", "zip"], KS2, "amount > 0")
    p = HdfsStateProvider(str(tmp_path / "states"))
    p.persist(a, NumMatchesAndCount(5, 9))
    assert p.load(a) == NumMatchesAndCount(5, 9)
    assert a.loadStateAndComputeMetric(p).value.get() == 5 / 9


def test_empty_state_as_compliance():
    a, like = ReferentialIntegrity("cid", KS1), Compliance("c", "cid >= 0")
    ma, ml = a.computeMetricFrom(None), like.computeMetricFrom(None)
    assert ma.value.isFailure and ml.value.isFailure
    assert type(ma.value.failed) is type(ml.value.failed)
    assert str(ma.value.failed) == f"Empty state for analyzer {a}, all input values were NULL."
    # no state anywhere: the aggregated run gives the same failure for both
    ctx = AnalysisRunner.runOnAggregatedStates(SCHEMA, [a, like], [InMemoryStateProvider()])
    assert type(ctx.metric(a).value.failed) is type(ctx.metric(like).value.failed)
    # a denominator of 0 that did reach a state divides as Compliance's does
    assert str(a.computeMetricFrom(NumMatchesAndCount(0, 0)).value.get()) == \
        str(like.computeMetricFrom(NumMatchesAndCount(0, 0)).value.get()) == "nan"


@pytest.mark.parametrize("kind", ["memory", "file"])
def test_repository_keeps_columns_where_and_size(kind, tmp_path):
    from deequ_amd.repository import deserialize_analyzer, serialize_analyzer

    a = ReferentialIntegrity(["country", "zip"], KS2, "amount > 0")
    node = serialize_analyzer(a)
    assert node == {"analyzerName": "ReferentialIntegrity", "columns": ["country", "zip"], "where": "amount > 0",
                    "numKeys": 1234}
    back = deserialize_analyzer(node)
    assert isinstance(back.reference, StoredKeySet) and back == a and str(back) == str(a)
    repo = InMemoryMetricsRepository() if kind == "memory" else FileSystemMetricsRepository(str(tmp_path / "m.json"))
    metric = DoubleMetric(Entity.Mutlicolumn, "ReferentialIntegrity", "country,zip", Success(0.875))
    key = ResultKey(1000, {"run": "a"})
    repo.save(key, AnalyzerContext({a: metric}))
    loaded = repo.loadByKey(key)
    assert loaded.metric(a).value.get() == 0.875  # the live analyzer keys the stored metric
    got = repo.load().forAnalyzers([a]).get()
    assert len(got) == 1 and got[0].analyzerContext.metric(a).value.get() == 0.875
    # the analyzer that came back refuses to run, with the reason
    stored = next(iter(loaded.metricMap)) if kind == "file" else back
    e = _failure(stored)
    assert "was loaded from a metrics repository" in str(e) and "cannot run" in str(e)
    m = stored.calculate(object())
    assert m.value.isFailure


def test_row_level_planning():
    """The constraint has a row-level form; one whose preconditions fail, or whose `where` is outside the GPU
    grammar, is listed in `skipped` with the reason and leaves its check."""
    from deequ_amd.rowlevel import plan_row_level, row_form

    ok = Check(CheckLevel.Error, "ok").hasReferentialIntegrity("cid", KS1).where("amount > 0")
    f = row_form(ok.constraints[-1])
    assert (f.kind, f.columns, f.where, f.analyzer) == ("contains", ("cid",), "amount > 0",
                                                        ReferentialIntegrity("cid", KS1, "amount > 0"))
    bad_where = Check(CheckLevel.Error, "w").hasReferentialIntegrity("cid", KS1).where("upper(country) = 'X'")
    bad_type = Check(CheckLevel.Error, "t").hasReferentialIntegrity("cid32", KS1)
    plan = plan_row_level([ok, bad_where, bad_type], SCHEMA)
    assert list(plan.forms) == [str(ok.constraints[-1])] and not plan.programs
    assert plan.checks == [("ok", [str(ok.constraints[-1])]), ("w", []), ("t", [])]
    reasons = dict(plan.skipped)
    assert reasons[str(bad_where.constraints[-1])].startswith("UnsupportedPredicate: ")
    assert reasons[str(bad_type.constraints[-1])].startswith("WrongColumnTypeException: ")
    assert "found i32 instead" in reasons[str(bad_type.constraints[-1])]


def test_row_level_planning_with_an_arithmetic_where():
    """The `where` of the constraint may hold arithmetic, as any predicate: its derived column is planned with the
    predicates' (the same `where` on isComplete plans the same way), and the other constraints are planned too."""
    from deequ_amd.rowlevel import plan_row_level

    ref = Check(CheckLevel.Error, "ref").hasReferentialIntegrity("cid", KS1).where("amount * 2 > 0")
    other = Check(CheckLevel.Error, "other").isComplete("cid").where("amount * 2 > 0").isComplete("country")
    plan = plan_row_level([ref, other], SCHEMA)
    assert not plan.skipped
    assert plan.checks == [("ref", [str(ref.constraints[-1])]), ("other", [str(c) for c in other.constraints])]
    assert plan.forms[str(ref.constraints[-1])].kind == "contains"
    assert list(plan.expr_columns) == ["(`amount` * 2)"]
    assert plan.expr_columns["(`amount` * 2)"] in [c[0] for c in plan.schema]
    alone = plan_row_level([ref], SCHEMA)
    assert not alone.skipped and list(alone.expr_columns) == ["(`amount` * 2)"] and not alone.programs
