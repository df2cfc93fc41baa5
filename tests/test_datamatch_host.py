"""Dataset match without a device: analyzer identity, printing and hashing, the three forms of compareColumns, the
check's constraint string, the preconditions over a bare schema (their text names the column and both types), what a
metrics repository keeps of the analyzer and its refusal to run, and the row-level planning.  The references here are
host stand-ins: a KeyedRows over a key set whose table handle is never dereferenced and a payload of bare schemas."""
import pytest

from deequ_amd import _lib as L
from deequ_amd import (AnalysisRunner, Check, CheckLevel, DatasetMatch, FileSystemMetricsRepository,
                       InMemoryMetricsRepository, InMemoryStateProvider, KeyedRows, NumMatchesAndCount, ResultKey)
from deequ_amd.grouping import FreqTable
from deequ_amd.matching import KeySet, StoredKeyedRows
from deequ_amd.metrics import DoubleMetric, Entity, Success
from deequ_amd.runner import AnalyzerContext


class HostKeySet(KeySet):
    def __init__(self, types, columns, num_keys):
        super().__init__(FreqTable(None, types), columns)
        self._n = num_keys

    @property
    def num_keys(self):
        return self._n


class HostColumn:
    def __init__(self, dtype):
        self.dtype = dtype


class HostPayload:
    def __init__(self, cols):
        self.columns = {n: HostColumn(dt) for n, dt in cols}
        self.num_rows = 0


REF = KeyedRows(HostKeySet([L.TYPE_I64], ["id"], 50),
                HostPayload([("amount", "f64"), ("name", "utf8"), ("price", "decimal(10,2)")]))
SCHEMA = [("cid", "i64", True), ("cid32", "i32", True), ("amount", "f64", True), ("amount32", "f32", True),
          ("name", "large_utf8", True), ("label", "dict_utf8", True), ("price", "decimal(10,2)", True),
          ("price3", "decimal(10,3)", True)]


def test_keyed_rows_describes_itself():
    assert (REF.num_keys, REF.key_columns, REF.columns) == (50, ("id",), ("amount", "name", "price"))
    assert REF.dtypes == ("f64", "utf8", "decimal(10,2)") and str(REF) == "50 keys"


def test_compare_columns_normalisation():
    assert DatasetMatch("cid", ["amount", "name"], REF).mapping == (("amount", "amount"), ("name", "name"))
    assert DatasetMatch("cid", "amount", REF).mapping == (("amount", "amount"),)
    assert DatasetMatch("cid", {"label": "name", "amount": "amount"}, REF).mapping == \
        (("label", "name"), ("amount", "amount"))
    assert DatasetMatch("cid", None, REF).mapping == (("amount", "amount"), ("name", "name"), ("price", "price"))
    a = DatasetMatch(["cid"], {"label": "name"}, REF)
    assert (a.keyColumns, a.compareColumns, a.groupingColumns()) == (["cid"], ["label"], ["cid", "label"])


def test_identity_str_and_hash():
    a, b = DatasetMatch("cid", ["amount"], REF), DatasetMatch(["cid"], {"amount": "amount"}, REF)
    assert a == b and hash(a) == hash(b)
    assert str(a) == "DatasetMatch(cid,amount,50 keys,None)"
    assert str(DatasetMatch("cid", {"label": "name", "amount": "amount"}, REF, "amount > 0")) == \
        "DatasetMatch(cid,label->name,amount,50 keys,Some(amount > 0))"
    assert a != DatasetMatch("cid", ["amount"], REF, "amount > 0")
    assert a != DatasetMatch("cid", ["amount", "name"], REF)
    assert a != DatasetMatch("cid", {"amount32": "amount"}, REF)
    assert a != DatasetMatch("cid32", ["amount"], REF)
    # another reference of the same size is another analyzer; a stored one of that size keys the same metrics
    other = KeyedRows(HostKeySet([L.TYPE_I64], ["id"], 50), HostPayload([("amount", "f64")]))
    assert a != DatasetMatch("cid", ["amount"], other)
    stored = DatasetMatch("cid", ["amount"], StoredKeyedRows(50))
    assert a == stored and hash(a) == hash(stored) and str(a) == str(stored)
    assert a != DatasetMatch("cid", ["amount"], StoredKeyedRows(51))
    assert (a.name, a.instance, a.entity) == ("DatasetMatch", "cid,amount", Entity.Mutlicolumn)
    m = a.computeMetricFrom(NumMatchesAndCount(3, 4))
    assert (m.entity, m.name, m.instance, m.value.get()) == (Entity.Mutlicolumn, "DatasetMatch", "cid,amount", 0.75)
    assert a.computeMetricFrom(None).value.isFailure  # the empty state
    assert a._lower_op() == L.OP_COMPLIANCE


def test_check_construction_and_printing():
    check = Check(CheckLevel.Error, "orders").doesDatasetMatch("cid", ["amount", "name"], REF)
    c = check.constraints[-1]
    assert str(c) == "DatasetMatchConstraint(DatasetMatch(cid,amount,name,50 keys,None))"
    filtered = check.where("amount > 0")
    assert str(filtered.constraints[-1]) == \
        "DatasetMatchConstraint(DatasetMatch(cid,amount,name,50 keys,Some(amount > 0)))"
    assert check.requiredAnalyzers() == [DatasetMatch("cid", ["amount", "name"], REF)]
    assert filtered.requiredAnalyzers() == [DatasetMatch("cid", ["amount", "name"], REF, "amount > 0")]
    hinted = Check(CheckLevel.Warning, "w").doesDatasetMatch("cid", None, REF, lambda v: v > 0.9, hint="h")
    assert hinted.constraints[-1].inner.hint == "h"
    a = DatasetMatch("cid", ["amount", "name"], REF)  # the default assertion is "== 1.0"
    ok = c.evaluate({a: DoubleMetric(Entity.Mutlicolumn, "DatasetMatch", a.instance, Success(1.0))})
    bad = c.evaluate({a: DoubleMetric(Entity.Mutlicolumn, "DatasetMatch", a.instance, Success(0.5))})
    assert ok.status.name == "Success" and bad.status.name == "Failure"


def _failure(analyzer, schema=SCHEMA):
    from deequ_amd.analyzers import Preconditions

    return Preconditions.findFirstFailing(schema, analyzer.preconditions())


def test_preconditions_over_a_bare_schema():
    assert _failure(DatasetMatch("cid", ["amount", "name", "price"], REF)) is None  # (name: the other offset width)
    assert _failure(DatasetMatch("cid", {"label": "name"}, REF)) is None            # (a dictionary-encoded column)
    assert _failure(DatasetMatch("cid", None, REF)) is None
    e = _failure(DatasetMatch("nope", ["amount"], REF))
    assert type(e).__name__ == "NoSuchColumnException" and str(e) == "Input data does not include column nope!"
    e = _failure(DatasetMatch("cid", ["nope"], REF))
    assert type(e).__name__ == "NoSuchColumnException" and "column nope" in str(e)
    e = _failure(DatasetMatch("cid", {"amount": "nope"}, REF))
    assert type(e).__name__ == "NoSuchColumnException" and "reference does not include column nope" in str(e)
    e = _failure(DatasetMatch("cid32", ["amount"], REF))
    assert type(e).__name__ == "WrongColumnTypeException"
    assert "column cid32 to be i64, the type of column id of the key set, but found i32" in str(e)
    e = _failure(DatasetMatch("cid", {"amount32": "amount"}, REF))
    assert type(e).__name__ == "WrongColumnTypeException"
    assert str(e) == ("Expected type of column amount32 to be f64, the type of column amount of the reference, but "
                      "found f32 instead! (no implicit widening: cast the column first)")
    e = _failure(DatasetMatch("cid", {"price3": "price"}, REF))
    assert "column price3 to be decimal(10,2), the type of column price of the reference, but found decimal(10,3)" in str(e)
    e = _failure(DatasetMatch(["cid", "cid32"], ["amount"], REF))
    assert str(e) == "2 columns (cid, cid32) cannot be matched with a key set over 1 (id)"
    e = _failure(DatasetMatch([], ["amount"], REF))
    assert str(e) == "At least one column needs to be specified!"
    e = _failure(DatasetMatch("cid", [], REF))
    assert str(e) == "a dataset match compares 1 to 16 columns, got 0"
    wide = KeyedRows(REF.key_set, HostPayload([(f"c{i}", "f64") for i in range(17)]))
    e = _failure(DatasetMatch("cid", None, wide), [("cid", "i64", True)] + [(f"c{i}", "f64", True) for i in range(17)])
    assert str(e) == "a dataset match compares 1 to 16 columns, got 17"
    # a precondition failure is a Failure metric, before anything is launched (no device in this process)
    from deequ_amd.table import Table

    class Schema(Table):
        def __init__(self):
            pass

        schema = SCHEMA

    a = DatasetMatch("cid", {"amount32": "amount"}, REF)
    m = a.calculate(Schema())
    assert m.value.isFailure and "found f32 instead" in str(m.value.failed)
    assert (m.name, m.instance) == ("DatasetMatch", "cid,amount32")
    ctx = AnalysisRunner.runOnAggregatedStates(SCHEMA, [a], [InMemoryStateProvider()])
    assert ctx.metric(a).value.isFailure and "found f32 instead" in str(ctx.metric(a).value.failed)


def test_states_sum():
    a = DatasetMatch("cid", ["amount"], REF)
    p1, p2 = InMemoryStateProvider(), InMemoryStateProvider()
    p1.persist(a, NumMatchesAndCount(3, 10))
    p2.persist(a, NumMatchesAndCount(4, 6))
    ctx = AnalysisRunner.runOnAggregatedStates(SCHEMA, [a], [p1, p2])
    assert ctx.metric(a).value.get() == 7 / 16


@pytest.mark.parametrize("kind", ["memory", "file"])
def test_repository_round_trip_and_refusal_to_run(kind, tmp_path):
    from deequ_amd.repository import deserialize_analyzer, serialize_analyzer

    a = DatasetMatch(["cid"], {"label": "name", "amount": "amount"}, REF, "amount > 0")
    node = serialize_analyzer(a)
    assert node == {"analyzerName": "DatasetMatch", "keyColumns": ["cid"],
                    "compareColumns": [["label", "name"], ["amount", "amount"]], "where": "amount > 0", "numKeys": 50}
    back = deserialize_analyzer(node)
    assert isinstance(back.reference, StoredKeyedRows) and back == a and str(back) == str(a) and hash(back) == hash(a)
    repo = InMemoryMetricsRepository() if kind == "memory" else FileSystemMetricsRepository(str(tmp_path / "m.json"))
    metric = DoubleMetric(Entity.Mutlicolumn, "DatasetMatch", a.instance, Success(0.875))
    key = ResultKey(1000, {"run": "a"})
    repo.save(key, AnalyzerContext({a: metric}))
    loaded = repo.loadByKey(key)
    assert loaded.metric(a).value.get() == 0.875  # the live analyzer keys the stored metric
    stored = next(iter(loaded.metricMap)) if kind == "file" else back
    e = _failure(stored)
    assert "was loaded from a metrics repository" in str(e) and "cannot run" in str(e)
    assert stored.calculate(object()).value.isFailure


def test_row_level_planning():
    from deequ_amd.rowlevel import plan_row_level, row_form

    ok = Check(CheckLevel.Error, "ok").doesDatasetMatch("cid", ["amount"], REF).where("amount > 0")
    f = row_form(ok.constraints[-1])
    assert (f.kind, f.columns, f.where) == ("contains", ("cid", "amount"), "amount > 0")
    assert f.analyzer == DatasetMatch("cid", ["amount"], REF, "amount > 0")
    bad_type = Check(CheckLevel.Error, "t").doesDatasetMatch("cid", {"amount32": "amount"}, REF)
    plan = plan_row_level([ok, bad_type], SCHEMA)
    assert list(plan.forms) == [str(ok.constraints[-1])] and not plan.programs
    assert plan.checks == [("ok", [str(ok.constraints[-1])]), ("t", [])]
    assert dict(plan.skipped)[str(bad_type.constraints[-1])].startswith("WrongColumnTypeException: ")
