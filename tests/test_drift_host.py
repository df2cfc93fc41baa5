"""Distribution drift without a device: the CPU reference (tests/drift_ref.py) against hand-computed cases, the
analyzer's construction errors, printing, identity and preconditions, the check, what a metrics repository keeps of
the analyzer, and the argument validation of the two C entries under ASan + UBSan (a stand-alone program).  The
references here are host stand-ins: a ReferenceDistribution whose table handle is never dereferenced."""
import math
import os
import subprocess

import numpy as np
import pytest

from deequ_amd import _lib as L
from deequ_amd import (AnalysisRunner, Bins, Check, CheckLevel, DistributionDistance, FileSystemMetricsRepository,
                       InMemoryMetricsRepository, InMemoryStateProvider, ReferenceDistribution, ResultKey, StoredDistribution, Uniqueness)
from deequ_amd.grouping import FreqTable
from deequ_amd.matching import _dtype_of
from deequ_amd.metrics import DoubleMetric, Entity, Success
from deequ_amd.runner import AnalyzerContext
from tests import drift_ref
from tests.conftest import ROOT


class HostReference(ReferenceDistribution):
    """A reference of given sizes over given type codes, without a device table."""

    def __init__(self, types, columns, num_groups, num_values, binning=None):
        self.table = FreqTable(None, types)
        self.columns = tuple(columns)
        self.dtypes = tuple(_dtype_of(t) for t in types)
        self.binning = binning
        self.num_groups, self.num_values = num_groups, num_values


R1 = HostReference([L.TYPE_I64], ["id"], 7, 100)
R2 = HostReference([L.TYPE_UTF8, L.TYPE_I32], ["country", "n"], 12, 3456)
BINS = Bins.edges([0.0, 1.0, 2.5])
RB = HostReference([L.TYPE_UTF8], ["amount"], 4, 90, BINS)
SCHEMA = [("cid", "i64", True), ("cid32", "i32", True), ("country", "large_utf8", True), ("code", "dict_utf8", True),
          ("n", "i32", True), ("amount", "f64", True), ("flag", "bool", True)]


# ---- the reference against hand-computed cases --------------------------------------------------------------------

def test_reference_two_three_group_tables():
    a = {("x",): 2, ("y",): 1, ("z",): 1}   # p = 1/2, 1/4, 1/4
    b = {("x",): 1, ("y",): 1, ("w",): 2}   # q = 1/4, 1/4, 0 | w: 1/2
    d = drift_ref.distances(a, b)
    assert d["linf"] == 0.5 and d["tv"] == 0.5  # |p - q| = 1/4, 0, 1/4, 1/2
    # x: 1/2 ln(4/3) + 1/4 ln(2/3); y: 0; z: 1/4 ln 2; w: 1/2 ln 2
    want = 0.5 * (0.5 * math.log(4 / 3) + 0.25 * math.log(2 / 3) + 0.75 * math.log(2))
    assert abs(d["js"] - want) < 1e-15
    assert (d["common"], d["only_a"], d["only_b"], d["count_only_a"], d["count_only_b"], d["union"]) == (2, 1, 1, 1, 2, 4)
    assert d["linf_groups"] == {(("w",), 1)}


def test_reference_disjoint_tables():
    a, b = {(1,): 3, (2,): 1}, {(3,): 1, (4,): 1, (5,): 2}
    d = drift_ref.distances(a, b)
    assert d["linf"] == 0.75 and d["tv"] == 1.0 and abs(d["js"] - math.log(2)) < 1e-15
    assert (d["common"], d["only_a"], d["only_b"], d["count_only_a"], d["count_only_b"]) == (0, 2, 3, 4, 4)


def test_reference_identical_tables():
    a = {(1,): 3, (2,): 1, (9,): 5}
    d = drift_ref.distances(a, {g: 2 * c for g, c in a.items()})  # the same distribution at another size
    assert (d["linf"], d["tv"], d["js"]) == (0.0, 0.0, 0.0)
    assert (d["common"], d["only_a"], d["only_b"]) == (3, 0, 0) and len(d["linf_groups"]) == 3


def test_reference_none_rows_and_float_groups():
    f = drift_ref.freq([1.5, None, float("nan"), float("nan"), -0.0, 0.0, (None,)])
    assert sorted(f.values()) == [1, 1, 1, 2]  # one NaN group of 2; -0.0 and 0.0 apart; the NULLs nowhere
    assert drift_ref.freq([("a", 1), ("a", None), ("a", 1)]) == {(b"a", 1): 2}


def test_reference_ks_cases():
    below, above = drift_ref.freq([-5, -3, -3, 0]), drift_ref.freq([1, 2, 2, 9])
    assert drift_ref.ks(below, above) == 1.0 and drift_ref.ks(above, below) == 1.0
    assert drift_ref.ks(below, below) == 0.0
    assert drift_ref.ks(below, {g: 3 * c for g, c in below.items()}) == 0.0
    # F_a: 1/4 at 1, 1/2 at 2, 1 at 3; F_b: 0, 1/2, 1/2 -> 1/2 at 3... and |1/4 - 0| at 1
    assert drift_ref.ks(drift_ref.freq([1, 2, 3, 3]), drift_ref.freq([2, 4])) == 0.5


def test_reference_ks_float_order():
    inf, nan = float("inf"), float("nan")
    order = [-inf, -1.0, -0.0, 0.0, 1.0, inf, nan]
    ranks = [drift_ref._float_rank(drift_ref.canon(v)[1], 64) for v in order]
    assert ranks == sorted(ranks) and len(set(ranks)) == 7
    ranks32 = [drift_ref._float_rank(drift_ref.canon(v, f32=True)[1], 32) for v in order]
    assert ranks32 == sorted(ranks32) and len(set(ranks32)) == 7
    # -0.0 lies immediately below 0.0: a holds -0.0 alone, b holds 0.0 alone -> at -0.0 F_a = 1, F_b = 0
    assert drift_ref.ks(drift_ref.freq([-0.0]), drift_ref.freq([0.0])) == 1.0
    # NaN is greatest: all of a at +inf, all of b at NaN
    assert drift_ref.ks(drift_ref.freq([inf, inf]), drift_ref.freq([nan])) == 1.0
    # -inf is least
    assert drift_ref.ks(drift_ref.freq([-inf, 0.0]), drift_ref.freq([-1e308, 0.0])) == 0.5


def test_tolerance_is_the_issues_bound():
    assert drift_ref.tolerance(0) == 16 * 2.0 ** -53 and drift_ref.tolerance(99) == 1600 * 2.0 ** -53


# ---- construction, printing, identity -------------------------------------------------------------------------------

def test_construction_errors():
    with pytest.raises(ValueError, match="method: one of linf, tv, js, ks"):
        DistributionDistance("cid", R1, method="psi")
    with pytest.raises(ValueError, match="takes no binning"):
        DistributionDistance("amount", RB, method="ks", binning=BINS)
    with pytest.raises(ValueError, match="one ordered column, got 2"):
        DistributionDistance(["country", "n"], R2, method="ks")
    with pytest.raises(ValueError, match="a binning is over one column"):
        DistributionDistance(["amount", "n"], RB, binning=BINS)
    with pytest.raises(TypeError, match="a Bins is needed"):
        DistributionDistance("amount", RB, binning=[0, 1])
    for m in ("linf", "tv", "js", "ks"):
        assert DistributionDistance("cid", R1, m).method == m


def test_str_and_equality():
    a = DistributionDistance("cid", R1)
    assert str(a) == "DistributionDistance(List(cid),linf,7 groups of 100 values)" and repr(a) == str(a)
    assert str(DistributionDistance(["country", "n"], R2, "js", where="n > 0")) == \
        "DistributionDistance(List(country, n),js,12 groups of 3456 values,Some(n > 0))"
    assert str(DistributionDistance("amount", RB, "tv", BINS, "flag")) == \
        f"DistributionDistance(List(amount),tv,4 groups of 90 values,{BINS},Some(flag))"
    b = DistributionDistance(["cid"], R1, "linf")
    assert a == b and hash(a) == hash(b)
    assert a != DistributionDistance("cid", R1, "tv") and a != DistributionDistance("cid", R1, where="n > 0")
    assert a != DistributionDistance("cid32", R1) and a != Uniqueness("cid")
    assert DistributionDistance("amount", RB, binning=BINS) != DistributionDistance("amount", RB, binning=Bins.edges([0, 1]))
    # another reference of the same size is another analyzer; a stored one of that size keys the same metrics
    assert a != DistributionDistance("cid", HostReference([L.TYPE_I64], ["id"], 7, 100))
    stored = DistributionDistance("cid", StoredDistribution(7, 100))
    assert a == stored and hash(a) == hash(stored)
    assert a != DistributionDistance("cid", StoredDistribution(7, 101))
    assert a != DistributionDistance("cid", StoredDistribution(8, 100))


def test_metric_naming_entity_and_routing():
    one, two = DistributionDistance("cid", R1), DistributionDistance(["country", "n"], R2, "tv")
    assert (one.name, one.instance, one.entity) == ("DistributionDistance", "cid", Entity.Column)
    assert (two.name, two.instance, two.entity) == ("DistributionDistance", "country,n", Entity.Mutlicolumn)
    # without a binning: an ordinary grouping analyzer the runner groups by (columns, where); with one: its own pass
    assert one.grouping and not one.direct and one.groupingColumns() == ["cid"]
    assert DistributionDistance("amount", RB, binning=BINS).direct
    f = one.toFailureMetric(ValueError("x"))
    assert (f.entity, f.name, f.instance, f.value.isFailure) == (Entity.Column, "DistributionDistance", "cid", True)
    empty = one.computeMetricFrom(None)
    assert empty.value.isFailure and "Empty state for analyzer DistributionDistance(List(cid),linf" in str(empty.value.failed)


def _first_failure(analyzer, schema=SCHEMA):
    from deequ_amd.analyzers import Preconditions

    return Preconditions.findFirstFailing(schema, analyzer.preconditions())


def test_preconditions_fail_before_any_launch():
    assert _first_failure(DistributionDistance("cid", R1)) is None
    assert _first_failure(DistributionDistance(["code", "n"], R2, "js")) is None  # dict_utf8 against utf8: strings
    assert _first_failure(DistributionDistance("cid", R1, "ks")) is None
    assert _first_failure(DistributionDistance("amount", RB, "tv", BINS)) is None
    e = _first_failure(DistributionDistance("nope", R1))
    assert type(e).__name__ == "NoSuchColumnException" and "nope" in str(e)
    e = _first_failure(DistributionDistance(["cid", "n"], R1))
    assert isinstance(e, ValueError) and "2 columns (cid, n) cannot be compared with a distribution over 1 (id)" in str(e)
    e = _first_failure(DistributionDistance("cid32", R1))
    assert type(e).__name__ == "WrongColumnTypeException"
    assert str(e) == ("Expected type of column cid32 to be i64, the type of column id of the reference distribution, "
                      "but found i32 instead! (no implicit widening: cast the column first)")
    e = _first_failure(DistributionDistance("flag", HostReference([L.TYPE_BOOL], ["f"], 2, 9), "ks"))
    assert type(e).__name__ == "WrongColumnTypeException" and "for method ks, but found bool" in str(e)
    # the binning: equal Bins on both sides, a numeric column
    e = _first_failure(DistributionDistance("amount", RB, "tv", Bins.edges([0.0, 1.0])))
    assert isinstance(e, ValueError) and "different bins" in str(e)
    e = _first_failure(DistributionDistance("amount", RB, "tv"))
    assert isinstance(e, ValueError) and "different bins" in str(e)
    e = _first_failure(DistributionDistance("country", RB, "tv", BINS))
    assert type(e).__name__ == "WrongColumnTypeException"
    e = _first_failure(DistributionDistance("cid", StoredDistribution(7, 100)))
    assert isinstance(e, ValueError) and "cannot run" in str(e)


def test_check_construction_where_and_row_level_skip():
    from deequ_amd.rowlevel import row_form

    check = Check(CheckLevel.Error, "feed").hasDistributionDistance("cid", R1, lambda v: v < 0.1)
    c = check.constraints[-1]
    assert str(c) == "DistributionDistanceConstraint(DistributionDistance(List(cid),linf,7 groups of 100 values))"
    filtered = check.where("n > 0")
    assert str(filtered.constraints[-1]) == \
        "DistributionDistanceConstraint(DistributionDistance(List(cid),linf,7 groups of 100 values,Some(n > 0)))"
    assert check.requiredAnalyzers() == [DistributionDistance("cid", R1)]
    assert filtered.requiredAnalyzers() == [DistributionDistance("cid", R1, where="n > 0")]
    js = Check(CheckLevel.Warning, "feed").hasDistributionDistance("amount", RB, lambda v: v < 0.2, method="js",
                                                                   binning=BINS, hint="h")
    assert js.requiredAnalyzers() == [DistributionDistance("amount", RB, "js", BINS)]
    assert js.constraints[-1].inner.hint == "h"
    a = DistributionDistance("cid", R1)
    ok = c.evaluate({a: DoubleMetric(Entity.Column, "DistributionDistance", "cid", Success(0.05))})
    bad = c.evaluate({a: DoubleMetric(Entity.Column, "DistributionDistance", "cid", Success(0.5))})
    assert ok.status.name == "Success" and bad.status.name == "Failure"
    assert row_form(c) == "DistributionDistance has no row-level form"


# ---- the metrics repository -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("analyzer", [
    DistributionDistance("cid", R1),
    DistributionDistance(["country", "n"], R2, "js", where="n > 0"),
    DistributionDistance("amount", RB, "tv", BINS),
    DistributionDistance("cid", R1, "ks", where="amount >= 1.5"),
], ids=["linf", "js-where", "tv-binned", "ks-where"])
def test_repository_round_trip_to_a_stored_distribution(analyzer, tmp_path):
    from deequ_amd.repository import deserialize_analyzer, serialize_analyzer

    node = serialize_analyzer(analyzer)
    assert node["analyzerName"] == "DistributionDistance" and node["columns"] == list(analyzer.columns)
    assert (node["method"], node["where"]) == (analyzer.method, analyzer.where)
    assert (node["numGroups"], node["numValues"]) == (analyzer.reference.num_groups, analyzer.reference.num_values)
    assert node["binning"] == (None if analyzer.binning is None else {"edges": [0.0, 1.0, 2.5], "labels": None})
    back = deserialize_analyzer(node)
    assert isinstance(back.reference, StoredDistribution) and back == analyzer and str(back) == str(analyzer)
    metric = DoubleMetric(analyzer.entity, "DistributionDistance", analyzer.instance, Success(0.125))
    for repo in (InMemoryMetricsRepository(), FileSystemMetricsRepository(str(tmp_path / "metrics.json"))):
        repo.save(ResultKey(1, {"run": "a"}), AnalyzerContext({analyzer: metric}))
        loaded = repo.loadByKey(ResultKey(1, {"run": "a"}))
        assert loaded.metric(analyzer).value.get() == 0.125  # the live analyzer finds the stored analyzer's metric
    (stored,) = FileSystemMetricsRepository(str(tmp_path / "metrics.json")).loadByKey(ResultKey(1, {"run": "a"})).metricMap
    assert isinstance(stored.reference, StoredDistribution) and stored == analyzer
    # it refuses to run: a Failure metric from its preconditions, before any data is looked at
    m = AnalysisRunner.runOnAggregatedStates(SCHEMA, [stored], [InMemoryStateProvider()]).metric(stored)
    assert m.value.isFailure and "cannot run" in str(m.value.failed)
    with pytest.raises(ValueError, match="cannot run"):
        stored.computeMetricFrom(object())


# ---- the C entries' argument checks ---------------------------------------------------------------------------------

def test_distance_argument_validation_sanitized(tmp_path):
    """tests/drift_args_check.cpp, a stand-alone program with its own main: NULL out / ks / defined and NULL tables,
    each returning before the device is touched and writing nothing.  The entries' host code is compiled into the
    program with the host sanitizers; the kernels' device code is compiled as usual and never runs."""
    csrc = os.path.join(ROOT, "deequ_amd", "csrc")
    exe = tmp_path / "drift_args_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-result",
                    "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                    "-I", csrc, "-o", str(exe), os.path.join(ROOT, "tests", "drift_args_check.cpp"),
                    os.path.join(csrc, "dq_dist.hip"), os.path.join(csrc, "dq_group.hip"),
                    os.path.join(csrc, "dq_prim.hip"), os.path.join(csrc, "dq_freq_image.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_numpy_is_the_reference_arithmetic():
    """The reference's linf is a float64 division and subtraction per group, nothing wider."""
    d = drift_ref.distances({(1,): 1, (2,): 2}, {(1,): 1, (2,): 6})
    assert d["linf"] == float(np.abs(np.float64(1) / np.float64(3) - np.float64(1) / np.float64(7)))
