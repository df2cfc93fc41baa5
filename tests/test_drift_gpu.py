"""Distribution drift on the device: dq_freq_distance / dq_freq_ks, drift.ReferenceDistribution / DistributionDistance,
Check.hasDistributionDistance and breakdown(), against the independent CPU reference tests/drift_ref.py.

linf, ks and every integer count must be bit-equal to the reference.  tv and js are sums of G terms (G = the size of
the groups' union) and must lie within 16 (G + 1) 2^-53 of the reference's math.fsum: about 8 roundings per term on a
magnitude <= max(p, q), non-negative terms, and a summation error of at most G 2^-53 times a total <= 2 -- assuming
the device's log stays within 2 ulp."""
import decimal
import math

import numpy as np
import pytest

from tests import drift_ref

pytestmark = pytest.mark.gpu

WG = 256            # kDistThreads in deequ_amd/csrc/dq_dist.hip: groups per workgroup and grid-loop step
BIG = 2 ** 17 + 3   # > kDistMaxGrid (1024) workgroups' worth of items: the grid loop runs and 1024 partials merge


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd
    from deequ_amd import drift  # noqa: F401

    return deequ_amd


def table(data):
    """Table.from_pydict; a numpy array becomes a column directly (the large cases)."""
    from deequ_amd.table import Table, column_from_numpy

    cols = []
    for name, (dtype, vals) in data.items():
        if isinstance(vals, np.ndarray):
            cols.append(column_from_numpy(name, dtype, vals))
        else:
            cols.append(Table.from_pydict({name: (dtype, list(vals))}).columns[name])
    return Table(cols)


def rows_table(names, dtypes, rows):
    return table({nm: (dt, [r[c] for r in rows]) for c, (nm, dt) in enumerate(zip(names, dtypes))})


def reference(names, dtypes, rows, **kw):
    from deequ_amd.drift import ReferenceDistribution

    return ReferenceDistribution.from_data(rows_table(names, dtypes, rows), list(names), **kw)


def canon_group(group, f32=False):
    return tuple(drift_ref.canon(v, f32) for v in group)


def check_breakdown(b, want, f32=False, group_canon=None):
    """A breakdown() dict against drift_ref.distances: bits for linf and the counts, the bound for tv and js."""
    tol = drift_ref.tolerance(want["union"])
    print(f"G={want['union']} linf={b['linf']!r} tv_err={abs(b['tv'] - want['tv']):.3e} "
          f"js_err={abs(b['js'] - want['js']):.3e} tol={tol:.3e}")
    assert b["linf"] == want["linf"]
    assert (b["common"], b["only_data"], b["only_reference"]) == (want["common"], want["only_a"], want["only_b"])
    assert abs(b["tv"] - want["tv"]) <= tol and abs(b["js"] - want["js"]) <= tol
    assert 0.0 <= b["js"] <= math.log(2)
    got = group_canon(b["linf_group"]) if group_canon else canon_group(b["linf_group"], f32)
    assert got in {g for g, _ in want["linf_groups"]}
    return b


def compare(dq, names, dtypes, rows_a, rows_b, f32=False, ref_dtypes=None, group_canon=None):
    """The analyzer (three methods in one run), the check and breakdown over (rows_a, reference of rows_b)."""
    from deequ_amd import AnalysisRunner, Check, CheckLevel, DistributionDistance, VerificationSuite

    ta = rows_table(names, dtypes, rows_a)
    ref = reference(names, ref_dtypes or dtypes, rows_b)
    fa, fb = drift_ref.freq(rows_a, f32), drift_ref.freq(rows_b, f32)
    assert (ref.num_groups, ref.num_values) == (len(fb), sum(fb.values()))
    want = drift_ref.distances(fa, fb)
    b = check_breakdown(DistributionDistance(list(names), ref).breakdown(ta), want, f32, group_canon)
    assert b["mass_only_data"] == want["count_only_a"] / sum(fa.values())
    assert b["mass_only_reference"] == want["count_only_b"] / sum(fb.values())
    analyzers = [DistributionDistance(list(names), ref, m) for m in ("linf", "tv", "js")]
    ctx = AnalysisRunner.doAnalysisRun(ta, analyzers)
    got = [ctx.metric(a).value.get() for a in analyzers]
    assert got == [b["linf"], b["tv"], b["js"]]  # the same tables, the same launch shape: the same bits
    check = Check(CheckLevel.Error, "drift").hasDistributionDistance(list(names), ref, lambda v: v == want["linf"])
    assert VerificationSuite().onData(ta).addCheck(check).run().status.name == "Success"
    return b, want


# ---- group counts and key relations (unhashed i64 keys, negative ones among them) --------------------------------------

def relation_keys(rel, g):
    """(a's keys, b's keys): g groups on a's side (and about as many on b's), around zero."""
    lo = -(g // 2)
    a = np.arange(lo, lo + g, dtype=np.int64)
    if rel in ("identical", "same_keys"):
        return a, a.copy()
    if rel == "disjoint":
        return a, a + g
    if rel == "a_in_b":
        return a, np.arange(lo - 3, lo + g + max(1, g // 2), dtype=np.int64)
    if rel == "b_in_a":
        return a, a[::2] if g > 1 else a.copy()
    if rel == "interleaved":
        return a * 2, a * 3
    odd, even = np.arange(1, 2 * g - 1, 2, dtype=np.int64), np.arange(2, 2 * g, 2, dtype=np.int64)  # g - 1 keys each
    if rel == "common_first":  # one common group, the smallest key word: 0
        return np.concatenate([[0], odd]).astype(np.int64), np.concatenate([[0], even]).astype(np.int64)
    if rel == "common_last":   # one common group, the largest key word: -1, as unsigned
        return np.concatenate([odd, [-1]]).astype(np.int64), np.concatenate([even, [-1]]).astype(np.int64)
    raise AssertionError(rel)


def rows_of(keys, seed):
    """Every key 1..4 times, shuffled: a column of values."""
    rng = np.random.default_rng(seed)
    v = np.repeat(keys, rng.integers(1, 5, len(keys)))
    rng.shuffle(v)
    return v


def freq_of_array(v):
    k, c = np.unique(v, return_counts=True)
    return {(int(x),): int(n) for x, n in zip(k, c)}


RELATIONS = ("identical", "same_keys", "disjoint", "a_in_b", "b_in_a", "interleaved", "common_first", "common_last")


@pytest.mark.parametrize("g", [1, 63, 64, 65, WG - 1, WG, WG + 1])
def test_group_counts_and_key_relations(dq, g):
    from deequ_amd.drift import DistributionDistance, ReferenceDistribution

    for rel in RELATIONS:
        ka, kb = relation_keys(rel, g)
        va, vb = rows_of(ka, 1), rows_of(kb, 1 if rel == "identical" else 2)  # identical: the same table
        fa, fb = freq_of_array(va), freq_of_array(vb)
        want = drift_ref.distances(fa, fb)
        if rel == "identical":
            assert (want["linf"], want["tv"], want["js"]) == (0.0, 0.0, 0.0)
        if rel in ("common_first", "common_last"):
            assert want["common"] == 1
        ref = ReferenceDistribution.from_data(table({"c": ("i64", vb)}), "c")
        b = check_breakdown(DistributionDistance("c", ref).breakdown(table({"c": ("i64", va)})), want)
        # the tie rule: the smallest unsigned key word among the groups attaining linf, a group of both on side a
        ties = sorted((g0[0] % 2 ** 64, side) for g0, side in want["linf_groups"])
        assert b["linf_group"] == ((ties[0][0] + 2 ** 63) % 2 ** 64 - 2 ** 63,), rel
        assert b["mass_only_data"] == want["count_only_a"] / sum(fa.values())
        assert b["mass_only_reference"] == want["count_only_b"] / sum(fb.values())


@pytest.fixture(scope="module")
def big(dq):
    """2^17 + 3 groups per side, interleaved (a: multiples of 2, b: of 3, around zero): the state, the reference
    object and the reference result, computed once."""
    from deequ_amd.drift import ReferenceDistribution
    from deequ_amd.grouping import build_frequencies

    k = np.arange(-(BIG // 2), BIG - BIG // 2, dtype=np.int64)
    va, vb = rows_of(k * 2, 3), rows_of(k * 3, 4)
    ta = table({"c": ("i64", va)})
    ref = ReferenceDistribution.from_data(table({"c": ("i64", vb)}), "c")
    return {"ta": ta, "ref": ref, "state": build_frequencies(ta, ["c"]), "fa": freq_of_array(va),
            "fb": freq_of_array(vb)}


def test_many_workgroup_partials(dq, big):
    from deequ_amd.drift import DistributionDistance

    want = drift_ref.distances(big["fa"], big["fb"])
    assert want["union"] > 2 * BIG - BIG // 2
    check_breakdown(DistributionDistance("c", big["ref"]).breakdown(big["ta"]), want)


def test_two_calls_return_identical_bits(dq, big):
    from deequ_amd.drift import freq_distance

    r1 = freq_distance(big["state"].frequencies, big["ref"].table)
    r2 = freq_distance(big["state"].frequencies, big["ref"].table)
    as_bits = lambda r: [np.float64(v).view(np.uint64) for v in (r.linf, r.tv, r.js)]  # noqa: E731
    assert as_bits(r1) == as_bits(r2)
    assert (r1.linf_key, r1.linf_side, r1.n_common) == (r2.linf_key, r2.linf_side, r2.n_common)


# ---- hashed tables ------------------------------------------------------------------------------------------------------

def test_string_column_with_empty_and_long_values(dq):
    long = "L" * 300
    rows_a = [("",), ("",), (long,), ("a",), ("b",), (None,), ("żółć",), ("a",)]
    rows_b = [("",), (long,), (long,), ("b",), ("c",), ("żółć",), (None,)]
    b, want = compare(dq, ["s"], ["utf8"], rows_a, rows_b)
    assert (want["common"], want["only_a"], want["only_b"]) == (4, 1, 1)


def test_utf8_data_against_large_utf8_reference(dq):
    rows_a = [(w,) for w in ["x", "y", "y", "z" * 40, ""]]
    rows_b = [(w,) for w in ["x", "x", "y", "w", ""]]
    compare(dq, ["s"], ["utf8"], rows_a, rows_b, ref_dtypes=["large_utf8"])
    compare(dq, ["s"], ["large_utf8"], rows_a, rows_b, ref_dtypes=["utf8"])


def test_two_column_tuple(dq):
    rows_a = [("a", 1), ("a", 2), ("a", 1), ("b", 1), (None, 1), ("b", None), ("", -5)]
    rows_b = [("a", 1), ("b", 1), ("b", 1), ("b", 2), ("", -5), ("", -5)]
    b, want = compare(dq, ["s", "n"], ["utf8", "i32"], rows_a, rows_b)
    assert (want["common"], want["only_a"], want["only_b"]) == (3, 1, 1)


def test_decimal_column(dq):
    d = lambda s: decimal.Decimal(s)  # noqa: E731
    rows_a = [(d("1.50"),), (d("1.50"),), (d("-123456789012345678.25"),), (d("0.00"),), (None,)]
    rows_b = [(d("1.50"),), (d("-123456789012345678.25"),), (d("-123456789012345678.25"),), (d("7.01"),)]
    b, want = compare(dq, ["d"], ["decimal(20,2)"], rows_a, rows_b)
    assert (want["common"], want["only_a"], want["only_b"]) == (2, 1, 1)


def test_equal_hash_different_value_is_two_groups(dq):
    """The forged image of tests/test_refint_gpu.py: a reference group keeps the hash of "value-a" and stores
    "value-b".  Against data holding "value-a" the hash is found, the tuples differ: one group only in the data and one
    only in the reference, never a common one, and no collision error."""
    from deequ_amd.drift import DistributionDistance, ReferenceDistribution

    vals = ["value-a", "other-1", "other-2", "other-3"]
    ta = table({"s": ("utf8", vals + ["value-a"])})
    good = ReferenceDistribution.from_data(table({"s": ("utf8", vals)}), "s")
    image = good.to_bytes()
    assert image.count(b"value-a") == 1
    forged = ReferenceDistribution.from_bytes(image.replace(b"value-a", b"value-b"), ["s"])
    assert DistributionDistance("s", good).breakdown(ta)["common"] == 4
    b = DistributionDistance("s", forged).breakdown(ta)
    assert (b["common"], b["only_data"], b["only_reference"]) == (3, 1, 1)
    fa = drift_ref.freq(vals + ["value-a"])
    fb = drift_ref.freq(["value-b", "other-1", "other-2", "other-3"])
    check_breakdown(b, drift_ref.distances(fa, fb))
    assert b["linf_group"] == ("value-a",)  # 2/5 against 0: the data's side holds it
    assert (b["mass_only_data"], b["mass_only_reference"]) == (2 / 5, 1 / 4)


# ---- KS -----------------------------------------------------------------------------------------------------------------

INF, NAN = float("inf"), float("nan")
KS_CASES = {
    "i64_negatives": ("i64", [-2 ** 63, -5, -5, -1, 0, 3, 2 ** 63 - 1, None], [-7, -5, 0, 0, 1, 2 ** 63 - 1]),
    "i8": ("i8", [-128, -1, 0, 1, 127, 127], [-128, -128, 5, 127]),
    "i32": ("i32", [5, -5, 7], [-2 ** 31, 2 ** 31 - 1]),
    "i16": ("i16", [-300, 300], [-300, 0, 300]),
    "f64_specials": ("f64", [-INF, -1.5, -0.0, -0.0, 0.0, 2.5, INF, NAN, NAN, None], [-INF, -0.0, 0.0, 0.0, 1.0, NAN]),
    "f64_zero_signs": ("f64", [-0.0], [0.0]),
    "f64_nan_is_greatest": ("f64", [INF, INF], [NAN]),
    "f32": ("f32", [-INF, -2.5, -0.0, 0.0, 0.5, NAN], [-3.0, -0.0, 0.0, 0.0, INF, NAN, NAN]),
    "date32": ("date32", [-400, 0, 0, 19000], [-400, -1, 19000, 19001]),
    "timestamp": ("timestamp", [-10 ** 15, 0, 10 ** 15], [-1, 1]),
    "heavy_ties": ("i64", [1] * 50 + [2] * 30 + [3], [1] * 5 + [2] * 60 + [3] * 20),
    "one_group_each": ("i64", [4, 4, 4], [9]),
    "one_group_same": ("f64", [1.0], [1.0, 1.0]),
    "all_below": ("i64", [-3, -2, -2], [0, 5]),
    "identical": ("f64", [-1.0, 2.0, 2.0], [-1.0, -1.0, 2.0, 2.0, 2.0, 2.0]),
}


@pytest.mark.parametrize("case", sorted(KS_CASES))
def test_ks_cases(dq, case):
    from deequ_amd import AnalysisRunner, DistributionDistance

    dtype, va, vb = KS_CASES[case]
    f32 = dtype == "f32"
    fa, fb = drift_ref.freq(va, f32), drift_ref.freq(vb, f32)
    want = drift_ref.ks(fa, fb, 32 if f32 else 64)
    ref = reference(["c"], [dtype], [(v,) for v in vb])
    a = DistributionDistance("c", ref, "ks")
    got = AnalysisRunner.doAnalysisRun(table({"c": (dtype, va)}), [a]).metric(a).value.get()
    print(case, got, want)
    assert got == want
    if case in ("f64_zero_signs", "f64_nan_is_greatest", "all_below"):
        assert got == 1.0
    if case in ("identical", "one_group_same"):
        assert got == 0.0


def test_ks_many_values_against_few(dq):
    from deequ_amd.drift import DistributionDistance, ReferenceDistribution

    rng = np.random.default_rng(7)
    ka = np.arange(-(BIG // 2), BIG - BIG // 2, dtype=np.int64) * 5
    kb = np.sort(rng.choice(ka, 257, replace=False)) + 1
    va, vb = rows_of(ka, 5), rows_of(kb, 6)
    want = drift_ref.ks(freq_of_array(va), freq_of_array(vb))
    ref = ReferenceDistribution.from_data(table({"c": ("i64", vb)}), "c")
    m = DistributionDistance("c", ref, "ks").calculate(table({"c": ("i64", va)}))
    assert m.value.get() == want
    # the other way round: few against many
    ref2 = ReferenceDistribution.from_data(table({"c": ("i64", va)}), "c")
    assert DistributionDistance("c", ref2, "ks").calculate(table({"c": ("i64", vb)})).value.get() == want


def test_ks_refuses_unordered_tables_before_launch(dq):
    from deequ_amd import _lib as L
    from deequ_amd.drift import freq_ks
    from deequ_amd.grouping import build_frequencies

    s = build_frequencies(table({"s": ("utf8", ["a", "b"])}), ["s"]).materialize().frequencies
    flag = build_frequencies(table({"b": ("bool", [True, False])}), ["b"]).frequencies
    i32 = build_frequencies(table({"c": ("i32", [1, 2])}), ["c"]).frequencies
    i64 = build_frequencies(table({"c": ("i64", [1, 2])}), ["c"]).frequencies
    for a, b, status, text in ((s, s, L.DQ_E_UNSUPPORTED, "hashed"), (flag, flag, L.DQ_E_UNSUPPORTED, "no order"),
                               (i32, i64, L.DQ_E_INVALID, "type 3 in table a, 2 in table b")):
        with pytest.raises(L.DQError) as e:
            freq_ks(a, b)
        assert e.value.status == status and text in str(e.value)


# ---- sharing and state --------------------------------------------------------------------------------------------------

VALS_A = [5, 5, 7, None, -2, 9, 9, 9, 11, -2, 0]
VALS_B = [5, 7, 7, -2, 12, None, 0, 0]


def small(dq):
    from deequ_amd.drift import ReferenceDistribution

    ref = ReferenceDistribution.from_data(table({"c": ("i64", VALS_B)}), "c")
    want = drift_ref.distances(drift_ref.freq(VALS_A), drift_ref.freq(VALS_B))
    return table({"c": ("i64", VALS_A)}), ref, want


def test_runner_builds_one_frequency_table_for_the_column(dq, monkeypatch):
    from deequ_amd import AnalysisRunner, DistributionDistance, Entropy, Uniqueness, grouping

    ta, ref, want = small(dq)
    calls = []
    real = grouping.build_frequencies
    monkeypatch.setattr(grouping, "build_frequencies", lambda *a, **k: calls.append(a[1:3]) or real(*a, **k))
    analyzers = [DistributionDistance("c", ref), Uniqueness("c"), DistributionDistance("c", ref, "js"), Entropy("c"),
                 DistributionDistance("c", ref, "ks")]
    ctx = AnalysisRunner.doAnalysisRun(ta, analyzers)
    assert len(calls) == 1  # one frequency table for the five of them
    assert ctx.metric(analyzers[0]).value.get() == want["linf"]
    assert abs(ctx.metric(analyzers[2]).value.get() - want["js"]) <= drift_ref.tolerance(want["union"])
    assert ctx.metric(analyzers[4]).value.get() == drift_ref.ks(drift_ref.freq(VALS_A), drift_ref.freq(VALS_B))
    assert ctx.metric(analyzers[1]).value.isSuccess and ctx.metric(analyzers[3]).value.isSuccess


def test_chunks_incremental_and_aggregated_states_equal_the_single_run(dq, tmp_path):
    from deequ_amd import AnalysisRunner, DistributionDistance, HdfsStateProvider, InMemoryStateProvider

    ta, ref, want = small(dq)
    analyzers = [DistributionDistance("c", ref, m) for m in ("linf", "tv", "js", "ks")]
    single = AnalysisRunner.doAnalysisRun(ta, analyzers)
    values = [single.metric(a).value.get() for a in analyzers]
    assert values[0] == want["linf"]
    t1, t2 = table({"c": ("i64", VALS_A[:4])}), table({"c": ("i64", VALS_A[4:])})
    chunked = AnalysisRunner.doAnalysisRun([t1, t2], analyzers)
    assert [chunked.metric(a).value.get() for a in analyzers] == values
    # incremental: the first part's states saved, the second part's run aggregated with them and saved again
    p1, p2 = InMemoryStateProvider(), HdfsStateProvider(str(tmp_path / "states"))
    AnalysisRunner.doAnalysisRun(t1, analyzers, saveStatesWith=p1)
    inc = AnalysisRunner.doAnalysisRun(t2, analyzers, aggregateWith=p1, saveStatesWith=p2)
    assert [inc.metric(a).value.get() for a in analyzers] == values
    schema = ta.schema
    assert [AnalysisRunner.runOnAggregatedStates(schema, analyzers, [p2]).metric(a).value.get() for a in analyzers] == values
    p3 = InMemoryStateProvider()
    AnalysisRunner.doAnalysisRun(t2, analyzers, saveStatesWith=p3)
    agg = AnalysisRunner.runOnAggregatedStates(schema, analyzers, [p1, p3])
    assert [agg.metric(a).value.get() for a in analyzers] == values


def test_reference_from_a_loaded_state_and_from_bytes(dq, tmp_path):
    from deequ_amd import AnalysisRunner, DistributionDistance, HdfsStateProvider, Uniqueness
    from deequ_amd.drift import ReferenceDistribution

    rows_a = [("x",), ("y",), ("y",), (None,), ("zz",)]
    rows_b = [("x",), ("x",), ("y",), ("w" * 70,), (None,)]
    ta = rows_table(["s"], ["utf8"], rows_a)
    ref = reference(["s"], ["utf8"], rows_b)
    want = [DistributionDistance("s", ref, m).calculate(ta).value.get() for m in ("linf", "tv", "js")]
    assert want[0] == drift_ref.distances(drift_ref.freq(rows_a), drift_ref.freq(rows_b))["linf"]
    # yesterday's saved Uniqueness state is today's reference
    provider = HdfsStateProvider(str(tmp_path / "yesterday"))
    AnalysisRunner.doAnalysisRun(rows_table(["s"], ["utf8"], rows_b), [Uniqueness("s")], saveStatesWith=provider)
    loaded = ReferenceDistribution.from_state(provider.load(Uniqueness("s")), ["s"])
    assert (loaded.num_groups, loaded.num_values, loaded.dtypes) == (ref.num_groups, ref.num_values, ("utf8",))
    assert [DistributionDistance("s", loaded, m).calculate(ta).value.get() for m in ("linf", "tv", "js")] == want
    again = ReferenceDistribution.from_bytes(ref.to_bytes(), ["s"])
    assert [DistributionDistance("s", again, m).calculate(ta).value.get() for m in ("linf", "tv", "js")] == want
    assert str(again) == str(ref) == "3 groups of 4 values"


def test_where_equals_the_rows_copied_out(dq):
    from deequ_amd import Check, CheckLevel, DistributionDistance, VerificationSuite
    from deequ_amd.drift import ReferenceDistribution

    c = [5, 5, 7, None, -2, 9, 9, 9, 11, -2, 0]
    w = [1, 0, 1, 1, 1, 0, 1, 1, None, 1, 0]
    ref = ReferenceDistribution.from_data(table({"c": ("i64", VALS_B)}), "c")
    ta = table({"c": ("i64", c), "w": ("i32", w)})
    kept = table({"c": ("i64", [v for v, k in zip(c, w) if k == 1])})
    for m in ("linf", "tv", "js", "ks"):
        got = DistributionDistance("c", ref, m, where="w = 1").calculate(ta).value.get()
        assert got == DistributionDistance("c", ref, m).calculate(kept).value.get()
    want = drift_ref.distances(drift_ref.freq([v for v, k in zip(c, w) if k == 1]), drift_ref.freq(VALS_B))
    check = Check(CheckLevel.Error, "drift").hasDistributionDistance("c", ref, lambda v: v == want["linf"]).where("w = 1")
    assert VerificationSuite().onData(ta).addCheck(check).run().status.name == "Success"
    # a filtered reference: the distribution of the rows the filter keeps
    fref = ReferenceDistribution.from_data(ta, "c", where="w = 1")
    assert DistributionDistance("c", fref).calculate(kept).value.get() == 0.0


def test_arrow_data_equals_from_pydict(dq):
    pa = pytest.importorskip("pyarrow")
    from deequ_amd import AnalysisRunner, DistributionDistance
    from deequ_amd.drift import ReferenceDistribution

    words_a, words_b = ["a", "b", "b", None, "cc", ""], ["a", "a", "b", "dd", None]
    arrow_a = pa.table({"s": pa.array(words_a, pa.string()), "n": pa.array([1, 2, 2, 3, None, 5], pa.int64())})
    arrow_b = pa.table({"s": pa.array(words_b, pa.string())})
    ref = ReferenceDistribution.from_data(arrow_b, "s")
    plain_ref = ReferenceDistribution.from_data(table({"s": ("utf8", words_b)}), "s")
    assert ref.to_bytes() == plain_ref.to_bytes()
    analyzers = [DistributionDistance("s", ref, m) for m in ("linf", "tv", "js")]
    got = AnalysisRunner.doAnalysisRun(arrow_a, analyzers)
    want = AnalysisRunner.doAnalysisRun(table({"s": ("utf8", words_a)}), analyzers)
    assert [got.metric(a).value.get() for a in analyzers] == [want.metric(a).value.get() for a in analyzers]
    assert DistributionDistance("s", ref).breakdown(arrow_a)["linf_group"] == \
        DistributionDistance("s", ref).breakdown(table({"s": ("utf8", words_a)}))["linf_group"]


def test_dictionary_column_follows_the_index_path(dq):
    from deequ_amd import AnalysisRunner, DistributionDistance
    from deequ_amd.drift import ReferenceDistribution
    from deequ_amd.table import Table, dict_utf8_column, encode_dictionary

    words_a, words_b = ["a", "b", "b", None, "cc", "a", "b"], ["a", "a", "b", "dd"]
    idx, values = encode_dictionary(words_a)
    td = Table([dict_utf8_column("s", idx, values)])
    ref = ReferenceDistribution.from_data(table({"s": ("utf8", words_b)}), "s")
    a = DistributionDistance("s", ref, "tv")
    got = AnalysisRunner.doAnalysisRun(td, [a]).metric(a).value.get()
    assert got == a.calculate(table({"s": ("utf8", words_a)})).value.get()


def test_binned_distribution(dq):
    from deequ_amd import AnalysisRunner, Bins, DistributionDistance, InMemoryStateProvider
    from deequ_amd.drift import ReferenceDistribution

    bins = Bins.edges([0.0, 1.0, 2.5, 4.0])
    va = [-3.0, 0.0, 0.5, 1.0, 2.4, 2.5, 4.0, 4.5, NAN, None, 9.0, -INF]
    vb = [0.1, 0.2, 1.5, 3.0, 3.5, 100.0, NAN, NAN, None, None]
    labels = bins.slot_labels()

    def slot(x):
        if x is None:
            return None
        if math.isnan(x):
            return labels[-1]
        if x < 0.0:
            return labels[0]
        if x > 4.0:
            return labels[-2]
        return labels[1 + (0 if x < 1.0 else 1 if x < 2.5 else 2)]

    fa, fb = drift_ref.freq([slot(x) for x in va]), drift_ref.freq([slot(x) for x in vb])
    want = drift_ref.distances(fa, fb)
    ref = ReferenceDistribution.from_data(table({"x": ("f64", vb)}), "x", binning=bins)
    assert (ref.binning, ref.num_groups, ref.num_values, ref.dtypes) == (bins, len(fb), 8, ("utf8",))
    ta = table({"x": ("f64", va)})
    a = DistributionDistance("x", ref, "linf", binning=bins)
    b = check_breakdown(a.breakdown(ta), want)
    assert b["linf_group"][0] in labels
    analyzers = [DistributionDistance("x", ref, m, binning=bins) for m in ("linf", "tv", "js")]
    p = InMemoryStateProvider()
    ctx = AnalysisRunner.doAnalysisRun(ta, analyzers, saveStatesWith=p)
    assert [ctx.metric(x).value.get() for x in analyzers] == [b["linf"], b["tv"], b["js"]]
    agg = AnalysisRunner.runOnAggregatedStates(ta.schema, analyzers, [p])
    assert [agg.metric(x).value.get() for x in analyzers] == [b["linf"], b["tv"], b["js"]]
    # unequal Bins, or none on one side: a Failure before any launch
    from deequ_amd import drift

    before = drift.distance_calls
    for other in (Bins.edges([0.0, 1.0, 2.5]), None):
        bad = DistributionDistance("x", ref, "linf", binning=other)
        m = AnalysisRunner.doAnalysisRun(ta, [bad]).metric(bad)
        assert m.value.isFailure and "different bins" in str(m.value.failed)
    assert drift.distance_calls == before


# ---- failures before any launch -----------------------------------------------------------------------------------------

def test_failures_before_launch(dq):
    from deequ_amd import AnalysisRunner, DistributionDistance, StoredDistribution, drift
    from deequ_amd.drift import ReferenceDistribution

    ref = ReferenceDistribution.from_data(table({"c": ("i64", VALS_B)}), "c")
    ta = table({"c": ("i64", VALS_A), "c32": ("i32", [1] * len(VALS_A)), "nulls": ("i64", [None] * len(VALS_A))})
    before = (drift.distance_calls, drift.ks_calls)

    def failure(analyzer):
        m = AnalysisRunner.doAnalysisRun(ta, [analyzer]).metric(analyzer)
        assert m.value.isFailure and m.name == "DistributionDistance"
        return m.value.failed

    e = failure(DistributionDistance("c32", ref))
    assert type(e).__name__ == "WrongColumnTypeException" and "to be i64" in str(e) and "found i32" in str(e)
    e = failure(DistributionDistance(["c", "c32"], ref))
    assert "2 columns (c, c32) cannot be compared with a distribution over 1 (c)" in str(e)
    e = failure(DistributionDistance("missing", ref, "ks"))
    assert type(e).__name__ == "NoSuchColumnException"
    e = failure(DistributionDistance("c", StoredDistribution(ref.num_groups, ref.num_values)))
    assert "cannot run" in str(e)
    assert (drift.distance_calls, drift.ks_calls) == before
    # an all-NULL column: the empty state of the frequency analyzers (the C entry returns defined = 0, no launch)
    for m in ("linf", "ks"):
        e = failure(DistributionDistance("nulls", ref, m))
        assert type(e).__name__ == "EmptyStateException" and "all input values were NULL" in str(e)
    with pytest.raises(ValueError, match="no non-NULL value"):
        ReferenceDistribution.from_data(ta, "nulls")


def test_c_entry_refuses_mismatched_tables_before_launch(dq):
    from deequ_amd import _lib as L
    from deequ_amd.drift import freq_distance
    from deequ_amd.grouping import build_frequencies

    i32 = build_frequencies(table({"c": ("i32", [1, 2])}), ["c"]).frequencies
    i64 = build_frequencies(table({"c": ("i64", [1, 2])}), ["c"]).frequencies
    s_raw = build_frequencies(table({"s": ("utf8", ["a", "b"])}), ["s"])
    s = build_frequencies(table({"s": ("utf8", ["a", "b"])}), ["s"]).materialize().frequencies
    pair = build_frequencies(table({"s": ("utf8", ["a"]), "n": ("i32", [1])}), ["s", "n"]).materialize().frequencies
    d1 = build_frequencies(table({"d": ("decimal(20,2)", [decimal.Decimal("1.00")])}), ["d"]).materialize().frequencies
    d2 = build_frequencies(table({"d": ("decimal(20,3)", [decimal.Decimal("1.000")])}), ["d"]).materialize().frequencies
    cases = ((i32, i64, L.DQ_E_INVALID, "column 0 has type 3 in table a, 2 in table b"),
             (s_raw.frequencies, s, L.DQ_E_STATE, "table a does not own its values"),
             (s, s_raw.frequencies, L.DQ_E_STATE, "table b does not own its values"),
             (s, pair, L.DQ_E_INVALID, "table a has 1 columns, table b has 2"),
             (d1, d2, L.DQ_E_INVALID, "column 0 has type"),
             (s, i64, L.DQ_E_INVALID, "column 0 has type 4 in table a, 2 in table b"))
    for a, b, status, text in cases:
        with pytest.raises(L.DQError) as e:
            freq_distance(a, b)
        assert e.value.status == status and text in str(e.value), str(e.value)
