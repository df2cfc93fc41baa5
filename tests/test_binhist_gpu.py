"""Binned histograms on the GPU: dq_bins_create / dq_bin_count against the numpy reference of tests/binhist_ref.py
(counts are integers: EQUAL, no tolerance), then Histogram(binning=...), the checks and the profiler over it.

Shapes: rows around the 64-row group and the 512-row wave block, and one size over four workgroup ranges with a ragged
last group (a range is dq_bin.hip's rows_per_range: kRowsPerIter = 2048 rows while n <= 2048 * 2048); validity absent,
all-valid, all-NULL and random with a NULL-only 64-row group; k = 1, 2, 100, 4096 (evenly spaced edges take the
first-guess path, uneven ones the binary search: both are run)."""
import ctypes
from decimal import Context, Decimal

import numpy as np
import pytest

import binhist_ref as ref

pytestmark = pytest.mark.gpu

RANGE = 2048  # rows per workgroup range for the sizes used here (dq_bin.hip: whole kRowsPerIter blocks)
ROWS = [1, 63, 64, 65, 511, 512, 513, 3 * RANGE + 101]  # the last: 4 ranges, a 37-row last group
SENTINEL = -0x0123456789ABCDEF


def _mods():
    import deequ_amd as dq
    from deequ_amd import _lib as L, table

    return dq, L, table


def _edges(k, even=True):
    """k bins over [-50, 50]: evenly spaced, or with every second inner edge moved (so the first guess is refused)."""
    e = np.linspace(-50.0, 50.0, k + 1)
    if not even and k >= 2:
        w = e[1] - e[0]
        e[1:-1:2] += 0.45 * w
        e[2:-1:2] -= 0.45 * w
    return e


class _Bins:
    def __init__(self, edges):
        import torch

        _, L, _ = _mods()
        self.L, self.k = L, len(edges) - 1
        arr = (ctypes.c_double * len(edges))(*[float(x) for x in edges])
        self.h = ctypes.c_void_p()
        L.check(L.lib.dq_bins_create(arr, len(edges), torch.cuda.current_device(), ctypes.byref(self.h)))

    def count(self, col, type_code=None, counts=None, pad=0):
        """One dq_bin_count of a table.Column into `counts` (a fresh zeroed array with `pad` sentinel words on both
        sides when None); returns the device tensor."""
        import torch

        L = self.L
        if counts is None:
            counts = torch.full((self.k + 3 + 2 * pad,), SENTINEL, dtype=torch.int64, device="cuda")
            counts[pad:pad + self.k + 3] = 0
        view = col.view()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(L.lib.dq_bin_count(self.h, col.type_code if type_code is None else type_code, ctypes.byref(view),
                                   col.n_rows, counts.data_ptr() + 8 * pad, torch.cuda.current_device(), stream))
        return counts

    def __del__(self):
        self.L.lib.dq_bins_destroy(self.h)


def _column(dtype, values, valid=None):
    """values: a numpy array, or for a decimal dtype a list of unscaled Python ints."""
    _, _, table = _mods()
    return table.column_from_numpy("x", dtype, values, valid)


def _check(dtype, values, valid, edges, kind=None, ref_values=None):
    """GPU counts of one column == the reference's, exactly; the words around the counts untouched."""
    b = _Bins(edges)
    got = b.count(_column(dtype, values, valid), pad=3).cpu().numpy()
    assert (got[:3] == SENTINEL).all() and (got[-3:] == SENTINEL).all()
    want = ref.slot_counts(values if ref_values is None else ref_values, valid, edges, kind or dtype)
    assert got[3:-3].tolist() == want.tolist(), (dtype, len(edges) - 1)
    return want


def _validities(n, rng):
    rnd = rng.random(n) < 0.7
    if n >= 128:
        rnd[64:128] = False  # a NULL-only 64-row group
    return {"absent": None, "all valid": np.ones(n, bool), "all NULL": np.zeros(n, bool), "random": rnd}


@pytest.mark.parametrize("n", ROWS)
def test_shapes(n):
    rng = np.random.default_rng(n)
    x = rng.uniform(-60.0, 60.0, n)  # below and above are hit too
    x[rng.random(n) < 0.02] = np.nan
    x[rng.random(n) < 0.02] = np.inf
    xi = rng.integers(-60, 61, n).astype(np.int32)
    for k in (1, 2, 100, 4096):
        for even in (True, False):
            edges = _edges(k, even)
            for name, valid in _validities(n, rng).items():
                want = _check("f64", x, valid, edges)
                _check("i32", xi, valid, edges)
                assert want.sum() == (n if valid is None else valid.sum()), name


def _probe_values(edges, dtype=np.float64):
    """Every edge, its two neighbours in `dtype` (k <= 100), the last edge, +-0.0, denormals, +-inf, NaN of both signs."""
    e = np.asarray(edges, dtype=dtype)
    vals = [e, e[-1:]]
    if len(edges) - 1 <= 100:
        vals += [np.nextafter(e, dtype(-np.inf)), np.nextafter(e, dtype(np.inf))]
    tiny = np.finfo(dtype).smallest_subnormal
    vals.append(np.array([0.0, -0.0, tiny, -tiny, 1000 * tiny, np.finfo(dtype).tiny / 2, np.inf, -np.inf,
                          np.nan, -np.nan], dtype=dtype))
    out = np.concatenate(vals)
    neg_nan = np.array([np.nan], dtype=dtype)
    neg_nan.view(np.uint64 if dtype is np.float64 else np.uint32)[0] |= 1 << (63 if dtype is np.float64 else 31)
    return np.concatenate([out, neg_nan])  # (a NaN with the sign bit set, whatever -np.nan gave)


@pytest.mark.parametrize("k", [1, 2, 100, 4096])
def test_f64_edge_values(k):
    for even in (True, False):
        edges = _edges(k, even)
        edges[k // 2] = 0.0 if k > 1 else edges[k // 2]  # an edge at 0.0 for the -0.0 probe
        _check("f64", _probe_values(edges), None, edges)
    # uneven magnitudes, denormal edges: the guess must be refused or corrected, never trusted
    edges = np.array([-1e300, -1.0, -5e-324, 0.0, 5e-324, 1e-310, 1e-5, 0.1, 1.0, 2.0 ** 53, 1e300])
    _check("f64", _probe_values(edges), None, edges)
    edges = np.array([0.0, 5e-324]) if k == 1 else np.array([-0.1, 0.0, 0.1 + 0.2])
    _check("f64", _probe_values(edges), None, edges)


def test_f32_values():
    for k in (1, 2, 100):
        edges = _edges(k).astype(np.float32).astype(np.float64)  # edges a float can hit
        if k > 1:
            edges[k // 2] = 0.0
        _check("f32", _probe_values(edges, np.float32), None, edges)
    # 0.1f widens to 0.100000001490116...: above the double 0.1, so it is in the bin that starts there
    edges = [0.0, 0.1, 0.2]
    vals = np.array([0.1, 0.2, np.nextafter(np.float32(0.1), np.float32(0)), 0.0], dtype=np.float32)
    want = _check("f32", vals, None, edges)
    assert want.tolist() == [0, 2, 1, 1, 0]  # 0.2f > 0.2: above
    edges = _edges(4096).astype(np.float32).astype(np.float64)
    _check("f32", _probe_values(edges, np.float32), None, edges)


def test_i64_rounding_to_nearest_even():
    big = [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, -(2 ** 53) - 1, -(2 ** 53) - 3, 2 ** 63 - 1,
           -(2 ** 63), 0, -1, 2 ** 62, 9_223_372_036_854_775_000, 2 ** 63 - 513, 2 ** 63 - 512, -(2 ** 63) + 1025]
    vals = np.array(big, dtype=np.int64)
    for edges in ([-9.3e18, -(2.0 ** 53), 0.0, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 53 + 4, 9.3e18],
                  [-(2.0 ** 63), -(2.0 ** 53) - 2, 2.0 ** 53, 2.0 ** 63],          # 2^63 - 1 rounds onto the last edge
                  [-(2.0 ** 63) + 2048, 2.0 ** 53 + 2, 2.0 ** 63 - 1024]):         # below and above are hit
        want = _check("i64", vals, None, edges)
        assert want.sum() == len(big)
    # 2^53 + 1 ties to 2^53 (even): on the edge 2^53, not in the bin above it
    assert ref.slot_counts(np.array([2 ** 53 + 1], np.int64), None, [0.0, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 54], "i64").tolist() == \
        [0, 0, 1, 0, 0, 0]
    valid = np.array([i % 3 != 1 for i in range(len(big))])
    _check("i64", vals, valid, [-9.3e18, 0.0, 9.3e18])


def test_small_integer_extremes():
    for dtype, np_t in (("i8", np.int8), ("i16", np.int16), ("i32", np.int32)):
        lo, hi = int(np.iinfo(np_t).min), int(np.iinfo(np_t).max)
        vals = np.array([lo, lo + 1, -1, 0, 1, hi - 1, hi] * 11, dtype=np_t)
        for edges in ([float(lo), 0.0, float(hi)], [float(lo) + 1, float(hi) - 1], [float(lo) - 1, -0.5, 0.5, float(hi) + 1]):
            _check(dtype, vals, None, edges)
            _check(dtype, vals, np.array([i % 4 != 0 for i in range(len(vals))]), edges)
    _check("i8", np.arange(-128, 128).astype(np.int8), None, np.arange(-128.0, 128.0))  # one bin per value


@pytest.mark.parametrize("dtype", ["decimal(38,10)", "decimal(9,2)", "decimal(18,0)", "decimal(20,20)"])
def test_decimals_rounding_onto_edges(dtype):
    p, s = (int(v) for v in dtype[8:-1].split(","))
    if dtype == "decimal(38,10)":
        # 2^53 + 0.5 (an exact tie -> even, 2^53), 2^53 + 1 (tie -> 2^53), 2^53 + 1.0000000001 (above the tie -> 2^53 + 2)
        texts = ["9007199254740992.5", "9007199254740993", "9007199254740993.0000000001", "9007199254740992",
                 "0.1", "0.3", "-0.1", "12345678901234567890.1234567891", "-9999999999999999999999999999.9999999999",
                 "9999999999999999999999999999.9999999999", "0", "0.0000000001"]
    elif dtype == "decimal(9,2)":
        texts = ["0.10", "0.30", "1234567.89", "-1234567.89", "9999999.99", "-9999999.99", "0.01", "0", "-0.01", "0.29"]
    elif dtype == "decimal(18,0)":
        texts = ["999999999999999999", "-999999999999999999", "9007199254740993", "9007199254740992", "0", "1"]
    else:
        texts = ["0.1", "0.30000000000000004441", "0.29999999999999998890", "0.3", "0.00000000000000000001", "0", "-0.5"]
    ctx = Context(prec=80)  # (the default 28 digits would round a 38-digit value)
    decs = [Decimal(t) for t in texts]
    unscaled = [int(d.scaleb(s, context=ctx)) for d in decs]
    assert all(Decimal(u).scaleb(-s, context=ctx) == d for u, d in zip(unscaled, decs))
    doubles = sorted({float(d) for d in decs})
    # every value's own double is an edge: the rounding lands on it
    for edges in (doubles, [doubles[0], doubles[-1]], doubles[1:-1]):
        if len(edges) >= 2:
            _check(dtype, unscaled, None, edges, kind="decimal", ref_values=decs)
    valid = np.array([i % 3 != 0 for i in range(len(decs))])
    _check(dtype, unscaled, valid, doubles, kind="decimal", ref_values=decs)
    # many rows: every 64-row group shape
    rng = np.random.default_rng(p)
    many = [int(v) for v in rng.integers(-10 ** min(p, 18) + 1, 10 ** min(p, 18), 1000)]
    many_d = [Decimal(u).scaleb(-s, context=ctx) for u in many]
    lo, hi = float(min(many_d)), float(max(many_d))
    _check(dtype, many, rng.random(1000) < 0.8, np.linspace(lo, hi, 101), kind="decimal", ref_values=many_d)


def test_accumulation_over_chunks():
    rng = np.random.default_rng(5)
    edges = _edges(100)
    a, b = rng.uniform(-60, 60, 1500), rng.uniform(-60, 60, 777)
    va, vb = rng.random(1500) < 0.9, rng.random(777) < 0.5
    bins = _Bins(edges)
    counts = bins.count(_column("f64", a, va), pad=2)
    again = bins.count(_column("f64", b, vb), counts=counts, pad=2)
    got = again.cpu().numpy()
    assert (got[:2] == SENTINEL).all() and (got[-2:] == SENTINEL).all()
    want = ref.slot_counts(np.concatenate([a, b]), np.concatenate([va, vb]), edges)
    assert got[2:-2].tolist() == want.tolist()
    # chunks of two types into one array
    c = rng.integers(-60, 61, 300).astype(np.int16)
    got = bins.count(_column("i16", c, None), counts=counts, pad=2).cpu().numpy()
    assert got[2:-2].tolist() == (want + ref.slot_counts(c, None, edges, "i16")).tolist()
    # no rows: DQ_OK, nothing written
    empty = bins.count(_column("f64", np.zeros(0), None), pad=1).cpu().numpy()
    assert empty.tolist() == [SENTINEL] + [0] * 103 + [SENTINEL]


def test_refusals():
    import torch

    dq, L, table = _mods()
    bins = _Bins([0.0, 1.0])
    t = dq.Table.from_pydict({"b": ("bool", [True, False]), "d": ("date32", [1, 2]), "t": ("timestamp", [1, 2]),
                              "s": ("utf8", ["a", "b"]), "l": ("large_utf8", ["a", "b"]), "c": ("dict_utf8", ["a", "b"])})
    names = {"b": "BOOL", "d": "DATE32", "t": "TIMESTAMP", "s": "UTF8", "l": "LARGE_UTF8", "c": "DICT_UTF8"}
    for name, col in t.columns.items():
        with pytest.raises(L.DQError) as e:
            bins.count(col, pad=1)
        assert e.value.status == L.DQ_E_UNSUPPORTED and names[name] in e.value.message, name
    counts = torch.zeros(3 + 2, dtype=torch.int64, device="cuda")
    for name, col in t.columns.items():
        with pytest.raises(L.DQError):
            bins.count(col, counts=counts)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [0] * 5  # refused before any launch
    with pytest.raises(L.DQError) as e:
        _Bins(np.arange(4098.0))  # 4097 bins
    assert e.value.status == L.DQ_E_UNSUPPORTED
    _Bins(np.arange(4097.0))
    for bad, where in (([0.0], "at least 2"), ([0.0, float("nan")], "edges[1] is not finite"),
                       ([0.0, 1.0, 1.0], "edges[2] is not greater than edges[1]"), ([float("-inf"), 0.0], "edges[0] is not finite")):
        with pytest.raises(L.DQError) as e:
            _Bins(bad)
        assert e.value.status == L.DQ_E_INVALID and where in e.value.message, bad
    # the Python validation words it the same way
    with pytest.raises(ValueError, match=r"edges\[2\] is not greater than edges\[1\]"):
        dq.Bins.edges([0.0, 1.0, 1.0])


# ------------------------------------------------------------------------------------------------- analyzer level
def _data(n=3000, seed=11):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 20.0, n)
    x[rng.random(n) < 0.01] = np.nan
    x[::97] = np.inf
    valid = rng.random(n) > 0.1
    return x, valid


def _table(dq, x, valid, dtype="f64"):
    return dq.Table.from_pydict({"x": (dtype, [None if not ok else v.item() for v, ok in zip(x, valid)])})


def _as_reference(metric):
    d = metric.value.get()
    return {k: (v.absolute, v.ratio) for k, v in d.values.items()}, d.numberOfBins


def test_histogram_metric_against_reference_and_label_column():
    dq, _, _ = _mods()
    x, valid = _data()
    edges = [-40.0, -10.0, -1.0, 1e-5, 2.5, 1000.0, 2000.0]  # the last bin stays empty
    bins = dq.Bins.edges(edges)
    labels = ref.default_labels(edges)
    assert bins.slot_labels() == labels
    t = _table(dq, x, valid)
    got = dq.Histogram("x", binning=bins).calculate(t)
    counts = ref.slot_counts(x, valid, edges)
    want_values, want_bins = ref.distribution(counts, labels, len(x))
    assert _as_reference(got) == (want_values, want_bins)
    assert "[1000.0, 2000.0]" not in want_values and "NullValue" in want_values and "NaN" in want_values
    assert want_bins == 9  # below, 5 non-empty bins, above (the infinities), NaN, and NullValue; the empty bin: no group
    # the same through the existing string Histogram over the labels a binning UDF would return
    slots = ref.row_slots(x, valid, edges)
    udf = dq.Table.from_pydict({"x": ("utf8", [None if s < 0 else labels[s] for s in slots])})
    assert got.value.get() == dq.Histogram("x").calculate(udf).value.get()
    # through the runner, other column types, chunked input
    ctx = dq.AnalysisRunner.onData([_table(dq, x[:1000], valid[:1000]), _table(dq, x[1000:], valid[1000:])]) \
        .addAnalyzer(dq.Histogram("x", binning=bins)).run()
    assert ctx.metric(dq.Histogram("x", binning=bins)) == got
    xi = np.clip(np.nan_to_num(x, nan=0.0, posinf=3000.0), -3000, 3000).astype(np.int16)
    got_i = dq.Histogram("x", binning=bins).calculate(_table(dq, xi, valid, "i16"))
    assert _as_reference(got_i) == ref.distribution(ref.slot_counts(xi, valid, edges, "i16"), labels, len(xi))


def test_max_detail_bins_below_the_non_empty_bins():
    dq, _, _ = _mods()
    x, valid = _data()
    edges = [-40.0, -10.0, 0.0, 2.5, 1000.0]
    labels = ref.default_labels(edges)
    counts = ref.slot_counts(x, valid, edges)
    assert len({int(c) for c in counts if c}) == np.count_nonzero(counts)  # no ties: the cut is defined
    for top in (1, 3):
        got = dq.Histogram("x", None, top, binning=dq.Bins.edges(edges)).calculate(_table(dq, x, valid))
        want = ref.distribution(counts, labels, len(x), top)
        assert _as_reference(got) == want and len(want[0]) == top and want[1] > top


def test_custom_labels_merge_equal_ones():
    dq, _, _ = _mods()
    x, valid = _data()
    edges = [-40.0, -10.0, 0.0, 10.0, 40.0]
    given = ["tail", "body", "body", "tail"]
    bins = dq.Bins.edges(edges, labels=given)
    labels = ["< -40.0"] + given + ["> 40.0", "NaN"]
    counts = ref.slot_counts(x, valid, edges)
    got = dq.Histogram("x", binning=bins).calculate(_table(dq, x, valid))
    want = ref.distribution(counts, labels, len(x))
    assert _as_reference(got) == want
    assert want[0]["body"][0] == counts[2] + counts[3] and want[1] == 6  # below, tail, body, above, NaN, NullValue
    # a label "NullValue" joins the NULLs
    bins = dq.Bins.edges(edges, labels=["NullValue", "b", "c", "d"])
    got = dq.Histogram("x", binning=bins).calculate(_table(dq, x, valid))
    want = ref.distribution(counts, ["< -40.0", "NullValue", "b", "c", "d", "> 40.0", "NaN"], len(x))
    assert _as_reference(got) == want
    assert want[0]["NullValue"][0] == counts[1] + int((~valid).sum())


def test_states_persist_merge_and_aggregate(tmp_path):
    dq, _, _ = _mods()
    from deequ_amd.state_provider import HdfsStateProvider, InMemoryStateProvider

    x, valid = _data()
    edges = _edges(100)
    a = dq.Histogram("x", binning=dq.Bins.edges(edges))
    ta, tb = _table(dq, x[:1700], valid[:1700]), _table(dq, x[1700:], valid[1700:])
    whole = a.calculate(_table(dq, x, valid))
    assert _as_reference(whole) == ref.distribution(ref.slot_counts(x, valid, edges), ref.default_labels(edges), len(x))
    for pa_, pb in ((InMemoryStateProvider(), InMemoryStateProvider()),
                    (HdfsStateProvider(str(tmp_path / "a")), HdfsStateProvider(str(tmp_path / "b")))):
        first = a.calculate(ta, saveStatesWith=pa_)
        assert _as_reference(first) == ref.distribution(ref.slot_counts(x[:1700], valid[:1700], edges),
                                                       ref.default_labels(edges), 1700)
        assert a.calculate(tb, aggregateWith=pa_) == whole
        # through the runner, and from the two stored states alone
        second = dq.AnalysisRunner.onData(tb).addAnalyzer(a).saveStatesWith(pb).run()
        assert second.metric(a).value.isSuccess
        ctx = dq.AnalysisRunner.onData(tb).addAnalyzer(a).aggregateWith(pa_).run()
        assert ctx.metric(a) == whole
        agg = dq.AnalysisRunner.runOnAggregatedStates(ta.schema, [a], [pa_, pb])
        assert agg.metric(a) == whole
        assert pa_.load(a).numRows == 1700 and pb.load(a).numRows == len(x) - 1700


def test_two_binnings_of_one_column_two_metrics_two_states(tmp_path):
    dq, _, _ = _mods()
    from deequ_amd.state_provider import HdfsStateProvider

    x, valid = _data()
    e1, e2 = [-40.0, 0.0, 40.0], [-40.0, 1.0, 40.0]
    a1, a2 = dq.Histogram("x", binning=dq.Bins.edges(e1)), dq.Histogram("x", binning=dq.Bins.edges(e2))
    plain = dq.Histogram("x")
    p = HdfsStateProvider(str(tmp_path / "st"))
    t = _table(dq, x, valid)
    ctx = dq.AnalysisRunner.onData(t).addAnalyzers([a1, a2, plain]).saveStatesWith(p).run()
    assert len(ctx.metricMap) == 3
    for a, e in ((a1, e1), (a2, e2)):
        assert _as_reference(ctx.metric(a)) == ref.distribution(ref.slot_counts(x, valid, e), ref.default_labels(e), len(x))
        assert a.computeMetricFrom(p.load(a)) == ctx.metric(a)
    assert ctx.metric(a1) != ctx.metric(a2)
    assert len([f for f in tmp_path.iterdir() if f.name.endswith("-frequencies.dqf")]) == 3
    assert ctx.metric(plain).value.get().numberOfBins > 1000  # the exact-value histogram is still what it was


def test_checks_in_a_verification_suite():
    dq, _, _ = _mods()
    from deequ_amd import Check, CheckLevel, CheckStatus, VerificationSuite

    x, valid = _data()
    edges = [-40.0, 0.0, 40.0]
    bins = dq.Bins.edges(edges)
    counts = ref.slot_counts(x, valid, edges)
    share = counts[1] / len(x)
    t = _table(dq, x, valid)

    def run(values_ok, bins_ok):
        check = (Check(CheckLevel.Error, "distribution")
                 .hasHistogramValues("x", lambda d: values_ok(d["[-40.0, 0.0)"].ratio) and d["[-40.0, 0.0)"].absolute == counts[1],
                                     binning=bins)
                 .hasNumberOfDistinctValues("x", bins_ok, binning=bins))
        r = VerificationSuite().onData(t).addCheck(check).run()
        return r.status, [c.status for cr in r.checkResults.values() for c in cr.constraintResults]

    n_bins = ref.distribution(counts, ref.default_labels(edges), len(x))[1]
    status, each = run(lambda r: r == share, lambda n: n == n_bins)
    assert status == CheckStatus.Success, each
    status, each = run(lambda r: r > share, lambda n: n == n_bins)
    assert status == CheckStatus.Error and each == [dq.ConstraintStatus.Failure, dq.ConstraintStatus.Success]
    status, each = run(lambda r: r == share, lambda n: n == n_bins + 1)
    assert status == CheckStatus.Error and each == [dq.ConstraintStatus.Success, dq.ConstraintStatus.Failure]
    # a non-numeric column: the constraint fails with the wrong-column-type metric
    s = dq.Table.from_pydict({"x": ("utf8", ["a", "b"])})
    m = dq.Histogram("x", binning=bins).calculate(s)
    assert m.value.isFailure and "Expected type of column x" in str(m.value.failed)


def test_arrow_record_batch_input():
    pa = pytest.importorskip("pyarrow")
    dq, _, _ = _mods()
    x, valid = _data(1000)
    vals = [None if not ok else v.item() for v, ok in zip(x, valid)]
    bins = dq.Bins.equal_width(-50, 50, 10)
    a = dq.Histogram("x", binning=bins)
    batch = pa.record_batch([pa.array(vals, type=pa.float64())], names=["x"])
    got = dq.AnalysisRunner.onData(batch).addAnalyzer(a).run().metric(a)
    want = dq.AnalysisRunner.onData(dq.Table.from_pydict({"x": ("f64", vals)})).addAnalyzer(a).run().metric(a)
    assert got == want and want.value.isSuccess
    assert _as_reference(got) == ref.distribution(ref.slot_counts(x, valid, bins.bin_edges),
                                                  ref.default_labels(bins.bin_edges), len(x))


# ------------------------------------------------------------------------------------------------------- profiler
def test_profiler_numeric_distributions():
    import json

    dq, _, _ = _mods()
    rng = np.random.default_rng(3)
    n = 2000
    f = rng.normal(5.0, 3.0, n)
    fv = rng.random(n) > 0.2
    ints = rng.integers(-1000, 1000, n)
    data = {"f": ("f64", [None if not ok else v.item() for v, ok in zip(f, fv)]),
            "s": ("utf8", [None if i % 13 == 0 else str(int(v)) for i, v in enumerate(ints)]),
            "const": ("i32", [7] * n), "nulls": ("f64", [None] * n), "word": ("utf8", ["a", "b"] * (n // 2))}
    t = dq.Table.from_pydict(data)
    buckets = 16
    on = dq.ColumnProfilerRunner().onData(t).withNumericDistributions(buckets).run()
    off = dq.ColumnProfilerRunner().onData(t).run()
    for name, x, valid in (("f", f, fv), ("s", ints, np.array([i % 13 != 0 for i in range(n)]))):
        p = on.profiles[name]
        lo, hi = float(np.min(x[valid])), float(np.max(x[valid]))
        assert (p.minimum, p.maximum) == (lo, hi)
        width = (hi - lo) / buckets
        edges = [lo + i * width for i in range(buckets)] + [hi]  # equal_width's rule, restated
        want = ref.distribution(ref.slot_counts(x.astype(np.float64), valid, edges), ref.default_labels(edges), n)
        assert ({k: (v.absolute, v.ratio) for k, v in p.distribution.values.items()}, p.distribution.numberOfBins) == want
        assert sum(v.absolute for v in p.distribution.values.values()) == n and want[1] <= buckets + 1
    assert on.profiles["const"].distribution is None and on.profiles["nulls"].distribution is None
    assert not hasattr(on.profiles["word"], "distribution")
    # default bucket count
    d100 = dq.ColumnProfilerRunner().onData(t).restrictToColumns(["f"]).withNumericDistributions().run().profiles["f"]
    assert 50 < d100.distribution.numberOfBins <= 101
    # off: the profiles are today's, and their JSON has no such entry
    import dataclasses

    for name, p in off.profiles.items():
        assert getattr(p, "distribution", None) is None
        assert dataclasses.replace(on.profiles[name], **({"distribution": None} if hasattr(p, "distribution") else {})) == p
    js_on = json.loads(dq.ColumnProfiles.toJson(list(on.profiles.values())))
    js_off = json.loads(dq.ColumnProfiles.toJson(list(off.profiles.values())))
    with_entry = [c["column"] for c in js_on["columns"] if "distribution" in c]
    assert with_entry == ["f", "s"] and not any("distribution" in c for c in js_off["columns"])
    for c in js_on["columns"]:
        c.pop("distribution", None)
    assert js_on == js_off
    entry = json.loads(dq.ColumnProfiles.toJson([on.profiles["f"]]))["columns"][0]["distribution"]
    assert sorted(entry[0]) == ["count", "ratio", "value"] and sum(e["count"] for e in entry) == n
