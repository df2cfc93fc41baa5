"""Segmented metrics on the GPU: every case compares the segmented run with the CPU reference (tests/segment_ref.py)
and, for exactness, with the existing analyzers run on schema.take_rows of each segment (at most 64 segments a case).

Bars.  Size, Completeness, Compliance, Minimum, Maximum, integral Sum, the row counts and which segments fail: bit for
bit equal to both.  Float Sum: |got - fsum| <= n 2^-53 sum|x| (any summation order).  Mean: that over n, plus one ulp.
StandardDeviation: tests/test_moments_adversarial.py's REL (1e-12 relative to the exact value), and for the
large-offset column (`wide`) its WIDE_BAR rule: max(REL, the error of Spark's own row order on the segment).  Every case
runs twice and must give identical bits, and dq_segment_order must run once per non-empty chunk.

Two tuples forced under one 64-bit hash: the grouping tests have no helper that makes such a pair (they patch the
search to report collisions), so that case is left out.
"""
import math

import numpy as np
import pytest

from tests import segment_ref as R
from tests.test_moments_adversarial import REL

pytestmark = pytest.mark.gpu

EXACT = ("Size", "Completeness", "Compliance", "Minimum", "Maximum")


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deequ_amd

    return deequ_amd


def _w(r):  # the SQL outcome of `w > 0`
    return None if r["w"] is None else r["w"] > 0


def specs(dq, x="x", i="i", where=True, wide=False):
    """(analyzer, kind, column, where outcome, predicate outcome, wide bar) over a float column x, an integral column i
    and, with `where`, the filter `w > 0`."""
    out = [(dq.Size(), "Size", None, None, None)]
    for col in (x, i):
        for kind in ("Completeness", "Sum", "Mean", "StandardDeviation", "Minimum", "Maximum"):
            out.append((getattr(dq, kind)(col), kind, col, None, None))
            if where:
                out.append((getattr(dq, kind)(col, where="w > 0"), kind, col, _w, None))
    pred = lambda r: None if r[i] is None else r[i] >= 0  # noqa: E731
    out.append((dq.Compliance("nonneg", f"{i} >= 0"), "Compliance", None, None, pred))
    if where:
        out.append((dq.Size(where="w > 0"), "Size", None, _w, None))
        out.append((dq.Compliance("nonneg", f"{i} >= 0", where="w > 0"), "Compliance", None, _w, pred))
    return [s + (wide,) for s in out]


def _bits(v):
    return None if v != v else np.float64(v).tobytes()


def _bitmap(mask):
    import torch

    words = (len(mask) + 63) // 64
    b = np.zeros((words + 1) * 8, dtype=np.uint8)
    p = np.packbits(mask, bitorder="little")
    b[:len(p)] = p
    return torch.from_numpy(b).cuda()


def _run(dq, data, keys, sp):
    from deequ_amd import segments

    before = segments.order_calls
    ctx = dq.AnalysisRunner.onData(data).segmentBy(keys).addAnalyzers([s[0] for s in sp]).run()
    return ctx, segments.order_calls - before


def check(dq, cols, keys, sp, cuts=None, oracle=True):
    from deequ_amd.schema import take_rows
    from deequ_amd.table import plain_utf8

    names = list(cols)
    n = len(next(iter(cols.values()))[1]) if cols else 0
    rows = [{c: cols[c][1][r] for c in names} for r in range(n)]
    whole = dq.Table.from_pydict(cols)
    if cuts is None:
        data, live = whole, int(n > 0)
    else:
        edges = [0] + list(cuts) + [n]
        data = [dq.Table.from_pydict({c: (cols[c][0], cols[c][1][a:b]) for c in names}) for a, b in zip(edges, edges[1:])]
        live = sum(1 for a, b in zip(edges, edges[1:]) if b > a)
    ctx, calls = _run(dq, data, keys, sp)
    again, calls2 = _run(dq, data, keys, sp)
    assert calls == live and calls2 == live, (calls, calls2, live)  # once per non-empty chunk, whatever the analyzers
    parts = R.split([tuple(r[k] for k in keys) for r in rows])
    segs = ctx.segments
    assert ctx.num_segments == len(segs) == len(parts) and set(segs) == set(parts)
    assert (segs[-1] is None) == (None in parts) if segs else not parts
    assert None not in segs[:-1]
    assert [int(v) for v in ctx.rows_per_segment] == [len(parts[s]) for s in segs]
    bad = []
    for a, kind, col, where, pred, wide in sp:
        got, fails = ctx.values(a), ctx.failures(a)
        assert got.dtype == np.float64 and got.shape == (len(segs),)
        # two runs: identical bits, identical failures
        assert got.tobytes() == again.values(a).tobytes() and set(fails) == set(again.failures(a)), a
        integral = col is not None and cols[col][0] not in ("f64", "f32")
        for si, s in enumerate(segs):
            part = [rows[r] for r in parts[s]]
            ref = R.metric(kind, len(part), values=None if col is None else [r[col] for r in part],
                           where=None if where is None else [where(r) for r in part],
                           pred=None if pred is None else [pred(r) for r in part], integral=integral)
            if ref[0] == "empty":
                if si not in fails or "Empty state for analyzer" not in str(fails[si]):
                    bad.append((str(a), s, "expected the empty-state failure", got[si]))
                continue
            if si in fails:
                bad.append((str(a), s, "unexpected failure", str(fails[si])))
                continue
            g, want = float(got[si]), ref[1]
            if kind in EXACT or (integral and kind == "Sum") or want != want or math.isinf(want):
                if _bits(g) != _bits(want):
                    bad.append((str(a), s, g, want))
                continue
            xs = [float(r[col]) for r in part if r[col] is not None and (where is None or where(r) is True)]
            if kind == "Sum":
                tol = R.sum_bound(xs)
            elif kind == "Mean":
                tol = R.sum_bound(xs) / len(xs) + math.ulp(want)
            else:
                rel = max(REL, abs(R.spark_order_sd(xs) - want) / want) if wide and want > 0 else REL
                tol = rel * want
            print(f"SEGMENT {a} segment={s} got={g!r} want={want!r} err={abs(g - want):.3e} tol={tol:.3e}")
            if not abs(g - want) <= tol:
                bad.append((str(a), s, g, want, abs(g - want), tol))
    assert not bad, bad[:10]
    if oracle and 0 < len(segs) <= 64:
        keyed = [None if any(r[k] is None for k in keys) else tuple(r[k] for k in keys) for r in rows]
        for si, s in enumerate(segs):
            mask = np.array([k == s for k in keyed], dtype=bool)
            part = take_rows(plain_utf8(whole), _bitmap(mask), int(mask.sum()))  # (a row take reads decoded strings)
            plain = dq.AnalysisRunner.onData(part).addAnalyzers([x[0] for x in sp]).run()
            for a, kind, col, *_ in sp:
                m, mine = plain.metric(a), ctx.metric(a, si)
                assert m.value.isSuccess == mine.value.isSuccess, (str(a), s, m.value, mine.value)
                integral = col is not None and cols[col][0] not in ("f64", "f32")
                if m.value.isSuccess and (kind in EXACT or (integral and kind == "Sum")):
                    assert _bits(m.value.get()) == _bits(mine.value.get()), (str(a), s, m.value.get(), mine.value.get())
    return ctx


def _cols(n, keys, seed=0, nulls=True):
    rng = np.random.default_rng(seed)
    x = [None if nulls and rng.random() < 0.2 else float(v) for v in rng.normal(1e3, 1.0, n)]
    i = [None if nulls and rng.random() < 0.1 else int(v) for v in rng.integers(-50, 1000, n)]
    w = [None if nulls and rng.random() < 0.1 else int(v) for v in rng.integers(-2, 3, n)]
    return {"k": ("i32", list(keys)), "x": ("f64", x), "i": ("i32", i), "w": ("i32", w)}


def test_no_rows(dq):
    ctx = check(dq, {"k": ("i32", []), "x": ("f64", []), "i": ("i32", []), "w": ("i32", [])}, ["k"], specs(dq))
    assert ctx.num_segments == 0 and ctx.segments == [] and ctx.successMetricsAsRows() == []


def test_one_row(dq):
    ctx = check(dq, _cols(1, [7], nulls=False), ["k"], specs(dq))
    assert ctx.segments == [(7,)] and ctx.values(dq.Size())[0] == 1.0


@pytest.mark.parametrize("n", [63, 64, 65])
def test_wave_edges_with_where_and_nulls(dq, n):
    check(dq, _cols(n, [r % 3 if r % 11 else None for r in range(n)], seed=n), ["k"], specs(dq))


def test_one_segment(dq):
    ctx = check(dq, _cols(300, [5] * 300, seed=2), ["k"], specs(dq))
    assert ctx.segments == [(5,)]


def test_every_key_null(dq):
    ctx = check(dq, _cols(130, [None] * 130, seed=3), ["k"], specs(dq))
    assert ctx.segments == [None] and ctx.rows_per_segment.tolist() == [130]


def test_every_row_its_own_segment(dq):
    n = 5000
    ctx = check(dq, _cols(n, list(range(n)), seed=4), ["k"], specs(dq), oracle=False)
    assert ctx.num_segments == n and ctx.rows_per_segment.tolist() == [1] * n


def test_tile_edges_among_single_row_segments(dq):
    from deequ_amd.segments import TILE

    keys = list(range(300))
    for j, length in enumerate((TILE - 1, TILE, TILE + 1, 3 * TILE + 1)):
        keys += [1000 + j] * length
    order = np.random.default_rng(5).permutation(len(keys))
    keys = [keys[p] for p in order]
    ctx = check(dq, _cols(len(keys), keys, seed=5), ["k"], specs(dq), oracle=False)
    by = dict(zip(ctx.segments, ctx.rows_per_segment.tolist()))
    assert [by[(1000 + j,)] for j in range(4)] == [TILE - 1, TILE, TILE + 1, 3 * TILE + 1]
    # the four long segments against take_rows too (the oracle takes at most 64 segments a case)
    sel = [k if k >= 1000 else None for k in keys]
    cols = _cols(len(keys), sel, seed=5)
    check(dq, cols, ["k"], specs(dq))


def test_dictionary_key_and_two_column_key(dq):
    n = 200
    words = ["de", "fr", "a much longer country name", "", None]
    cols = _cols(n, [r % 4 for r in range(n)], seed=6)
    cols["c"] = ("dict_utf8", [words[(r * 7) % 5] for r in range(n)])
    cols["s"] = ("utf8", [words[(r * 3) % 5] for r in range(n)])
    ctx = check(dq, cols, ["c"], specs(dq))
    assert set(ctx.segments) == {("de",), ("fr",), ("a much longer country name",), ("",), None}
    ctx = check(dq, cols, ["k", "s"], specs(dq) + [(dq.Completeness("c"), "Completeness", "c", None, None, False)])
    assert (0, "de") in ctx.segments and ctx.segments[-1] is None


def test_three_chunks_one_empty_one_segment_only_in_the_middle(dq):
    keys = [1, 2, 1, 2, None] * 20 + [9] * 30 + [2, 1] * 10 + [1, 2, 1] * 25
    ctx = check(dq, _cols(len(keys), keys, seed=7), ["k"], specs(dq), cuts=[100, 150, 150])
    assert ctx.rows_per_segment[ctx.segments.index((9,))] == 30


def test_where_excludes_every_row_of_one_segment(dq):
    n = 150
    cols = _cols(n, [r % 3 for r in range(n)], seed=8)
    w = list(cols["w"][1])
    for r in range(n):  # segment 0: `w > 0` is FALSE or NULL everywhere, and NULL in all of its rows for segment 1
        w[r] = -1 if r % 3 == 0 else (None if r % 3 == 1 else (w[r] if w[r] is not None else 1))
    cols["w"] = ("i32", w)
    ctx = check(dq, cols, ["k"], specs(dq))
    a = dq.Mean("x", where="w > 0")
    assert set(ctx.failures(a)) == {ctx.segments.index((0,)), ctx.segments.index((1,))}
    assert "Empty state for analyzer" in str(ctx.failures(a)[0]) and not ctx.failures(dq.Mean("x"))
    assert ctx.values(dq.Size()).tolist() == [50.0, 50.0, 50.0]
    assert set(ctx.failures(dq.Size(where="w > 0"))) == {ctx.segments.index((1,))}  # all NULL: a NULL sum


def test_arithmetic_compliance_and_where(dq):
    n = 120
    cols = _cols(n, [r % 5 for r in range(n)], seed=9, nulls=False)
    cols["j"] = ("i32", [None if r % 13 == 0 else (r * 5) % 17 for r in range(n)])
    pred = lambda r: None if r["j"] is None else r["i"] + r["j"] > 300  # noqa: E731
    even = lambda r: None if r["j"] is None else r["j"] % 2 == 0  # noqa: E731
    sp = [(dq.Compliance("sum", "i + j > 300"), "Compliance", None, None, pred, False),
          (dq.Mean("x", where="j % 2 = 0"), "Mean", "x", even, None, False),
          (dq.Compliance("sum", "i + j > 300", where="j % 2 = 0"), "Compliance", None, even, pred, False)]
    check(dq, cols, ["k"], sp)


def test_seventy_analyzers_split_into_two_launches(dq):
    from deequ_amd import segments

    n = 90
    cols = _cols(n, [r % 4 for r in range(n)], seed=10)
    sp = []
    for t in range(70):
        pred = (lambda t: lambda r: None if r["i"] is None else r["i"] >= t)(t)
        sp.append((dq.Compliance(f"c{t}", f"i >= {t}"), "Compliance", None, None, pred, False))
    before = segments.scan_calls
    check(dq, cols, ["k"], sp, oracle=False)
    assert segments.scan_calls - before == 2 * 3  # 140 slots: three launches a run, two runs


def test_special_floats_and_cancellation(dq):
    from deequ_amd.segments import TILE

    inf, nan = math.inf, math.nan
    rng = np.random.default_rng(11)
    keys, x, far = [], [], []
    groups = {0: [nan, 1.0, -0.0, 0.0], 1: [inf, 2.0, 3.0], 2: [-inf, inf, 1.0], 3: [-0.0, 0.0, -0.0], 4: [nan, nan],
              5: [0.0, -0.0, 5.0, None], 6: [-inf, -1.0]}
    for k, vals in groups.items():
        keys += [k] * len(vals)
        x += vals
    m = 3 * TILE + 1  # the adversarial file's `offset` family: a large offset, a tiny variance
    keys += [7] * m
    x += [float(v) for v in rng.normal(1.0, 1.0, m)]
    far = [1e12 + float(v) for v in rng.normal(0.0, 1.0, len(keys))]
    order = rng.permutation(len(keys))
    cols = {"k": ("i32", [keys[p] for p in order]), "x": ("f64", [x[p] for p in order]),
            "far": ("f64", [far[p] for p in order]), "i": ("i32", [int(p) % 7 for p in order]),
            "w": ("i32", [int(p) % 3 - 1 for p in order])}
    check(dq, cols, ["k"], specs(dq))
    check(dq, cols, ["k"], specs(dq, x="far", wide=True))


def test_verification_per_segment(dq):
    cols = {"k": ("utf8", ["a", "a", "b", "b", "c", "c"]), "x": ("f64", [1.0, 3.0, 2.0, None, 10.0, 30.0])}
    t = dq.Table.from_pydict(cols)
    check_ = dq.Check(dq.CheckLevel.Error, "per key").isComplete("x").hasMean("x", lambda v: v < 5.0)
    warn = dq.Check(dq.CheckLevel.Warning, "distinct").hasApproxCountDistinct("x", lambda v: v > 0)
    res = dq.VerificationSuite().onData(t).segmentBy("k").addCheck(check_).addCheck(warn).run()
    segs = res.segments
    assert sorted(segs) == [("a",), ("b",), ("c",)]
    assert res.status == dq.CheckStatus.Error
    by = dict(zip(segs, res.status_by_segment))
    assert by[("b",)] == by[("c",)] == dq.CheckStatus.Error and by[("a",)] == dq.CheckStatus.Warning
    assert sorted(res.failing_segments(check_)) == [("b",), ("c",)] and len(res.failing_segments()) == 3
    for s in segs:
        direct = check_.evaluate(res.context.context(s))
        mine = res.check_results(s)[check_]
        assert mine.status == direct.status
        assert [r.status for r in mine.constraintResults] == [r.status for r in direct.constraintResults]
        unsupported = res.check_results(s)[warn].constraintResults[0]
        assert unsupported.status == dq.ConstraintStatus.Failure and "not supported in segmented runs" in unsupported.message
    b = res.check_results(("b",))[check_].constraintResults
    assert [r.status for r in b] == [dq.ConstraintStatus.Failure, dq.ConstraintStatus.Success]
    rows = res.context.successMetricsAsRows()
    assert {"k": "a", "entity": "Column", "instance": "x", "name": "Mean", "value": 2.0} in rows
    with pytest.raises(ValueError, match="3 segments of \\(k\\) found, more than maxSegments = 2"):
        dq.VerificationSuite().onData(t).segmentBy("k", maxSegments=2).addCheck(check_).run()
