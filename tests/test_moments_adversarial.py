"""Adversarial data for the shifted-sum moments: the column scan (dq_column_scan: range_shift_of, masked_moments,
float_block_checked), the decimal scan (decimal_range) and the Correlation pass (dq_pair_scan: range_shift).

All three take ONE shift per workgroup range -- the mean of the range's first 64-row group holding finite selected
values -- form (n, mean = shift + S1 / n, m2 = S2 - S1^2 / n) per wave and merge with Chan's formula.  The data
here make that first group unrepresentative or nearly empty: columns far from zero relative to their spread
(`offset`, `trend`), a first group holding ONE valid value far from all the rest (`lone_outlier`), ranges / chunks
that start with or consist of NULLs (`late_start`), a 1 % `where` and a `where` that starts mid-range
(`sparse_where`), a constant (`constant`: exact zero variance), magnitudes whose squares approach or pass the
fp64 range (`wide`).  NULL and unselected slots hold values far from the selected ones (and NaN, for the float
kinds): a value taken from an unselected row shows at once.

Reference: oracle/c dqo_exact_moments / dqo_exact_comoments (double-double sums around the first selected value)
combined exactly with Fraction; decimals: every cast float(Fraction(unscaled, 10^scale)) (correctly rounded, as
Decimal.toDouble), moments of those doubles in Fraction.  Bars, all taken from the existing suite:
  * n / count, Minimum, Maximum, integral Sum (wrapping int64; Mean of an integral column is that sum over the
    count) and the decimal Sum: equal to O.compute_state;
  * Mean (float kinds) and the StandardDeviation state's avg: |got - exact| <= 1e-12 (|mean| + sd)
    (test_gpu_parity.assert_state_close);
  * float Sum: |got - exact| <= 1e-12 sum|x| (test_gpu_parity's header);
  * StandardDeviation metric and m2, Correlation: 1e-12 (relative; absolute for the correlation), or the error of
    Spark's own row order on one partition (C.column_stats / C.corr, nparts = 1) where that is larger
    (test_pair_lane's drift test).  Only `offset` and `trend` use the second term: test_strict_families_* asserts on
    the CPU that Spark's order is itself inside 1e-12 on every other family, so there the bar IS 1e-12.  For
    that to hold `late_start` and `sparse_where` use family-1 data at a level of ~1e3 spreads (MILD), not 1e12.

DateType / TimestampType columns are not numeric (Preconditions.isNumeric; the plan refuses their moments with
DQ_E_TYPE, tests/test_types_gpu.py::test_non_numeric_preconditions): they ride along with Completeness only;
their layouts are the i32 / i64 kernels'.

`wide`, the +-1e160 column (every square overflows): Spark's CentralMomentAgg update m2 += delta (delta - deltaN)
adds +inf (both factors have delta's sign), never inf - inf, and the kernels' checked path agrees (finite values
stay in the sums: S2 = +inf, m2 = fma(-S1, S1 / n, +inf) = +inf).  But Spark's final aggregate then merges that
partial into the zero buffer with StandardDeviation.scala:37-44's algebra, m2 + delta deltaN n1 n2 with n1 = 0 and
delta = avg: once avg (avg / n) overflows too (here the 5 % NULLs leave avg ~ 1e157) the term is inf * 0 and Spark's
m2 and metric are NaN, not +inf.  The kernels gave +inf; decision: follow the reference's algebra -- dq_finish adds
that merge term (+-0 for every other input) when it forms the StandardDeviation state, so the class is Spark's.

Found by this file and fixed with it: with one far value alone in a range's first 64-row group the shift was that
value, and m2 / StandardDeviation / Correlation lost up to 4.4e-11 / 2.2e-11 / 2.3e-11 (lone_outlier, 40 001 rows);
the shift now comes from the first group with at least 32 selected rows (kShiftMinRows).

Each GPU test prints one `MOMENTS ...` line per case (pytest -s): the worst relative error of the
StandardDeviation metric and of m2 against exact, beside Spark's order on the same input.
"""
from __future__ import annotations

import functools
import math
import zlib
from fractions import Fraction

import numpy as np
import pytest

from oracle import dq_oracle as O
from oracle import dq_oracle_c as C

REL = 1e-12
NP = {"f64": np.float64, "f32": np.float32, "i64": np.int64, "i32": np.int32, "i16": np.int16, "i8": np.int8,
      "date32": np.int32, "timestamp": np.int64}
FLOAT = ("f64", "f32")
MOMENT_KINDS = ("f64", "f32", "i64", "i32", "i16", "i8")
COUNT_ONLY_KINDS = ("date32", "timestamp")  # not numeric in Spark: Completeness only
# family 1: (level, spread) per kind; i16 / i8: level +- spread uniform, the others N(0, spread)
OFFSET = {"f64": (1e12, 1.0), "f32": (1e6, 8.0), "i64": (2.0 ** 52, 100), "timestamp": (2.0 ** 52, 100),
          "i32": (2e9, 50), "date32": (2e9, 50), "i16": (32000, 50), "i8": (120, 5)}
# the same shape at ~1e3 spreads from zero: Spark's own order stays inside 1e-12 (the strict families)
MILD = {"f64": (1e3, 1.0), "f32": (1e4, 8.0), "i64": (1e5, 100), "timestamp": (1e5, 100), "i32": (5e4, 50),
        "date32": (5e4, 50), "i16": (32000, 50), "i8": (120, 5)}
# what NULL / unselected slots hold
FAR = {"f64": -3e15, "f32": -3e9, "i64": -(2 ** 61), "timestamp": -(2 ** 61), "i32": -(2 ** 30), "date32": -(2 ** 30),
       "i16": -32768, "i8": -128}
WIDE_BAR = ("offset", "trend")  # the only families whose bar may be Spark's own error
FORMS = [pytest.param(4097, False, id="n4097"), pytest.param(40_001, False, id="n40001"),
         pytest.param(40_001, True, id="chunked")]
SIZES = (4097, 40_001)
CHUNK_CUT = 20_000
# the column ranges of 40 001 rows are [0, 20480) and [20480, 40001) (dq_plan.cpp size_ranges: two ranges of
# whole 2048-row iterations); late_start leaves the whole first range -- and the whole first chunk -- NULL
FIRST_RANGE_ROWS = 20_480


@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available()
    import deequ_amd

    return deequ_amd


def _bm(b):
    return np.packbits(b, bitorder="little")


def _dd(p):
    return Fraction(float(p[0])) + Fraction(float(p[1]))


def _rng(tag, n):
    return np.random.default_rng([zlib.crc32(tag.encode()), n])


def _cluster(kind, level, spread, n, rng, z):
    """level + noise as float64 (integral for the integer kinds); z: a component shared by the table's columns, so
    that pairs of them correlate"""
    if kind in ("i16", "i8"):
        return level + rng.integers(-spread, spread + 1, n).astype(np.float64)
    e = spread * (0.6 * z + 0.8 * rng.normal(size=n))
    return level + (e if kind in FLOAT else np.rint(e))


def _store(kind, x, dead):
    """cast to the kind; slots in `dead` (NULL or never selected) hold a far value, every seventh a NaN (floats)"""
    v = np.asarray(x, dtype=np.float64).astype(NP[kind])
    v[dead] = FAR[kind]
    if kind in FLOAT:
        v[dead & (np.arange(len(v)) % 7 == 3)] = np.nan
    return v


class Col:
    """One column under test and its exact / Spark-order references over valid & where."""

    def __init__(self, name, kind, values, valid, where=None, mask=None, exact_zero=None, class_only=False,
                 dtype=None, unscaled=None):
        self.name, self.kind, self.values, self.valid = name, kind, values, valid
        self.where, self.mask = where, mask
        self.exact_zero = exact_zero  # the constant: avg == it, m2 == 0.0 exactly
        self.class_only = class_only  # squares overflow: only the class of the metric is compared
        self.dtype = dtype or kind  # "decimal(p,s)": `values` are the casts, `unscaled` the Python ints
        self.unscaled = unscaled
        n = len(values)
        self.all_valid = np.ones(n, bool) if valid is None else valid
        self.sel = self.all_valid if mask is None else self.all_valid & mask

    def bitmaps(self):
        return (None if self.valid is None else _bm(self.valid)), (None if self.mask is None else _bm(self.mask))

    @functools.cached_property
    def ref(self):
        """(m, mean, sd, m2, sum, sum|x|) exact, each the correctly rounded double of the Fraction"""
        m = int(self.sel.sum())
        if m == 0:
            return None
        if self.class_only:  # the squares overflow the double-double sums too: only the count
            return {"m": m}
        if self.unscaled is not None:  # decimals: moments of the casts, in Fraction
            xs = [Fraction(float(x)) for x in self.values[self.sel]]
            s1, s2, piv = sum(xs), sum(x * x for x in xs), Fraction(0)
        else:
            vb, mb = self.bitmaps()
            piv = float(self.values[np.argmax(self.sel)])
            cnt, p1, p2 = C.exact_moments(self.kind, self.values, vb, piv, 1, mb)
            assert cnt == m, (self.name, cnt, m)
            s1, s2, piv = _dd(p1), _dd(p2), Fraction(piv)
        mean = piv + s1 / m
        m2 = s2 - s1 * s1 / m
        x = self.values[self.sel].astype(np.float64)
        return {"m": m, "mean": float(mean), "sd": math.sqrt(float(m2 / m)), "m2": float(m2),
                "sum": float(mean * m), "abs": float(np.abs(x).sum())}

    @functools.cached_property
    def spark(self):
        """Spark's row order on one partition: the oracle's CentralMomentAgg"""
        if self.unscaled is not None:
            return C.column_stats("f64", self.values, _bm(self.sel), None, 1)
        vb, mb = self.bitmaps()
        return C.column_stats(self.kind, self.values, vb, mb, 1)

    def spark_errors(self):
        """relative error of Spark's order: (metric, m2)"""
        r, s = self.ref, self.spark
        return _rel(math.sqrt(s.m2 / s.n), r["sd"]), _rel(s.m2, r["m2"])

    @functools.cached_property
    def oracle(self):
        """O.compute_state over the selected rows: {analyzer name: state}"""
        c = O.OColumn(self.dtype, self.unscaled if self.unscaled is not None else self.values, self.sel)
        return {op: O.compute_state((op, "x", None), {"x": c}, len(self.values))
                for op in ("Sum", "Mean", "Minimum", "Maximum")}


def _rel(got, want):
    if got == want:
        return 0.0
    return abs(got - want) / abs(want) if want != 0.0 else math.inf


class Case:
    def __init__(self, family, n, cols, aux=(), wheres=None):
        self.family, self.n, self.cols, self.aux = family, n, cols, list(aux)
        self.wheres = wheres or {}  # where text -> bool mask


def _valid5(n, rng):
    return rng.random(n) > 0.05


def _lone(valid):
    """the table's first 64-row group: row 0 valid, rows 1..63 NULL"""
    valid[0] = True
    valid[1:64] = False
    return valid


def _late(valid, n):
    valid[:192 if n < FIRST_RANGE_ROWS else FIRST_RANGE_ROWS] = False
    return valid


def _family_values(family, kind, n, rng, z):
    """(float64 values before the cast, valid) of one numeric column of a family built on the 5 %-null pattern"""
    valid = _valid5(n, rng)
    if family == "offset":
        x = _cluster(kind, *OFFSET[kind], n, rng, z)
    elif family == "trend":
        x = OFFSET[kind][0] + np.arange(n, dtype=np.float64)
    elif family == "lone_outlier_a":  # 0 against a cluster at the level
        x = _cluster(kind, *OFFSET[kind], n, rng, z)
        x[0] = 0.0
        valid = _lone(valid)
    elif family == "lone_outlier_b":  # the level against a cluster at 0
        x = _cluster(kind, 0.0, OFFSET[kind][1], n, rng, z)
        x[0] = OFFSET[kind][0]
        valid = _lone(valid)
    elif family == "late_start":
        x = _cluster(kind, *MILD[kind], n, rng, z)
        valid = _late(valid, n)
    else:
        raise AssertionError(family)
    return x, valid


def _kinds_of(family):
    return ("f64", "i64", "i32") if family == "trend" else MOMENT_KINDS + COUNT_ONLY_KINDS


def _where_columns(n, rng):
    w = rng.integers(0, 100, n).astype(np.int32)
    w[0] = 0  # the table's first row is selected (lone_outlier under the where keeps its outlier)
    k = np.arange(n, dtype=np.int64)
    return [("w", "i32", w, None), ("k", "i64", k, None)], {"w = 0": w == 0, "k >= 5000": k >= 5000}


@functools.lru_cache(maxsize=None)
def column_case(family, n):
    rng = _rng("col:" + family, n)
    z = rng.normal(size=n)
    cols = []
    if family in ("offset", "trend", "lone_outlier_a", "lone_outlier_b", "late_start"):
        for kind in _kinds_of(family):
            x, valid = _family_values(family, kind, n, rng, z)
            cols.append(Col(kind, kind, _store(kind, x, ~valid), valid))
        return Case(family, n, cols)
    if family == "sparse_where":  # full validity; one set of columns per predicate, unselected rows far away
        aux, wheres = _where_columns(n, rng)
        for tag, where in (("a", "w = 0"), ("b", "k >= 5000")):
            for kind in MOMENT_KINDS + COUNT_ONLY_KINDS:
                x = _cluster(kind, *MILD[kind], n, rng, z)
                cols.append(Col(f"{tag}_{kind}", kind, _store(kind, x, ~wheres[where]), None, where, wheres[where]))
        return Case(family, n, cols, aux, wheres)
    if family == "constant":  # 37 of the first group's 64 rows valid
        for name, kind, c in (("f64", "f64", 0.1), ("f32", "f32", 0.1), ("f64_b", "f64", 123456.789)):
            valid = _valid5(n, rng)
            valid[:64] = False
            valid[rng.choice(64, 37, replace=False)] = True
            v = _store(kind, np.full(n, c), ~valid)
            cols.append(Col(name, kind, v, valid, exact_zero=float(NP[kind](c))))
        return Case(family, n, cols)
    if family == "wide":
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        for name, x, class_only in (("pm150", 1e150 * sign, False), ("tiny", 1e-150 * rng.normal(size=n), False),
                                    ("pm160", 1e160 * sign, True)):
            valid = _valid5(n, rng)
            cols.append(Col(name, "f64", _store("f64", x, ~valid), valid, class_only=class_only))
        return Case(family, n, cols)
    raise AssertionError(family)


COLUMN_FAMILIES = ("offset", "trend", "lone_outlier_a", "lone_outlier_b", "late_start", "sparse_where", "constant",
                   "wide")
DECIMALS = ((18, 2), (38, 10))
# (level, spread) of the unscaled values: values near 1e15 with a spread of 1e3 (the casts round: ulp 0.125), and for
# the strict late_start the same spread at ~1e3 spreads from zero
DEC_OFFSET = {(18, 2): (10 ** 17, 10 ** 5), (38, 10): (10 ** 25, 10 ** 13)}
DEC_MILD = {(18, 2): (10 ** 8, 10 ** 5), (38, 10): (10 ** 22, 10 ** 19)}
DEC_CONSTANTS = {(18, 2): (10, 12345678), (38, 10): (10 ** 9, 1234567890000000)}  # 0.1 and 123456.78(9)
DECIMAL_FAMILIES = ("offset", "lone_outlier_a", "lone_outlier_b", "late_start", "constant")


@functools.lru_cache(maxsize=None)
def decimal_case(family, n):
    rng = _rng("dec:" + family, n)
    cols = []
    for p, s in DECIMALS:
        for j, const in enumerate(DEC_CONSTANTS[(p, s)] if family == "constant" else (None,)):
            valid = _valid5(n, rng)
            level, spread = (DEC_MILD if family == "late_start" else DEC_OFFSET)[(p, s)]
            noise = [int(e * spread) for e in rng.normal(size=n)]
            if family == "constant":
                u = [const] * n
                valid[:64] = False
                valid[rng.choice(64, 37, replace=False)] = True
            elif family == "lone_outlier_b":
                u = [level] + noise[1:]
                valid = _lone(valid)
            else:
                u = [level + e for e in noise]
                if family == "lone_outlier_a":
                    u[0] = 0
                    valid = _lone(valid)
                elif family == "late_start":
                    valid = _late(valid, n)
            far = -(10 ** (p - 1))
            u = [x if ok else far for x, ok in zip(u, valid)]
            casts = np.array([float(Fraction(x, 10 ** s)) for x in u], dtype=np.float64)
            zero = float(Fraction(const, 10 ** s)) if family == "constant" else None
            cols.append(Col(f"d{p}_{s}_{j}", "f64", casts, valid, exact_zero=zero, dtype=f"decimal({p},{s})",
                            unscaled=u))
    return Case(family, n, cols)


PAIRS = (("i64", "f64"), ("i32", "f32"), ("f32", "f64"), ("i64", "i32"))
PAIR_KINDS = ("i64", "f64", "i32", "f32")
PAIR_CASES = (("offset", None), ("offset", "w = 0"), ("lone_outlier_a", None), ("lone_outlier_a", "w = 0"),
              ("lone_outlier_b", None), ("lone_outlier_b", "w = 0"), ("sparse_where", "w = 0"))


@functools.lru_cache(maxsize=None)
def pair_case(family, where, n):
    rng = _rng("pair:" + family, n)
    z = rng.normal(size=n)
    aux, wheres = _where_columns(n, rng)
    mask = None if where is None else wheres[where]
    cols = []
    for kind in PAIR_KINDS:
        if family == "sparse_where":
            x, valid = _cluster(kind, *MILD[kind], n, rng, z), None
            v = _store(kind, x, ~mask)
        else:
            x, valid = _family_values(family, kind, n, rng, z)
            v = _store(kind, x, ~valid)
        cols.append(Col(kind, kind, v, valid, where, mask))
    return Case(family, n, cols, aux, wheres)


def corr_reference(a, b):
    """(rows in both, exact correlation, Spark's order on one partition) of two Cols under their common where"""
    both = a.sel & b.sel
    (va, mb), (vb, _) = a.bitmaps(), b.bitmaps()
    px, py = float(a.values[np.argmax(both)]), float(b.values[np.argmax(both)])
    r = C.exact_comoments(a.kind, a.values, va, b.kind, b.values, vb, px, py, 1, mb)
    m = r[0]
    sx, sy, sxy, sxx, syy = (_dd(q) for q in r[1:])
    ck, xm, ym = sxy - sx * sy / m, sxx - sx * sx / m, syy - sy * sy / m
    o = C.corr(a.kind, a.values, va, b.kind, b.values, vb, mb, 1)
    return m, float(ck) / math.sqrt(float(xm) * float(ym)), o[3] / math.sqrt(o[4] * o[5])


# ---------------------------------------------------------------------------------------------------------------
# CPU: the reference before it judges the kernels, and the bar before it can hide anything
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(k for k in C.KINDS if k in NP))
def test_exact_moments_matches_fraction(kind):
    """C.exact_moments' double-double sums against pure Fraction arithmetic, per numeric kind: 300 rows of
    lone_outlier under a mask, pivot = the outlier; hi + lo within 2^-100 relative of the exact sums."""
    n = 300
    rng = _rng("selfcheck:" + kind, n)
    x, valid = _family_values("lone_outlier_a", kind, n, rng, rng.normal(size=n))
    v = _store(kind, x, ~valid)
    mask = rng.random(n) < 0.5
    mask[0] = True
    piv = float(v[0])
    cnt, p1, p2 = C.exact_moments(kind, v, _bm(valid), piv, 1, _bm(mask))
    d = [Fraction(float(t)) - Fraction(piv) for t in v[valid & mask]]
    s1, s2 = sum(d), sum(t * t for t in d)
    assert cnt == len(d) and cnt > 64
    assert abs(_dd(p1) - s1) <= abs(s1) / 2 ** 100, (kind, p1, float(s1))
    assert abs(_dd(p2) - s2) <= abs(s2) / 2 ** 100, (kind, p2, float(s2))


def _strict_cols():
    for n in SIZES:
        for family in COLUMN_FAMILIES:
            for c in column_case(family, n).cols:
                yield "column", family, n, c
        for family in DECIMAL_FAMILIES:
            for c in decimal_case(family, n).cols:
                yield "decimal", family, n, c
        for family, where in PAIR_CASES:
            for c in pair_case(family, where, n).cols:
                yield "pair", family, n, c


def test_strict_families_spark_order_within_bar():
    """max(1e-12, Spark's own error) is the bar of the drift test; here, on every family but `offset` and `trend`,
    Spark's order on one partition (the oracle's CentralMomentAgg / Corr updates) is itself within 1e-12 of exact,
    so the bar of those families is the strict 1e-12.  The constant: the exact mean is c, Spark's m2 == 0.0 exactly."""
    bad = []
    for scan, family, n, c in _strict_cols():
        if family in WIDE_BAR or c.kind in COUNT_ONLY_KINDS or c.class_only or c.ref is None:
            continue
        if c.exact_zero is not None:
            # (the final merge from the zero buffer forms avg = (c / n) n: within an ulp of c, not always c)
            if not (abs(c.spark.avg - c.exact_zero) <= math.ulp(c.exact_zero) and c.spark.m2 == 0.0 and
                    c.ref["m2"] == 0.0 and c.ref["mean"] == c.exact_zero):
                bad.append((scan, family, n, c.name, c.spark.avg, c.spark.m2))
            continue
        e_sd, e_m2 = c.spark_errors()
        if not (e_sd <= REL and e_m2 <= REL):
            bad.append((scan, family, n, c.name, c.where, e_sd, e_m2))
    for n in SIZES:
        for family, where in PAIR_CASES:
            if family in WIDE_BAR:
                continue
            by = {c.name: c for c in pair_case(family, where, n).cols}
            for x, y in PAIRS:
                _, exact, spark = corr_reference(by[x], by[y])
                if not abs(spark - exact) <= REL:
                    bad.append(("corr", family, where, n, x, y, spark, exact))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _tables(dq, case, chunked, extra=()):
    from deequ_amd.table import column_from_numpy

    cuts = [(0, CHUNK_CUT), (CHUNK_CUT, case.n)] if chunked else [(0, case.n)]
    out = []
    for lo, hi in cuts:
        cols = []
        for c in list(case.cols) + list(extra):
            v = c.unscaled[lo:hi] if c.unscaled is not None else c.values[lo:hi]
            cols.append(column_from_numpy(c.name, c.dtype, v, None if c.valid is None else c.valid[lo:hi]))
        for name, kind, v, valid in case.aux:
            cols.append(column_from_numpy(name, kind, v[lo:hi], valid))
        out.append(dq.Table(cols))
    return out if chunked else out[0]


def _moment_analyzers(dq, c, completeness=True):
    w = c.where
    if c.kind in COUNT_ONLY_KINDS:
        return [dq.Completeness(c.name, w)]
    out = [dq.Sum(c.name, w), dq.Mean(c.name, w), dq.StandardDeviation(c.name, w), dq.Minimum(c.name, w),
           dq.Maximum(c.name, w)]
    return out + ([dq.Completeness(c.name, w)] if completeness else [])


class Worst:
    """worst relative errors of a case, GPU and Spark's order: printed as the case's MOMENTS line"""

    def __init__(self):
        self.sd = self.m2 = self.spark_sd = self.spark_m2 = 0.0

    def add(self, sd, m2, spark):
        self.sd, self.m2 = max(self.sd, sd), max(self.m2, m2)
        self.spark_sd, self.spark_m2 = max(self.spark_sd, spark[0]), max(self.spark_m2, spark[1])


def _check_col(dq, case, c, got, bad, worst, minmax=True, completeness=True):
    """the states of one column's analyzers against its references; breaches are appended to `bad`"""
    n, w = case.n, c.where
    tag = (case.family, n, c.name, w)
    if completeness:
        want = dq.NumMatchesAndCount(int(c.sel.sum()), n if c.mask is None else int(c.mask.sum()))
        if got[dq.Completeness(c.name, w)] != want:
            bad.append(tag + ("Completeness", got[dq.Completeness(c.name, w)], want))
    if c.kind in COUNT_ONLY_KINDS:
        return
    st = {k: got[getattr(dq, k)(c.name, w)] for k in ("Sum", "Mean", "StandardDeviation") +
          (("Minimum", "Maximum") if minmax else ())}
    r = c.ref
    if r is None:  # nothing selected: no state
        if any(s is not None for s in st.values()):
            bad.append(tag + ("state of an empty selection", st))
        return
    if any(s is None for s in st.values()):
        bad.append(tag + ("missing state", st))
        return
    o = c.oracle
    sd_state, mean_state = st["StandardDeviation"], st["Mean"]
    if sd_state.n != r["m"] or mean_state.count != r["m"] or mean_state.count != o["Mean"].count:
        bad.append(tag + ("count", sd_state.n, mean_state.count, r["m"]))
    if minmax and (st["Minimum"].minValue != o["Minimum"].minValue or st["Maximum"].maxValue != o["Maximum"].maxValue):
        bad.append(tag + ("min / max", st["Minimum"], st["Maximum"], o["Minimum"], o["Maximum"]))
    g = sd_state.metricValue()
    if c.class_only:  # squares overflow: the class of Spark's metric (+inf here, see the module docstring)
        s = c.spark
        spark_metric = math.sqrt(s.m2 / s.n) if s.m2 == s.m2 else math.nan
        same = (math.isnan(g) and math.isnan(spark_metric)) or (g == math.inf and spark_metric == math.inf)
        if not same:
            bad.append(tag + ("class of the metric", g, spark_metric))
        return
    # Sum and Mean
    if c.kind in FLOAT and c.unscaled is None:
        for name, s in (("Sum", st["Sum"].sum_), ("Mean.sum", mean_state.sum_)):
            if not abs(s - r["sum"]) <= REL * r["abs"]:
                bad.append(tag + (name, s, r["sum"], REL * r["abs"]))
        if not abs(mean_state.metricValue() - r["mean"]) <= REL * (abs(r["mean"]) + r["sd"]):
            bad.append(tag + ("Mean", mean_state.metricValue(), r["mean"]))
    elif st["Sum"].sum_ != o["Sum"].sum_ or mean_state.sum_ != o["Mean"].sum_:  # integral (wrapping), decimal (exact)
        bad.append(tag + ("Sum", st["Sum"], mean_state, o["Sum"]))
    # the StandardDeviation state
    if c.exact_zero is not None:
        if not (sd_state.avg == c.exact_zero and sd_state.m2 == 0.0 and g == 0.0):
            bad.append(tag + ("constant", sd_state.avg, sd_state.m2, g, c.exact_zero))
        worst.add(0.0, 0.0, (0.0, 0.0))
        return
    if not abs(sd_state.avg - r["mean"]) <= REL * (abs(r["mean"]) + r["sd"]):
        bad.append(tag + ("avg", sd_state.avg, r["mean"], REL * (abs(r["mean"]) + r["sd"])))
    spark = c.spark_errors()
    e_sd, e_m2 = _rel(g, r["sd"]), _rel(sd_state.m2, r["m2"])
    worst.add(e_sd, e_m2, spark)
    wide = case.family in WIDE_BAR
    bar_sd, bar_m2 = (max(REL, spark[0]), max(REL, spark[1])) if wide else (REL, REL)
    if not e_sd <= bar_sd:
        bad.append(tag + ("StandardDeviation", g, r["sd"], e_sd, bar_sd))
    if not e_m2 <= bar_m2:
        bad.append(tag + ("m2", sd_state.m2, r["m2"], e_m2, bar_m2))


def _report(scan, case, chunked, worst, where=None):
    print(f"\nMOMENTS scan={scan} family={case.family} where={where!r} n={case.n} chunked={int(chunked)} "
          f"sd={worst.sd:.2e} m2={worst.m2:.2e} spark_sd={worst.spark_sd:.2e} spark_m2={worst.spark_m2:.2e}")


def _nan_copy(case):
    """a second copy of the case's first NaN-free f64 column with one NaN at a selected row two thirds down"""
    for c in case.cols:
        if c.kind == "f64" and c.unscaled is None and not c.class_only:
            v = c.values.copy()
            rows = np.nonzero(c.sel)[0]
            if len(rows) == 0:
                continue
            v[rows[2 * len(rows) // 3]] = np.nan
            return Col(c.name + "_nan", "f64", v, c.valid, c.where, c.mask)
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunked", FORMS)
@pytest.mark.parametrize("family", COLUMN_FAMILIES)
def test_column_scan_moments(dq, family, n, chunked):
    """dq_column_scan alone (no Correlation in the run): every kind of the family in one table and one scan; plus a
    copy of the f64 column with one selected NaN -- its block takes float_block_checked and its moments are
    Spark's NaN (as test_infinities_vs_oracle), while the first copy still meets the bars."""
    from deequ_amd.runner import scan_states

    case = column_case(family, n)
    nan = _nan_copy(case)
    an = [a for c in case.cols for a in _moment_analyzers(dq, c)]
    if nan is not None:
        an += _moment_analyzers(dq, nan)
    got = scan_states(_tables(dq, case, chunked, [nan] if nan is not None else []), an)
    bad, worst = [], Worst()
    for c in case.cols:
        _check_col(dq, case, c, got, bad, worst)
    if nan is not None:
        w, o = nan.where, nan.oracle
        sd, mean, total = (got[k(nan.name, w)] for k in (dq.StandardDeviation, dq.Mean, dq.Sum))
        m = int(nan.sel.sum())
        if not (sd.n == m and mean.count == m and math.isnan(sd.metricValue()) and math.isnan(mean.sum_) and
                math.isnan(total.sum_) and math.isnan(o["Sum"].sum_)):
            bad.append((family, n, nan.name, "NaN propagation", sd, mean, total))
        lo, hi = got[dq.Minimum(nan.name, w)], got[dq.Maximum(nan.name, w)]
        if not (lo.minValue == o["Minimum"].minValue and math.isnan(hi.maxValue) and math.isnan(o["Maximum"].maxValue)):
            bad.append((family, n, nan.name, "NaN min / max", lo, hi, o["Minimum"], o["Maximum"]))
        want = dq.NumMatchesAndCount(m, n if nan.mask is None else int(nan.mask.sum()))
        if got[dq.Completeness(nan.name, w)] != want:
            bad.append((family, n, nan.name, "Completeness", got[dq.Completeness(nan.name, w)], want))
    _report("column", case, chunked, worst)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunked", FORMS)
@pytest.mark.parametrize("family", DECIMAL_FAMILIES)
def test_decimal_scan_moments(dq, family, n, chunked):
    """decimal_range: DecimalType(18, 2) (the 64-bit cast) and DecimalType(38, 10) (the 128-bit cast) near 1e15, where
    the casts themselves round; Sum / Mean are the exact decimal sum, StandardDeviation the moments of the casts."""
    from deequ_amd.runner import scan_states

    case = decimal_case(family, n)
    an = [a for c in case.cols for a in _moment_analyzers(dq, c, completeness=False)]
    got = scan_states(_tables(dq, case, chunked), an)
    bad, worst = [], Worst()
    for c in case.cols:
        _check_col(dq, case, c, got, bad, worst, completeness=False)
    _report("decimal", case, chunked, worst)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunked", FORMS)
@pytest.mark.parametrize("family,where", PAIR_CASES)
def test_pair_pass_moments_narrow_kinds_and_where(dq, family, where, n, chunked):
    """dq_pair_scan on mixed-kind pairs (the register-staged fold), with and without the 1 % where: Correlation
    against exact_comoments, and the Mean / StandardDeviation of both columns, which the pair pass fuses."""
    from deequ_amd.runner import scan_states

    case = pair_case(family, where, n)
    by = {c.name: c for c in case.cols}
    an = [dq.Correlation(x, y, where) for x, y in PAIRS]
    for c in case.cols:
        an += [dq.Sum(c.name, where), dq.Mean(c.name, where), dq.StandardDeviation(c.name, where)]
    got = scan_states(_tables(dq, case, chunked), an)
    bad, worst = [], Worst()
    for c in case.cols:
        _check_col(dq, case, c, got, bad, worst, minmax=False, completeness=False)
    worst_corr = worst_spark = 0.0
    for x, y in PAIRS:
        m, exact, spark = corr_reference(by[x], by[y])
        st = got[dq.Correlation(x, y, where)]
        err, spark_err = abs(st.metricValue() - exact), abs(spark - exact)
        worst_corr, worst_spark = max(worst_corr, err), max(worst_spark, spark_err)
        bar = max(REL, spark_err) if family in WIDE_BAR else REL
        if st.n != m or not err <= bar:
            bad.append((family, where, n, x, y, st.n, m, st.metricValue(), exact, err, bar))
    _report("pair", case, chunked, worst, where)
    print(f"MOMENTS scan=pair-corr family={family} where={where!r} n={n} chunked={int(chunked)} "
          f"corr={worst_corr:.2e} spark_corr={worst_spark:.2e}")
    assert not bad, bad
