"""Predicate type coercion at precision boundaries (Lowering::emit_col_lit in deequ_amd/csrc/dq_pred_lower.cpp).

Spark 2.2 picks the type a comparison runs in from both sides (findTightestCommonType, DecimalPrecision; restated
in oracle.dq_oracle._widen): integral vs integer / decimal exactly, anything vs double in double, a FloatType
column vs an integer literal in float but vs a decimal literal in double, and a COALESCE(col, literal) operand in
the common type of the column and its fallback.  On small integers and doubles near 0.5 those rules all give the
same rows, so the tables here carry the values where they part: 2^24, 2^53, the integer extremes, ties of the
long -> double rounding, the neighbours of 0.1 and 2.5, and for every literal of the matrix the representable
values on either side of it.

Reference: oracle.dq_oracle.OracleExpr, the per-row evaluator on Python int / Fraction / float, through
O.compute_state.  Counts are compared bit-exact through the interpreter and the compiled pass.

CPU tests (no GPU): the vectorised NpPredicate agrees with OracleExpr row by row on the same tables; routing
(gpu_eligible) equals REFUSED; the compare constant that the generated kernel gets (runner.explain) is the IEEE
bit pattern of the oracle's coerced literal.
"""
from __future__ import annotations

import math
import struct
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

from oracle import dq_oracle as O

TYPES = ("i64", "i32", "i16", "i8", "f64", "f32")
SIZES = (2049, 4097)  # one 2048-row workgroup slice + 1 row / two + 1; partial 64-row waves and 32-row words
OPS = ("<", "<=", ">", ">=", "=", "!=")
_NP = {"i64": np.int64, "i32": np.int32, "i16": np.int16, "i8": np.int8, "f64": np.float64, "f32": np.float32}
_F32_MAX = 3.4028234663852886e38

# predicates of the matrix that the planner refuses (UnsupportedOnGpuPathException through AnalysisRunner)
REFUSED: list = []

# ---------------------------------------------------------------------------------------------------------
# literals per column type: (text, all six operators?)
# ---------------------------------------------------------------------------------------------------------
_INTEGRAL_DEC = ["2.5", "-2.5", "-0.5", "0.000000000000000001", "3.0", "-3.00", "922337203685477580.7",
                 "-922337203685477580.7"]
_INTEGRAL_DBL = ["9007199254740992e0", "9.007199254740993e15", "9223372036854775807e0", "-9223372036854775808e0",
                 "2.5e0", "1e300"]
INT_LITS = {
    "i64": ["9007199254740992", "9223372036854775807", "-9223372036854775808", "0", "9007199254740993",
            "-9007199254740993", "9223372036854775806", "922337203685477581"],
    "i32": ["16777217", "2147483648", "-2147483649", "0", "-16777216", "2147483647", "-2147483648",
            "9223372036854775807"],
    "i16": ["32767", "32768", "-32769", "0", "1", "-32768"],
    "i8": ["127", "300", "-129", "0", "-1", "-128"],
    "f64": ["9007199254740993", "9007199254740992", "0", "-9007199254740993", "9223372036854775807", "3"],
    "f32": ["16777217", "-16777217", "33554433", "9223372036854775807", "16777216", "0"],
}
DEC_LITS = {
    "i64": _INTEGRAL_DEC,
    "i32": _INTEGRAL_DEC + ["2147483647.5", "-2147483648.5"],
    "i16": _INTEGRAL_DEC + ["32767.5", "-32768.5"],
    "i8": _INTEGRAL_DEC + ["127.5", "-128.5"],
    "f64": ["0.1", "2.5", "-2.5", "9007199254740993.0", "0.10000000000000001", "-0.0", "0.000000000000000001"],
    "f32": ["16777217.", "16777217.0", "0.1", "2.5", "-2.5", "33554433.", "0.100000001490116119"],
}
DBL_LITS = {
    "i64": _INTEGRAL_DBL,
    "i32": _INTEGRAL_DBL + ["2147483647e0"],
    "i16": _INTEGRAL_DBL,
    "i8": _INTEGRAL_DBL,
    "f64": ["1e-1", "9007199254740992e0", "2.5e0", "9.007199254740994e15", "1.7976931348623157e308", "5e-324",
            "1e309", "-0.0e0"],
    "f32": ["16777217e0", "1e-1", "2.5e0", "3.4028234663852886e38", "3.4028235e38", "1e-45", "1e39"],
}
# COALESCE(col, fallback) CMP literal: (fallback, literal, all six operators?).  The first rows are the cases where
# the fallback alone widens the comparison.
_INTEGRAL_COALESCE = [("1e0", "2", True), ("2.5", "2", True), ("0.0", "0", True), ("NULL", "0", True),
                      ("1e0", "0.5", False), ("3", "2.5e0", False), ("-3.00", "-3", False)]
COALESCE = {
    "i64": [("1e0", "9007199254740992", True), ("1e0", "922337203685477580.7", False),
            ("9007199254740993", "9007199254740992e0", False), ("NULL", "9007199254740993", False)]
           + _INTEGRAL_COALESCE,
    "i32": _INTEGRAL_COALESCE,
    "i16": _INTEGRAL_COALESCE,
    "i8": _INTEGRAL_COALESCE,
    "f64": [("9007199254740993", "9007199254740992", True), ("0.1", "0.10000000000000001", False),
            ("NULL", "0.1", False), ("1e0", "1", False)],
    "f32": [("0.5", "16777217", True), ("1e0", "16777217", True), ("5", "16777217", False),
            ("16777217", "16777216.0", False), ("0.5", "0.5", False), ("NULL", "16777217", False),
            ("1e0", "0.1", False), ("0.1", "1e-1", False)],
}
# two `where` users per column type: (Size's where, Sum's where)
WHERES = {
    "i64": ("c_i64 > 922337203685477580.7", "COALESCE(c_i64, 1e0) > 9007199254740992"),
    "i32": ("c_i32 < 2147483648", "COALESCE(c_i32, 0.0) >= 0"),
    "i16": ("c_i16 >= -32769", "c_i16 > 32767.5"),
    "i8": ("c_i8 = 300", "COALESCE(c_i8, 2.5) > 2"),
    "f64": ("c_f64 > 0.1", "c_f64 <= 9007199254740993"),
    "f32": ("c_f32 = 16777217.", "COALESCE(c_f32, 0.5) >= 16777217"),
}
# column vs column
PAIRS = (("i64", "f64"), ("i32", "i64"), ("i8", "i16"), ("f32", "f64"), ("f32", "i16"))


def _ops(i, full):
    """All six operators, or a strict / non-strict / equality triple that alternates with the literal's index."""
    return OPS if full else (OPS[0::2] if i % 2 == 0 else OPS[1::2])


def _build_matrix(dtype):
    c = f"c_{dtype}"
    out = []
    for lits, n_full in ((INT_LITS[dtype], 3), (DEC_LITS[dtype], len(DEC_LITS[dtype])), (DBL_LITS[dtype], 2)):
        for i, lit in enumerate(lits):
            out += [f"{c} {op} {lit}" for op in _ops(i, i < n_full)]
        out.append(f"{lits[0]} {OPS[len(out) % 4]} {c}")  # L op col (an ordering operator): flip_cmp
    for i, (fb, lit, full) in enumerate(COALESCE[dtype]):
        out += [f"COALESCE({c}, {fb}) {op} {lit}" for op in _ops(i, full)]
    fb, lit, _ = COALESCE[dtype][0]
    out.append(f"{lit} < COALESCE({c}, {fb})")
    assert len(set(out)) == len(out)
    return out


MATRIX = {t: _build_matrix(t) for t in TYPES}
# the three silently wrong cases this matrix was written for stay in it
assert "COALESCE(c_i64, 1e0) > 9007199254740992" in MATRIX["i64"]
assert {"c_f32 = 16777217.", "COALESCE(c_f32, 0.5) >= 16777217", "COALESCE(c_f32, 1e0) = 16777217"} <= set(MATRIX["f32"])
assert {"COALESCE(c_i64, 2.5) > 2", "COALESCE(c_i64, NULL) >= 0"} <= set(MATRIX["i64"])
assert {"COALESCE(c_i32, 0.0) >= 0", "COALESCE(c_i32, NULL) >= 0"} <= set(MATRIX["i32"])


# ---------------------------------------------------------------------------------------------------------
# boundary values per column type
# ---------------------------------------------------------------------------------------------------------
def _f32_next(x, up):
    return float(np.nextafter(np.float32(x), np.float32(math.inf if up else -math.inf)))


def _extras(dtype):
    """The values named for the type, as Python ints / floats."""
    if dtype == "i64":
        p53 = [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3]
        return [0, 1, -1] + p53 + [-v for v in p53] + [2 ** 63 - 1, 2 ** 63 - 2, 2 ** 63 - 513, 2 ** 63 - 512, -2 ** 63,
                                                       -2 ** 63 + 1, 922337203685477580, 922337203685477581]
    if dtype == "i32":
        return [0, 1, -1, 2 ** 24, -2 ** 24, 2 ** 24 + 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31]
    if dtype == "i16":
        return [0, 1, -1, 32767, -32768]
    if dtype == "i8":
        return [0, 1, -1, 127, -128]
    if dtype == "f64":
        return [2.0 ** 53, 2.0 ** 53 + 2, math.nextafter(2.5, 0), math.nextafter(2.5, 3), math.nextafter(0.1, 0),
                math.nextafter(0.1, 1), 0.0, -0.0, math.nan, math.inf, -math.inf, 5e-324, 1.7976931348623157e308,
                -1.7976931348623157e308]
    return [16777216.0, 16777218.0, _f32_next(0.1, False), _f32_next(0.1, True), _f32_next(2.5, False),
            _f32_next(2.5, True), 0.0, -0.0, math.nan, math.inf, -math.inf, _F32_MAX, -_F32_MAX, 1e-45]


def _literal_texts(dtype):
    out = INT_LITS[dtype] + DEC_LITS[dtype] + DBL_LITS[dtype]
    return out + [x for fb, lit, _ in COALESCE[dtype] for x in (fb, lit) if x != "NULL"]


def _neighbours(dtype, text):
    """The column type's representable values nearest the literal on each side, and the literal itself."""
    v = O.OracleExpr._num(text)[2]
    if dtype in O.INTEGRAL:
        if isinstance(v, float) and not math.isfinite(v):
            return []
        info = np.iinfo(_NP[dtype])
        f = math.floor(Fraction(v))
        return [x for x in (f - 1, f, f + 1, f + 2) if info.min <= x <= info.max]
    with np.errstate(over="ignore"):
        r = _NP[dtype](float(v))
        return [float(x) for x in (np.nextafter(r, _NP[dtype](-math.inf)), r, np.nextafter(r, _NP[dtype](math.inf)))]


def _key(x):
    return struct.pack("<d", x) if isinstance(x, float) else x


@lru_cache(maxsize=None)
def boundary_values(dtype):
    """The boundary list of a column type as an array of odd length (so tiling it moves every value through the
    lanes of a 64-row wave)."""
    vals, seen = [], set()
    for x in _extras(dtype) + [y for t in _literal_texts(dtype) for y in _neighbours(dtype, t)]:
        if _key(x) not in seen:
            seen.add(_key(x))
            vals.append(x)
    if len(vals) % 2 == 0:
        vals.append(7 if dtype in O.INTEGRAL else 7.5)
    assert 2 * len(vals) <= SIZES[0], (dtype, len(vals))
    return np.array(vals, dtype=_NP[dtype])


@lru_cache(maxsize=None)
def host_table(dtype, n):
    """{name: (dtype, values, valid)}: the boundary list tiled over all rows, ~10 % NULLs, the first len(list) rows
    valid and the next len(list) rows (the same values again) NULL; `k` weighs the rows of a `where` Sum."""
    vals = boundary_values(dtype)
    rng = np.random.default_rng(20260 + TYPES.index(dtype))
    valid = rng.random(n) >= 0.1
    valid[:len(vals)] = True
    valid[len(vals):2 * len(vals)] = False
    k = (np.arange(n) % 251 + 1).astype(np.int32)
    return {f"c_{dtype}": (dtype, np.resize(vals, n), valid), "k": ("i32", k, np.ones(n, dtype=bool))}


def _pair_values(dtype, other):
    """The named values of both types, as this type holds them (rounded / truncated; out of range dropped)."""
    vals, seen = [], set()
    for x in _extras(dtype) + _extras(other):
        if dtype in O.INTEGRAL:
            if isinstance(x, float) and not math.isfinite(x):
                continue
            x = int(x)
            if not np.iinfo(_NP[dtype]).min <= x <= np.iinfo(_NP[dtype]).max:
                continue
        else:
            with np.errstate(over="ignore"):
                x = float(_NP[dtype](x))
        if _key(x) not in seen:
            seen.add(_key(x))
            vals.append(x)
    return vals


@lru_cache(maxsize=None)
def pair_table(ta, tb, n):
    """Two columns carrying both types' named values with coprime periods, so within len(a) * len(b) rows every
    value of one meets every value of the other (equal and adjacent ones included)."""
    a, b = _pair_values(ta, tb), _pair_values(tb, ta)
    while math.gcd(len(a), len(b)) != 1:
        b.append(b[len(b) % 3])
    assert len(a) * len(b) <= SIZES[0], (ta, tb, len(a), len(b))
    rng = np.random.default_rng(77 + PAIRS.index((ta, tb)))
    va, vb = rng.random(n) >= 0.1, rng.random(n) >= 0.1
    return {"a": (ta, np.resize(np.array(a, dtype=_NP[ta]), n), va),
            "b": (tb, np.resize(np.array(b, dtype=_NP[tb]), n), vb)}


def pair_predicates():
    return [f"a {op} b" for op in OPS] + ["b < a"]


def _ocols(host):
    return {k: O.OColumn(t, v, m) for k, (t, v, m) in host.items()}


def _schema(host):
    return [(k, t, True) for k, (t, _, _) in host.items()]


_REF = {}


def _ref_state(tag, host, n, spec):
    """The row-level oracle's state of `spec`, computed once per table and analyzer."""
    key = (tag, n, spec)
    if key not in _REF:
        _REF[key] = O.compute_state(spec, _ocols(host), n)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------
# GPU: the matrix through both passes against the row-level oracle
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import deequ_amd

    return deequ_amd


def _device_table(dq, host):
    from deequ_amd.table import column_from_numpy

    return dq.Table([column_from_numpy(k, t, v, m) for k, (t, v, m) in host.items()])


def _spec(a):
    name = type(a).__name__
    if name == "Compliance":
        return ("Compliance", a.instance, a.predicate, a.where)
    return ("Size", a.where) if name == "Size" else (name, a.column, a.where)


def _mismatches(dq, tag, host, n, analyzers):
    """(pass, analyzer text, got, want) of every analyzer whose state differs from the oracle's, over plans of at
    most 12 analyzers (the compiled pass takes 16 counters)."""
    from deequ_amd.runner import scan_states

    t = _device_table(dq, host)
    bad = []
    for lo in range(0, len(analyzers), 12):
        part = analyzers[lo:lo + 12]
        for pred_pass in ("interpreter", "compiled"):
            got = scan_states(t, part, pred_pass)
            for a in part:
                ref = _ref_state(tag, host, n, _spec(a))
                if ref is None:
                    want = None
                elif type(a).__name__ == "Compliance":
                    want = dq.NumMatchesAndCount(ref.numMatches, ref.count)
                elif type(a).__name__ == "Size":
                    want = dq.NumMatches(ref.numMatches)
                else:
                    want = dq.SumState(ref.sum_)  # a sum of small integers: exact
                if got[a] != want:
                    bad.append((pred_pass, getattr(a, "predicate", None) or a.where, got[a], want))
    return bad


def _report(bad):
    return "\n".join([f"{len(bad)} states differ from the row oracle's (pass: analyzer: got, want)"]
                     + [f"{p}: {text}: {got}, {want}" for p, text, got, want in bad])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", TYPES)
def test_boundary_matrix_vs_row_oracle(dq, dtype, n):
    """Every accepted predicate of the column type's matrix, and two `where` users (the bitmap path): counts
    bit-exact against OracleExpr through the interpreter and the compiled pass."""
    host = host_table(dtype, n)
    an = [dq.Compliance(f"{dtype} {i}", p) for i, p in enumerate(MATRIX[dtype]) if p not in REFUSED]
    size_where, sum_where = WHERES[dtype]
    an += [dq.Size(where=size_where), dq.Sum("k", where=sum_where)]
    bad = _mismatches(dq, dtype, host, n, an)
    assert not bad, _report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pair", PAIRS, ids="-".join)
def test_column_pairs_vs_row_oracle(dq, pair, n):
    host = pair_table(*pair, n)
    an = [dq.Compliance(f"pair {i}", p) for i, p in enumerate(pair_predicates())]
    bad = _mismatches(dq, pair, host, n, an)
    assert not bad, _report(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TYPES)
def test_refused_predicates_route_to_fallback(dq, dtype):
    """A refused predicate is a Failure with UnsupportedOnGpuPathException beside a good analyzer, not a wrong
    count."""
    from deequ_amd.metrics import UnsupportedOnGpuPathException

    good = dq.Compliance("ok", MATRIX[dtype][0])
    bad = [dq.Compliance(f"refused {i}", p) for i, p in enumerate(MATRIX[dtype]) if p in REFUSED]
    ctx = dq.AnalysisRunner.onData(_device_table(dq, host_table(dtype, SIZES[0]))).addAnalyzers([good] + bad).run()
    assert ctx.metric(good).value.isSuccess
    for a in bad:
        assert isinstance(ctx.metric(a).value.failed, UnsupportedOnGpuPathException), a


# ---------------------------------------------------------------------------------------------------------
# CPU: the vectorised oracle, routing and the compare constants
# ---------------------------------------------------------------------------------------------------------
def _np_raises(pred, host):
    """NpPredicate documents NotImplementedError for a non-integral decimal coalesced over an integral column."""
    for side in O.OracleExpr(pred).ast[2:]:
        if side[0] == "coalesce" and side[1][0][0] == "col" and host[side[1][0][1]][0] in O.INTEGRAL:
            fb = side[1][1]
            if fb[1] == "dec" and fb[2].denominator != 1:
                return True
    return False


def _assert_np_equals_rows(host, n, preds):
    ocols = _ocols(host)
    for p in preds:
        if _np_raises(p, host):
            with pytest.raises(NotImplementedError):
                O.NpPredicate(p).eval_bool(host, n)
            continue
        t, nn = O.NpPredicate(p).eval_bool(host, n)
        rt, rnn = O.OracleExpr(p).eval_bool(ocols, n)
        assert np.array_equal(nn, rnn), (p, np.nonzero(nn != rnn)[0][:5])
        diff = np.nonzero(t != rt)[0]
        assert diff.size == 0, (p, [(int(i), host[next(iter(host))][1][i]) for i in diff[:5]])


@pytest.mark.parametrize("dtype", TYPES)
def test_np_predicate_equals_row_oracle(dtype):
    """The vectorised evaluator of the full-scale parity runs restates the same coercions: row by row equal to
    OracleExpr on the boundary table (the 2049-row table is a prefix of this one)."""
    host = host_table(dtype, SIZES[1])
    assert any(_np_raises(p, host) for p in MATRIX[dtype]) == (dtype in O.INTEGRAL)
    _assert_np_equals_rows(host, SIZES[1], MATRIX[dtype] + list(WHERES[dtype]))


@pytest.mark.parametrize("pair", PAIRS, ids="-".join)
def test_np_predicate_equals_row_oracle_on_pairs(pair):
    _assert_np_equals_rows(pair_table(*pair, SIZES[1]), SIZES[1], pair_predicates())


def test_pair_tables_meet_equal_and_adjacent_values():
    """The pair tables do what they are for: every comparison outcome occurs, and 2^53 + 1 meets 2^53."""
    host = pair_table("i64", "f64", SIZES[0])
    a, b = host["a"][1], host["b"][1]
    assert ((a == 2 ** 53 + 1) & (b == 2.0 ** 53)).any()
    for pair in PAIRS:
        host = pair_table(*pair, SIZES[0])
        for p in ("a < b", "a = b", "a > b"):
            t, _ = O.OracleExpr(p).eval_bool(_ocols(host), SIZES[0])
            assert t.any(), (pair, p)


@pytest.mark.parametrize("dtype", TYPES)
def test_routing_is_host_only(dtype):
    """gpu_eligible (no GPU) refuses exactly REFUSED, at most a tenth of a column type's predicates."""
    import deequ_amd as dq
    from deequ_amd.runner import gpu_eligible

    schema = _schema(host_table(dtype, SIZES[0]))
    preds = MATRIX[dtype] + list(WHERES[dtype])
    refused = [p for p in preds if gpu_eligible(dq.Compliance("p", p), schema) is not None]
    assert refused == [p for p in preds if p in REFUSED]
    assert 10 * len(refused) <= len(preds)
    schema = _schema(pair_table(*PAIRS[0], SIZES[0]))
    assert all(gpu_eligible(dq.Compliance("p", p), schema) is None for p in pair_predicates())


def _compare_constant(pred, dtype):
    """IEEE bits of the literal of `column-or-COALESCE CMP literal` as the oracle coerces it for the comparison
    (None for an exact integer / decimal comparison)."""
    col_type = {"f32": "flt", "f64": "dbl"}.get(dtype, "int")
    _, _, x, y = O.OracleExpr(pred).ast
    lit, operand = (x, y) if x[0] == "lit" else (y, x)
    types = [col_type] if operand[0] == "col" else [col_type if e[0] == "col" else e[1] for e in operand[1]]
    common = O._widen([O._widen(types), lit[1]])
    if common not in ("flt", "dbl"):
        return None
    return "0x%016x" % struct.unpack("<Q", struct.pack("<d", O._coerce(lit[2], lit[1], common)))[0]


@pytest.mark.parametrize("dtype", TYPES)
def test_compare_constant_in_generated_kernel(dtype):
    """The literal a float / double comparison gets in the generated kernel (host-only plan text) is the oracle's
    coerced literal, bit for bit."""
    import deequ_amd as dq
    from deequ_amd.runner import explain

    schema = _schema(host_table(dtype, SIZES[0]))
    if dtype == "f32":  # the anchors
        assert _compare_constant("c_f32 = 16777217.", "f32") == "0x4170000010000000"
        assert _compare_constant("COALESCE(c_f32, 0.5) >= 16777217", "f32") == "0x4170000010000000"
        assert _compare_constant("c_f32 = 16777217", "f32") == "0x4170000000000000"
    checked, bad = 0, []
    for p in MATRIX[dtype]:
        want = _compare_constant(p, dtype)
        if want is None or p in REFUSED:
            continue
        text = explain([dq.Compliance("p", p)], schema, "compiled")
        assert "--- generated kernel source ---" in text, p
        checked += 1
        if want + "ull" not in text:
            bad.append((p, want))
    assert checked >= (40 if dtype in ("f32", "f64") else 20), checked
    assert not bad, bad
