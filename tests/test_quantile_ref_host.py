"""The quantile tests' plain reference (tests/quantile_ref.py) and inputs (tests/quantile_cases.py), checked on the
CPU: the comparator's order on a hand-written list, the reference against the oracle (whose doubles are ordered by
the sign-flip key transform the kernel also uses -- two formulations that must agree) on every case at reduced n
and on the inputs of test_quantiles.py, and every generator's property at the size the GPU tests run it: a case
that misses its property tests nothing.
"""
from __future__ import annotations

import functools
import math
import struct

import numpy as np
import pytest

from oracle import dq_oracle as O
from tests import quantile_cases as C
from tests import quantile_ref as R
from tests.test_quantiles import QS, _f64_data

ERRS = (0.0, 0.01)
DIGEST_ERRS = (0.0, 1e-4, 0.01, 0.3)


def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _f(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_comparator_order_hand_written():
    nan_pos, nan_neg = _f(0x7FF8000000000000), _f(0xFFF0000000000ABC)
    want = [-math.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, math.inf, nan_pos, nan_neg]
    assert math.isnan(nan_neg) and math.copysign(1.0, nan_neg) < 0
    for i, a in enumerate(want):
        for j, b in enumerate(want):
            c = R.compare_f64(a, b)
            if i >= 7 and j >= 7:
                assert c == 0, (a, b)  # every NaN equals every other
            else:
                assert c == (i > j) - (i < j), (a, b, c)
    rng = np.random.default_rng(1)
    for _ in range(20):
        shuffled = [want[k] for k in rng.permutation(len(want))]
        got = sorted(shuffled, key=functools.cmp_to_key(R.compare_f64))
        assert [_bits(x) for x in got[:7]] == [_bits(x) for x in want[:7]]
        assert all(math.isnan(x) for x in got[7:])
    assert R.same(nan_pos, nan_neg) and R.same(-0.0, -0.0) and not R.same(-0.0, 0.0) and not R.same(nan_pos, 1.0)


def test_reference_rank_rule_and_digest_by_hand():
    v = np.array([5.0, 1.0, 4.0, 2.0, 3.0, 99.0])
    ok = np.array([1, 1, 1, 1, 1, 0], bool)
    assert R.select(v, ok, [0.0, 0.2, 0.21, 0.5, 1.0], 0.0) == [1.0, 1.0, 2.0, 3.0, 5.0]
    assert R.select(v, ok, [0.1, 0.5, 0.9], 0.1) == [1.0, 3.0, 5.0]  # q <= err: rank 1; q >= 1 - err: rank n
    assert R.select(v, np.zeros(6, bool), [0.5], 0.0) is None
    assert R.digest(v, ok, 0.0) == (5, [(float(k), 1, 0) for k in range(1, 6)])
    assert R.digest(v, ok, 0.25) == (5, [(1.0, 1, 0), (3.0, 2, 0), (5.0, 2, 0)])  # s = floor(2 * 0.25 * 5) = 2
    assert R.digest(v, ok, 0.3) == (5, [(1.0, 1, 0), (4.0, 3, 0), (5.0, 1, 0)])   # s = 3: ranks 1, 4 and n
    assert R.digest(v, np.zeros(6, bool), 0.1) == (0, [])
    big = np.array([(1 << 62) + 1, -(1 << 62) - 1, 3], dtype=np.int64)  # int order, then float(int)
    assert R.select(big, np.ones(3, bool), [0.0, 0.5, 1.0], 0.0) == [-float(1 << 62), 3.0, float(1 << 62)]


def _agree(values, valid, tag, qlists=(QS, C.QS_UNSORTED), errs=ERRS, digest_errs=DIGEST_ERRS):
    srt = R.ordered(values, valid)
    for err in errs:
        for qs in qlists:
            want, got = R.select_ordered(srt, qs, err), O.approx_quantiles_exact(values, valid, qs, err)
            if want is None:
                assert got is None, tag
                continue
            assert len(got) == len(want) and all(R.same(a, b) for a, b in zip(got, want)), (tag, err, qs, got, want)
    for err in digest_errs:
        want, got = R.digest_ordered(srt, err), O.gk_digest_exact(values, valid, err)
        assert got[0] == want[0] and R.same_samples(got[1], want[1]), (tag, err)


def _reduced(name: str) -> int:
    if name.startswith("one_bit"):
        return 257
    if name.startswith("sample_blind"):
        return 2048
    return 3001 if name.startswith("hot") else 2003


@pytest.mark.parametrize("name", list(C.CASES))
def test_reference_agrees_with_oracle_on_cases(name):
    dtype, v, valid = C.CASES[name](_reduced(name))
    _agree(v, valid, name)


@pytest.mark.parametrize("dtype", ["f64", "i64", "i32"])
def test_reference_agrees_with_oracle_on_existing_inputs(dtype):
    """The columns of test_quantiles.py, same seeds and sizes (but for the 1,000,003-row columns)."""
    for n in (1, 2, 63, 1000, 70_001):  # test_gpu_quantiles_vs_oracle
        rng = np.random.default_rng(n * 7 + len(dtype))
        if dtype == "f64":
            v = _f64_data(rng, n)
        elif dtype == "i64":
            v = rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)
            v[rng.random(n) < 0.1] = rng.integers(-5, 5)
        else:
            v = rng.integers(-(1 << 31), (1 << 31) - 1, n, dtype=np.int64).astype(np.int32)
        valid = rng.random(n) >= 0.1
        _agree(v, valid, ("vs_oracle", dtype, n), qlists=(QS,), errs=(0.01, 0.0, 0.25), digest_errs=())
    n = 250_003  # test_gpu_quantiles_skip_equal_digits
    for case in ("i64_small", "i32_small", "i64_const", "f64_one_binade", "f64_const", "i64_two"):
        if case.split("_")[0] != dtype:
            continue
        rng = np.random.default_rng(len(case))
        v = {"i64_small": lambda: rng.integers(0, 1000, n, dtype=np.int64),
             "i32_small": lambda: rng.integers(0, 70_000, n, dtype=np.int64).astype(np.int32),
             "i64_const": lambda: np.full(n, -7, dtype=np.int64),
             "i64_two": lambda: rng.choice(np.array([1 << 40, (1 << 40) + 3], dtype=np.int64), n),
             "f64_one_binade": lambda: 1.0 + rng.random(n),
             "f64_const": lambda: np.full(n, 2.5)}[case]()
        _agree(v, rng.random(n) >= 0.1, case, qlists=(QS,), digest_errs=())
    n = 123_457  # test_gpu_digest_matches_exact_ranks
    rng = np.random.default_rng(11 + len(dtype))
    if dtype == "f64":
        skew = np.random.default_rng(11 + len("f64_skew"))
        sv = skew.choice(np.array([7.25, -0.0, 0.0, np.nan, np.inf, -np.inf, -3.0]), n,
                         p=[0.6, 0.05, 0.05, 0.05, 0.05, 0.05, 0.15])
        sv[skew.random(n) < 0.05] = skew.normal(0, 1, n)[:1]
        _agree(sv, skew.random(n) >= 0.1, "f64_skew", qlists=(), digest_errs=(0.0, 1e-5, 0.001, 0.01, 0.1, 0.5))
        v = _f64_data(rng, n)
    elif dtype == "i64":
        v = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    else:
        v = rng.integers(-(1 << 31), (1 << 31) - 1, n, dtype=np.int64).astype(np.int32)
    _agree(v, rng.random(n) >= 0.1, ("digest", dtype), qlists=(), digest_errs=(0.0, 1e-5, 0.001, 0.01, 0.1, 0.5))
    if dtype != "i32":  # test_gpu_digest_small_and_ragged
        for n in (1, 2, 63, 513, 2049, 16_385, 16_387):
            rng = np.random.default_rng(n)
            if dtype == "f64":
                v = _f64_data(rng, n)
            else:
                _f64_data(rng, n)  # (the test draws its f64 column first)
                rng.random(n)
                v = rng.integers(-50, 50, n, dtype=np.int64)
            valid = rng.random(n) >= 0.1
            valid[0] = True
            _agree(v, valid, ("ragged", dtype, n), qlists=(), digest_errs=(0.0, 0.001, 0.01, 0.3))


# ---- every generator delivers its property, at the size the GPU tests run it ----

def _valid_bits(v, valid):
    word = np.uint32 if v.dtype.itemsize == 4 else np.uint64
    return v.view(word)[valid]


def test_cases_are_deterministic_and_carry_nulls():
    for name, make in C.CASES.items():
        dtype, v, valid = make(_reduced(name))
        dtype2, v2, valid2 = make(_reduced(name))
        assert dtype == dtype2 and v.tobytes() == v2.tobytes() and valid.tobytes() == valid2.tobytes(), name
        assert len(v) == len(valid) == _reduced(name) and v.dtype == C._NP[dtype], name
        assert 0 < (~valid).sum() < len(v) // 2 + 1, name
        assert not (_valid_bits(v, ~valid) == 0).any(), name  # a null slot never holds a zero


def test_bits_cases_cover_the_value_domain():
    _, v, valid = C.bits_f64()
    x = v[valid]
    b = x.view(np.uint64)
    nan = np.isnan(x)
    assert (nan & (b >> np.uint64(63) == 1)).any() and (nan & (b >> np.uint64(63) == 0)).any()
    assert (nan & (b != np.uint64(0x7FF8000000000000))).sum() >= 3  # payloads
    exp = (b >> np.uint64(52)) & np.uint64(0x7FF)
    assert len(np.unique(exp)) > 2000 and ((exp == 0) & (b << np.uint64(1) != 0)).sum() >= 2  # denormals
    big = np.finfo(np.float64).max
    for want in (big, -big, 5e-324, -5e-324, 0.0, -0.0, np.inf, -np.inf):
        assert (b == np.array(want).view(np.uint64)).any(), want
    # unequal shares of the two zeros: swapping their order changes the sorted column
    assert (b == np.uint64(1 << 63)).sum() == 3 and (b == np.uint64(0)).sum() == 1
    _, v, valid = C.signed_zeros_f64()
    x = v[valid]
    neg = int(np.signbit(x).sum())
    assert (x == 0).all() and len(x) // 4 < neg < len(x) * 2 // 5  # 0.25 answers -0.0, 0.5 answers 0.0
    assert math.copysign(1, R.select(v, valid, [0.25], 0.0)[0]) < 0 < math.copysign(1, R.select(v, valid, [0.5], 0.0)[0])
    _, v, valid = C.bits_i64()
    assert {np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0} <= set(v[valid].tolist())
    _, v, valid = C.bits_i32()
    assert v.dtype == np.int32 and {np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 0} <= set(v[valid].tolist())


@pytest.mark.parametrize("dtype,b", [("i64", b) for b in C.ONE_BITS] + [("f64", b) for b in C.ONE_BITS_F64])
def test_one_bit_property(dtype, b):
    dt, v, valid = C.one_bit(b, dtype)
    assert dt == dtype and len(v) == C.N_SMALL
    u, cnt = np.unique(_valid_bits(v, valid), return_counts=True)
    assert len(u) == 2 and int(u[0]) ^ int(u[1]) == 1 << b
    assert cnt.min() > len(v) // 3
    if dtype == "f64":
        assert not np.isnan(v[valid]).any() and v[valid].min() == 1.0


@pytest.mark.parametrize("subset", C.DIGIT_SUBSETS)
def test_digits_property(subset):
    # the select's digits, most significant first: key bits 53-63, 42-52, 31-41, 20-30, 9-19, 0-8
    ranges = [(53, 63), (42, 52), (31, 41), (20, 30), (9, 19), (0, 8)]
    assert [(lo, lo + w - 1) for lo, w in C.DIGIT_BITS] == ranges
    dt, v, valid = C.digits(subset)
    assert dt == "i64" and len(v) == C.N_MID
    keys = _valid_bits(v, valid) ^ np.uint64(1 << 63)
    differ = int(np.bitwise_or.reduce(keys)) ^ int(np.bitwise_and.reduce(keys))
    for k, (lo, hi) in enumerate(ranges):
        m = ((1 << (hi - lo + 1)) - 1) << lo
        if k in subset:
            assert differ & m == m, (subset, k)  # every bit of a listed digit varies
            assert len(np.unique((keys >> np.uint64(lo)) & np.uint64(m >> lo))) > (1 << (hi - lo + 1)) // 2
        else:
            assert differ & m == 0, (subset, k)  # AND and OR agree: the pass over this digit is skipped


@pytest.mark.parametrize("dtype", ["f64", "i64"])
def test_hot_property(dtype):
    dt, v, valid = C.hot(dtype)
    hot_value = C.HOT_F64 if dtype == "f64" else C.HOT_I64
    x = v[valid]
    n_hot = int((x == hot_value).sum())
    assert dt == dtype and len(v) == C.N_HOT and n_hot > C.COMPACT_FLOOR
    rest = x[x != hot_value]
    assert len(np.unique(rest)) == len(rest) and (rest < hot_value).sum() > 1000 and (rest > hot_value).sum() > 1000
    assert len(rest) > C.COMPACT_FLOOR // 2  # (a non-constant column: no digit is skipped)
    srt = R.ordered(v, valid)
    for qs in (QS, C.QS_UNSORTED):
        for err in ERRS:
            got = R.select_ordered(srt, qs, err)
            on, off = sum(g == hot_value for g in got), len({g for g in got if g != hot_value})
            assert on >= 1 and off >= 2, (qs, err, got)
            # the first device call (eight quantiles) holds a quantile inside the hot value -- that call never
            # compacts -- next to quantiles whose prefixes shrink
            assert any(g == hot_value for g in got[:8]) and any(g != hot_value for g in got[:8])


@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("kind", ["nulls", "one_value"])
def test_sample_blind_property(kind, dtype):
    dt, v, valid = C.sample_blind(kind, dtype)
    assert dt == dtype and len(v) == C.N_BLIND
    rows = C.sample_rows(len(v))
    assert len(rows) == 16_384 and rows.tolist() == [i * len(v) // 16_384 for i in range(16_384)]
    assert (rows % 2 == 0).all()
    other = np.ones(len(v), bool)
    other[rows] = False
    if kind == "nulls":
        assert not valid[rows].any() and valid[other].all()
    else:
        assert valid[rows].all() and (v[rows] == (7.25 if dtype == "f64" else 7)).all()
        assert valid[other].sum() > 14_000
    rest = v[other & valid]
    assert len(np.unique(rest)) == len(rest) and len(rest) > 14_000


def test_wide_narrow_big_properties():
    _, v, valid = C.wide_f64()
    x = v[valid]
    with np.errstate(over="ignore"):
        assert np.isinf(x.max() - x.min()) and np.isfinite(x).all()
    assert (x < -1.69e308).sum() > 8000 and (x > 1.69e308).sum() > 8000
    _, v, valid = C.narrow_f64("ulps")
    x = v[valid]
    assert x.min() < 1.0 < x.max() and x.max() - x.min() <= 24 * 2.0 ** -52 and len(np.unique(x)) == 33
    _, v, valid = C.narrow_f64("denormals")
    x = v[valid]
    tiny = np.finfo(np.float64).tiny
    assert (np.abs(x) < tiny).all() and (x != 0).all() and len(np.unique(x)) == len(x)
    assert (x < 0).any() and (x > 0).any()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float64(2047.0) / (x.max() - x.min()))  # the cell table's scale overflows
    _, v, valid = C.big_i64()
    x = v[valid]
    assert len(np.unique(x)) == len(x) and (np.abs(x) >= 1 << 62).all() and (np.abs(x) < (1 << 62) + (1 << 20)).all()
    assert (x < 0).sum() > 8000 and (x > 0).sum() > 8000
    assert len(np.unique(x.astype(np.float64))) < len(x) // 4  # many keys share each double
