"""Named inputs of the quantile edge tests (test_quantile_edges_gpu.py), in plain numpy so that
test_quantile_ref_host.py checks the reference (tests/quantile_ref.py) and each generator's property on the very same
inputs without a GPU.

Every generator is deterministic from its seed and returns (dtype, values, valid).  Sizes are the smallest that reach
the code in question: the select reads 2,048 or 4,096 rows per workgroup iteration, stages 256 candidate keys in LDS
and compacts below 65,536 candidates; the digest samples 16,384 rows into 2,048 buckets and reads 1,024 rows per
workgroup iteration.  Unless a case says otherwise it carries 10 % random nulls, and a null slot never holds a zero:
it carries a random bit pattern, so that an invalid value leaking into the keys (or into the AND / OR the digit skip
is derived from) changes the answer.
"""
from __future__ import annotations

from typing import Callable, Dict, Sequence, Tuple

import numpy as np

Case = Tuple[str, np.ndarray, np.ndarray]

N_SMALL = 4099       # two workgroup iterations of the select plus a ragged tail
N_MID = 20_011       # more than the digest's 16,384 sample rows; compacts in the select's second pass
N_HOT = 150_001
N_BLIND = 32_768     # the digest samples row floor(i n / 16384): here exactly the even rows
COMPACT_FLOOR = 65_536
DIGEST_SAMPLE = 16_384

# the select's six digits as (lowest key bit, width), most significant first
DIGIT_BITS = ((53, 11), (42, 11), (31, 11), (20, 11), (9, 11), (0, 9))
ONE_BITS = (0, 8, 9, 19, 20, 30, 31, 41, 42, 52, 53, 62, 63)   # either side of every digit boundary
ONE_BITS_F64 = tuple(b for b in ONE_BITS if b <= 51)           # mantissa bits of 1.0: no NaN arises
DIGIT_SUBSETS = ((0,), (1,), (2,), (3,), (4,), (5,), (0, 5), (1, 3), (2, 4), (0, 2, 4), (1, 3, 5), (0, 1, 2, 3, 4, 5))

_NP = {"f64": np.float64, "i64": np.int64, "i32": np.int32}
_U64 = (1 << 64) - 1


def _rand_u64(rng, n: int) -> np.ndarray:
    return rng.integers(0, _U64, n, dtype=np.uint64, endpoint=True)


def _finish(rng, dtype: str, values: np.ndarray, valid: np.ndarray) -> Case:
    """The column with random bit patterns in its null slots (every third one all-ones)."""
    values = np.ascontiguousarray(values, dtype=_NP[dtype]).copy()
    valid = np.asarray(valid, dtype=bool).copy()
    dead = np.flatnonzero(~valid)
    word = np.uint32 if dtype == "i32" else np.uint64
    bits = values.view(word)
    fill = _rand_u64(rng, len(dead)).astype(word)
    fill[fill == 0] = 1
    fill[::3] = np.iinfo(word).max
    bits[dead] = fill
    return dtype, values, valid


def _nulls(rng, n: int, keep: Sequence[int] = ()) -> np.ndarray:
    valid = rng.random(n) >= 0.1
    valid[list(keep)] = True
    return valid


def _plant(rng, n: int, k: int) -> np.ndarray:
    """k distinct rows for the hand-picked values."""
    return rng.choice(n, size=min(k, n), replace=False)


def bits_f64(n: int = N_MID, seed: int = 101) -> Case:
    """Uniformly random 64-bit patterns as doubles -- every exponent, denormals, NaNs of both signs with payloads --
    plus +-DBL_MAX, +-5e-324, +-0.0 (three -0.0 to one 0.0: with equal shares, swapping the two zeros' order would
    not show), +-inf and four hand-picked NaN patterns."""
    rng = np.random.default_rng(seed)
    bits = _rand_u64(rng, n)
    fixed = np.array([np.finfo(np.float64).max, -np.finfo(np.float64).max, 5e-324, -5e-324, 0.0, -0.0, -0.0, -0.0,
                      np.inf, -np.inf]).view(np.uint64)
    nans = np.array([0x7FF0000000000001, 0xFFF8000000000123, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000], dtype=np.uint64)
    planted = np.concatenate([fixed, nans])
    at = _plant(rng, n, len(planted))
    bits[at] = planted[:len(at)]
    return _finish(rng, "f64", bits.view(np.float64), _nulls(rng, n, at))


def bits_i64(n: int = N_MID, seed: int = 101) -> Case:
    """The patterns of bits_f64 as int64, with INT64_MIN, INT64_MAX, -1 and 0."""
    rng = np.random.default_rng(seed)
    v = _rand_u64(rng, n).view(np.int64)
    planted = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0], dtype=np.int64)
    at = _plant(rng, n, len(planted))
    v[at] = planted[:len(at)]
    return _finish(rng, "i64", v, _nulls(rng, n, at))


def bits_i32(n: int = N_MID, seed: int = 102) -> Case:
    rng = np.random.default_rng(seed)
    v = rng.integers(0, (1 << 32) - 1, n, dtype=np.uint32, endpoint=True).view(np.int32)
    planted = np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 0], dtype=np.int32)
    at = _plant(rng, n, len(planted))
    v[at] = planted[:len(at)]
    return _finish(rng, "i32", v, _nulls(rng, n, at))


def one_bit(b: int, dtype: str = "i64", n: int = N_SMALL, seed: int = 7) -> Case:
    """Two values that differ in exactly bit b, in roughly equal shares.  i64: over a fixed random base; f64: the
    mantissa bit b of 1.0 (b <= 51)."""
    rng = np.random.default_rng(seed * 64 + b)
    if dtype == "f64":
        assert b <= 51
        base = int(np.array(1.0).view(np.uint64))
    else:
        base = int(_rand_u64(np.random.default_rng(seed), 1)[0]) & ~(1 << b) & _U64
    pair = np.array([base, base | (1 << b)], dtype=np.uint64)
    v = pair[rng.integers(0, 2, n)]
    v[:2] = pair[:min(n, 2)]
    return _finish(rng, dtype, v.view(_NP[dtype]), _nulls(rng, n, range(min(n, 2))))


def signed_zeros_f64(n: int = N_SMALL, seed: int = 9) -> Case:
    """-0.0 in a third of the rows, 0.0 in the others: the two compare equal, and only Double.compare's tie-break
    by sign orders them."""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(n) < 1.0 / 3.0, -0.0, 0.0)
    v[:2] = [-0.0, 0.0][:min(n, 2)]
    return _finish(rng, "f64", v, _nulls(rng, n, range(min(n, 2))))


def digit_mask(subset: Sequence[int]) -> int:
    m = 0
    for k in subset:
        lo, width = DIGIT_BITS[k]
        m |= ((1 << width) - 1) << lo
    return m


def digits(subset: Sequence[int], n: int = N_MID, seed: int = 11) -> Case:
    """An i64 column whose bits vary uniformly inside the listed select digits only; every other bit comes from one
    fixed random base.  (The order key of an int64 flips its sign bit: the same bits vary in the key.)"""
    rng = np.random.default_rng(seed * 64 + sum(1 << k for k in subset))
    m = np.uint64(digit_mask(subset))
    base = _rand_u64(np.random.default_rng(seed), 1)[0]
    v = (_rand_u64(rng, n) & m) | (base & ~m)
    if n >= 2:  # both ends of every listed digit occur: the digit differs whatever the draw
        v[0], v[1] = base & ~m, (base & ~m) | m
    return _finish(rng, "i64", v.view(np.int64), _nulls(rng, n, range(min(n, 2))))


HOT_F64, HOT_I64 = 7.25, 12_345


def hot(dtype: str = "f64", n: int = N_HOT, share: float = 0.6, seed: int = 13) -> Case:
    """One value in `share` of the rows (more than the select's compaction floor at the default n) and distinct
    random values on both sides of it in the others: a quantile inside the hot value keeps every pass on the
    whole column."""
    rng = np.random.default_rng(seed + len(dtype))
    n_hot = int(round(n * share))
    n_rest = n - n_hot
    if dtype == "f64":
        rest = np.unique(rng.normal(0.0, 1e3, 2 * n_rest + 16))
        rest = rest[rest != HOT_F64]
        v = np.full(n, HOT_F64)
    else:
        rest = np.unique(rng.integers(-(1 << 62), 1 << 62, 2 * n_rest + 16, dtype=np.int64))
        rest = rest[rest != HOT_I64]
        v = np.full(n, HOT_I64, dtype=np.int64)
    rest = rng.permutation(rest)[:n_rest]
    assert len(rest) == n_rest
    at = rng.permutation(n)[:n_rest]
    v[at] = rest
    return _finish(rng, dtype, v, _nulls(rng, n))


def sample_rows(n: int, m: int = DIGEST_SAMPLE) -> np.ndarray:
    """The rows of a one-chunk column the digest samples for its splitters: floor(i n / m), i < m (m = n below m)."""
    m = min(m, n)
    return np.array([i * n // m for i in range(m)], dtype=np.int64)


def sample_blind(kind: str, dtype: str = "f64", n: int = N_BLIND, seed: int = 17) -> Case:
    """Columns the digest's evenly spaced sample says nothing about (at n = 32,768 the sample of a one-chunk column
    is its even rows).  `nulls`: every even row NULL, the odd rows random and valid -- every splitter is the NULL
    marker and one bucket holds the column.  `one_value`: every even row holds 7.25 (7 for i64), the odd rows
    distinct random values with 10 % nulls -- every splitter is equal."""
    rng = np.random.default_rng(seed + len(kind) + len(dtype))
    assert n % 2 == 0
    if dtype == "f64":
        rest = np.unique(rng.normal(0.0, 50.0, n))
        rest = rest[rest != HOT_F64]
    else:
        rest = np.unique(rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64))
        rest = rest[rest != 7]
    rest = rng.permutation(rest)[:n // 2]
    assert len(rest) == n // 2
    v = np.zeros(n, dtype=_NP[dtype])
    v[1::2] = rest
    valid = np.ones(n, dtype=bool)
    if kind == "nulls":
        valid[0::2] = False
    elif kind == "one_value":
        v[0::2] = HOT_F64 if dtype == "f64" else 7
        valid[1::2] = rng.random(n // 2) >= 0.1
    else:
        raise ValueError(kind)
    return _finish(rng, dtype, v, valid)


def wide_f64(n: int = N_MID, seed: int = 19) -> Case:
    """Half the rows near -1.7e308, half near +1.7e308: the width of the splitters' value range overflows."""
    rng = np.random.default_rng(seed)
    mag = 1.7e308 * (1.0 - 1e-3 * rng.random(n))
    v = np.where(rng.integers(0, 2, n) == 0, -mag, mag)
    if n >= 2:
        v[0], v[1] = -1.7e308, 1.7e308
    return _finish(rng, "f64", v, _nulls(rng, n, range(min(n, 2))))


def narrow_f64(kind: str, n: int = N_MID, seed: int = 23) -> Case:
    """Value ranges so narrow that (cells - 1) / width is huge or overflows.  `ulps`: the 33 doubles within 16 ulps
    of 1.0 (ulps of 1.0 above it, half ulps below).  `denormals`: distinct denormals of both signs only -- the
    width is below 2^-1021 and the scale is infinite."""
    rng = np.random.default_rng(seed + len(kind))
    one = int(np.array(1.0).view(np.uint64))
    if kind == "ulps":
        bits = (one + rng.integers(-16, 17, n)).astype(np.uint64)
    elif kind == "denormals":
        mant = rng.choice((1 << 52) - 1, size=n, replace=False).astype(np.uint64) + np.uint64(1)
        bits = mant | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))
    else:
        raise ValueError(kind)
    return _finish(rng, "f64", bits.view(np.float64), _nulls(rng, n))


def big_i64(n: int = N_MID, seed: int = 29) -> Case:
    """Distinct values in [2^62, 2^62 + 2^20) and their negatives: above 2^53, 512 neighbouring keys share each
    double (the answer, and the value the digest's cell table sees)."""
    rng = np.random.default_rng(seed)
    off = rng.choice(1 << 20, size=n, replace=False).astype(np.int64)
    v = (np.int64(1) << np.int64(62)) + off
    v = np.where(rng.integers(0, 2, n) == 0, -v, v)
    return _finish(rng, "i64", v, _nulls(rng, n))


def _cases() -> Dict[str, Callable[..., Case]]:
    """name -> generator(n=None): n overrides the case's size (the host tests run them at reduced n)."""
    def sized(fn, *args, **kw):
        def make(n=None):
            return fn(*args, **kw) if n is None else fn(*args, n=n, **kw)
        return make

    out: Dict[str, Callable[..., Case]] = {
        "bits_f64": sized(bits_f64), "bits_i64": sized(bits_i64), "bits_i32": sized(bits_i32)}
    for b in ONE_BITS:
        out[f"one_bit_i64_{b}"] = sized(one_bit, b, "i64")
    for b in ONE_BITS_F64:
        out[f"one_bit_f64_{b}"] = sized(one_bit, b, "f64")
    out["signed_zeros_f64"] = sized(signed_zeros_f64)
    for sub in DIGIT_SUBSETS:
        out["digits_" + "".join(map(str, sub))] = sized(digits, sub)
    for dt in ("f64", "i64"):
        out[f"hot_{dt}"] = sized(hot, dt)
        for kind in ("nulls", "one_value"):
            out[f"sample_blind_{kind}_{dt}"] = sized(sample_blind, kind, dt)
    out["wide_f64"] = sized(wide_f64)
    out["narrow_f64_ulps"] = sized(narrow_f64, "ulps")
    out["narrow_f64_denormals"] = sized(narrow_f64, "denormals")
    out["big_i64"] = sized(big_i64)
    return out


CASES = _cases()

def layouts(n: int):
    """The chunk cuts every case runs in: whole, and split with a one-row and an empty chunk."""
    return {"whole": [0, n], "split": [0, min(1, n), n // 3, n // 3, n]}


# an unsorted quantile list with duplicates; 0.5 occurs at index 2 and 6, 0.9 at index 0 and 8: with at most eight
# quantiles per device call, the second 0.9 falls into the second call
QS_UNSORTED = [0.9, 0.1, 0.5, 0.1, 1.0, 0.0, 0.5, 0.25, 0.9, 0.75]
