"""Host-side inputs of the grouping edge tests (test_group_edges_gpu.py, test_group_metrics_exact_gpu.py), in plain
numpy so that test_group_ref_host.py checks the reference (tests/group_ref.py) on the very same inputs without a GPU.

A column is an HCol (name, dtype, values, valid); a chunk is a list of equally long HCols; a case is a list of chunks.
Null slots never hold zeros: they carry random non-zero payloads, every third one all-ones, so that an invalid value
leaking into the keys (or into the AND / OR from which the sort's bit range is derived) changes the table.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_NP = {"f64": np.float64, "f32": np.float32, "i64": np.int64, "i32": np.int32, "i16": np.int16, "i8": np.int8,
       "bool": np.bool_}
STRING = ("utf8", "large_utf8")

TILE = 2048                    # kCompactRows: rows per workgroup tile of group_compact
FULL_GRID = 2048 * TILE        # rows one pass of the capped launch grid covers
MULTI_TILE_ROWS = FULL_GRID + TILE + 1


@dataclass
class HCol:
    name: str
    dtype: str
    values: object                 # numpy array, or a list of bytes (strings)
    valid: Optional[np.ndarray]    # None: a column without a validity bitmap


Chunk = List[HCol]


def with_nulls(rng, name: str, dtype: str, values, valid: Optional[np.ndarray]) -> HCol:
    """The column with its null slots overwritten by non-zero payloads (every third one all-ones)."""
    if valid is None:
        return HCol(name, dtype, values if dtype in STRING else np.ascontiguousarray(values, dtype=_NP[dtype]), None)
    valid = np.asarray(valid, dtype=bool)
    dead = np.flatnonzero(~valid)
    if dtype in STRING:
        vals = list(values)
        for j, at in enumerate(dead):
            vals[at] = b"\xff" * 9 if j % 3 == 0 else b"null-%d" % int(rng.integers(0, 1 << 30))
        return HCol(name, dtype, vals, valid)
    vals = np.array(values, dtype=_NP[dtype])
    if dtype == "bool":
        vals[dead] = True
    elif dtype in ("f64", "f32"):
        w = np.uint64 if dtype == "f64" else np.uint32
        bits = vals.view(w)
        bits[dead] = rng.integers(1, np.iinfo(w).max, len(dead), dtype=w)
        bits[dead[::3]] = np.iinfo(w).max
    else:
        info = np.iinfo(_NP[dtype])
        fill = rng.integers(info.min, info.max, len(dead), dtype=_NP[dtype], endpoint=True)
        fill[fill == 0] = 1
        vals[dead] = fill
        vals[dead[::3]] = -1
    return HCol(name, dtype, vals, valid)


def forced_valid(rng, n: int, frac: float, keep: Sequence[int] = (), drop: Sequence[int] = ()) -> np.ndarray:
    valid = rng.random(n) >= frac
    for at in keep:
        if 0 <= at < n:
            valid[at] = True
    for at in drop:
        if 0 <= at < n:
            valid[at] = False
    return valid


def split(chunk: Chunk, cuts: Sequence[int]) -> List[Chunk]:
    """The chunk cut at the given row indices (ascending; equal neighbours give zero-row chunks)."""
    n = len(chunk[0].values)
    edges = [0] + list(cuts) + [n]
    return [[HCol(c.name, c.dtype, c.values[lo:hi], None if c.valid is None else c.valid[lo:hi]) for c in chunk]
            for lo, hi in zip(edges[:-1], edges[1:])]


def concat(chunks: Sequence[Chunk]) -> Chunk:
    out = []
    for k, c in enumerate(chunks[0]):
        parts = [ch[k] for ch in chunks]
        values = ([v for p in parts for v in p.values] if c.dtype in STRING
                  else np.concatenate([p.values for p in parts]))
        valid = None if c.valid is None else np.concatenate([p.valid for p in parts])
        out.append(HCol(c.name, c.dtype, values, valid))
    return out


def rows(case: Sequence[Chunk]) -> int:
    return sum(len(ch[0].values) for ch in case)


def key_columns(case: Sequence[Chunk], names: Sequence[str]):
    """(cols, valid) of the named columns over the whole case, as tests/group_ref.py ref_table takes them."""
    whole = {c.name: c for c in (concat(case) if len(case) > 1 else case[0])}
    return [(whole[n].dtype, whole[n].values) for n in names], [whole[n].valid for n in names]


def to_device(chunk: Chunk):
    """The chunk as a device Table.  A nullable string column keeps its null slots' payload bytes: it is built from
    all of its strings and then given the case's validity bitmap."""
    import torch

    from deequ_amd.table import Table, column_from_numpy, pack_validity, utf8_column

    cols = []
    for c in chunk:
        if c.dtype in STRING:
            col = utf8_column(c.name, list(c.values), large=c.dtype == "large_utf8", nullable=c.valid is not None)
            if c.valid is not None:
                col.validity = torch.from_numpy(pack_validity(c.valid)).to(col.values.device)
            cols.append(col)
        else:
            cols.append(column_from_numpy(c.name, c.dtype, c.values, c.valid, nullable=c.valid is not None))
    return Table(cols)


def to_device_case(case: Sequence[Chunk]):
    return to_device(case[0]) if len(case) == 1 else [to_device(ch) for ch in case]


# ---------------------------------------------------------------------------------------------------------------
# C.1  multi-tile compaction
# ---------------------------------------------------------------------------------------------------------------
def multi_tile(n: int = MULTI_TILE_ROWS, lone: int = FULL_GRID, wide: int = 50_000, tuples: int = 3000,
               many: int = 1_600_000, few: int = 700, seed: int = 41) -> Chunk:
    """One chunk whose row `lone` is the only row with its value in w, r and (l, i); the last row is valid.
    w: i64, ~`wide` distinct 64-bit values; r: i64 in [0, 299) and 299 at `lone` (9 key bits);
    (l, i): ~`tuples` distinct pairs; (m, j): pairs drawn from `many`; (d, e): `few` frequent pairs, none rare.
    w, r, l, m and d share one validity (~10% nulls); i, j and e have ~3% nulls of their own."""
    rng = np.random.default_rng(seed)
    valid = forced_valid(rng, n, 0.10, keep=(lone, n - 1))
    valid_b = forced_valid(rng, n, 0.03, keep=(lone, n - 1))
    pool = rng.integers(-(1 << 63), (1 << 63) - 1, wide, dtype=np.int64) | 1   # odd: never the lone row's value
    w = pool[rng.integers(0, wide, n)]
    w[lone] = 0x0123_4567_89AB_CDE0
    r = rng.integers(0, 299, n, dtype=np.int64)
    r[lone] = 299
    per = max(1, tuples // 6)
    pick = rng.integers(0, per * 6, n)
    l = pool[pick % per].copy()
    i = (pick // per).astype(np.int32) - 2      # -2 .. 3: negative values in the tuple hash too
    l[lone] = 0x0123_4567_89AB_CDE0
    pick = rng.integers(0, many, n)
    m = pick.astype(np.int64) * 1_000_003 - (1 << 40)
    j = (pick % 5).astype(np.int32)
    pick = rng.integers(0, few, n)
    d = pool[pick % min(wide, few)].copy()
    e = (pick % 7).astype(np.int32)
    return [with_nulls(rng, "w", "i64", w, valid), with_nulls(rng, "r", "i64", r, valid),
            with_nulls(rng, "l", "i64", l, valid), with_nulls(rng, "i", "i32", i, valid_b),
            with_nulls(rng, "m", "i64", m, valid), with_nulls(rng, "j", "i32", j, valid_b),
            with_nulls(rng, "d", "i64", d, valid), with_nulls(rng, "e", "i32", e, valid_b)]


MULTI_TILE_KEYS = [["w"], ["r"], ["l", "i"], ["m", "j"], ["d", "e"]]


# ---------------------------------------------------------------------------------------------------------------
# C.2  the sort's bit range
# ---------------------------------------------------------------------------------------------------------------
V_COMMON = 0x5A5A_0000_1234_5600
FLIP_BITS = (0, 7, 8, 15, 16, 23, 24, 31, 32, 33, 47, 48, 62, 63)


def _i64(u: int) -> int:
    return u - (1 << 64) if u >= 1 << 63 else u


def bit_edges(n: int = 5000, seed: int = 43) -> Dict[str, List[Chunk]]:
    """name -> case over one key column "k" (5% nulls)."""
    rng = np.random.default_rng(seed)

    def col(dtype, values, m=n):
        return [with_nulls(rng, "k", dtype, values, forced_valid(rng, m, 0.05, keep=(0, m - 1)))]

    out: Dict[str, List[Chunk]] = {}
    for v in (0, -1, 1 << 62):
        out[f"all-equal-{v}"] = [col("i64", np.full(n, v, dtype=np.int64))]
    for b in FLIP_BITS:
        pair = np.array([_i64(V_COMMON), _i64(V_COMMON ^ (1 << b))], dtype=np.int64)
        out[f"flip-bit-{b}"] = [col("i64", pair[rng.integers(0, 2, n)])]
    for span in (256, 257):
        vals = (1 << 40) + rng.integers(0, span, n, dtype=np.int64)
        vals[:span] = (1 << 40) + np.arange(span)   # every value of the range occurs
        out[f"base-plus-{span}"] = [col("i64", vals)]
    out["i32-signed"] = [col("i32", rng.integers(-5, 6, n).astype(np.int32) * 100_003)]
    out["i8-signed"] = [col("i8", rng.integers(-128, 128, n).astype(np.int8))]
    out["f64-zeros"] = [col("f64", np.where(rng.random(n) < 0.5, 0.0, -0.0))]
    nan_bits = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,
                         0x7FF4000000000BAD, 0xFFF0000000000001], dtype=np.uint64)
    out["f64-nans"] = [col("f64", nan_bits[rng.integers(0, len(nan_bits), n)].view(np.float64))]
    narrow = col("i64", rng.integers(0, 16, n, dtype=np.int64))
    wide_vals = rng.integers(0, 16, n, dtype=np.int64)
    wide_vals[n // 2] = 1 << 40
    wide = [with_nulls(rng, "k", "i64", wide_vals, forced_valid(rng, n, 0.05, keep=(n // 2,)))]
    out["wide-key-in-later-chunk"] = [narrow, wide]
    out["wide-key-in-first-chunk"] = [wide, narrow]
    return out


# ---------------------------------------------------------------------------------------------------------------
# C.3  the strided representative search
# ---------------------------------------------------------------------------------------------------------------
def strided(n: int, distinct: int, nulls: int, seed: int = 47) -> Chunk:
    """n rows of exactly `distinct` distinct (l, i) pairs, every one of them on at least one non-null row; `nulls`
    rows have a null l."""
    rng = np.random.default_rng(seed + distinct)
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
    valid = np.ones(n, dtype=bool)
    valid[distinct + rng.choice(n - distinct, size=nulls, replace=False)] = False
    order = rng.permutation(n)
    pick, valid = pick[order], valid[order]
    l = (pick // 3).astype(np.int64) * 0x1E37_79B9_7F4A_7C15   # wraps: an odd multiplier keeps the values distinct
    i = (pick % 3).astype(np.int32) - 1
    return [with_nulls(rng, "l", "i64", l, valid), with_nulls(rng, "i", "i32", i, None)]


def many_strings(n: int = 60_000, distinct: int = 20_000, seed: int = 53) -> Chunk:
    rng = np.random.default_rng(seed)
    pool = [b"str-%05d-%s" % (k, b"z" * (k % 23)) for k in range(distinct)]
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
    valid = forced_valid(rng, n, 0.02, keep=range(distinct))   # every string on at least one non-null row
    order = rng.permutation(n)
    return [with_nulls(rng, "s", "utf8", [pool[k] for k in pick[order]], valid[order])]


# ---------------------------------------------------------------------------------------------------------------
# C.4  ragged sizes and null edges
# ---------------------------------------------------------------------------------------------------------------
RAGGED_SIZES = (31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)


def ragged(n: int, seed: int = 59) -> Chunk:
    """k: i64 with nulls; (s, i): short strings x i32; p: i64 without a validity bitmap; z: an all-null i64.
    k, s and i are null at rows 0, 31, 32 and n - 1 (where they exist)."""
    rng = np.random.default_rng(seed + n)
    edge = (0, 31, 32, n - 1)
    words = [b"", b"a", b"b", b"ab", b"ba", b"abc", b"a b", b"\xc3\xa9"]
    k = rng.integers(-9, 10, n, dtype=np.int64) * 1_000_003
    s = [words[x] for x in rng.integers(0, len(words), n)]
    i = rng.integers(-2, 3, n).astype(np.int32)
    p = rng.integers(0, max(2, n // 4), n, dtype=np.int64) - 3
    return [with_nulls(rng, "k", "i64", k, forced_valid(rng, n, 0.2, drop=edge)),
            with_nulls(rng, "s", "utf8", s, forced_valid(rng, n, 0.1, drop=edge)),
            with_nulls(rng, "i", "i32", i, forced_valid(rng, n, 0.1, drop=edge)),
            with_nulls(rng, "p", "i64", p, None),
            with_nulls(rng, "z", "i64", np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool))]


# ---------------------------------------------------------------------------------------------------------------
# C.5  chunk shapes
# ---------------------------------------------------------------------------------------------------------------
def chunk_shapes(seed: int = 61) -> List[Chunk]:
    """64 chunks of 0, 1, 63, 64, 65 or 700 rows (the first, the last and at least one more have none):
    f: f64 (NaN, -0.0, 0.0, nulls); (s, l): strings x wide i64."""
    rng = np.random.default_rng(seed)
    sizes = rng.choice([0, 1, 63, 64, 65, 700], size=64)
    sizes[[0, 17, 18, 40, 63]] = 0
    sizes[[1, 62]] = (1, 700)
    n = int(sizes.sum())
    fpool = np.concatenate([[np.nan, -0.0, 0.0], rng.normal(size=37) * 1e6])
    f = fpool[rng.integers(0, len(fpool), n)]
    spool = [b"k%d-%s" % (k, b"q" * (k % 11)) for k in range(90)]
    s = [spool[x] for x in rng.integers(0, len(spool), n)]
    l = rng.integers(0, 4, n, dtype=np.int64) * 0x0101_0101_0101_0101 - 5
    whole = [with_nulls(rng, "f", "f64", f, forced_valid(rng, n, 0.1)),
             with_nulls(rng, "s", "utf8", s, forced_valid(rng, n, 0.1)),
             with_nulls(rng, "l", "i64", l, forced_valid(rng, n, 0.05))]
    return split(whole, np.cumsum(sizes)[:-1].tolist())


# ---------------------------------------------------------------------------------------------------------------
# C.6  the column limit
# ---------------------------------------------------------------------------------------------------------------
EIGHT = ["c_i64", "c_i32", "c_f64", "c_f32", "c_i16", "c_i8", "c_bool", "c_utf8"]


def nine_columns(n: int = 3000, seed: int = 67) -> Chunk:
    """Eight key columns of eight types (EIGHT) with few values each and 2% nulls each, and a ninth (c_more: i64)."""
    rng = np.random.default_rng(seed)
    f64 = np.array([np.nan, -0.0, 0.0, 1.5])[rng.integers(0, 4, n)]
    f32 = np.array([np.nan, -0.0, 0.0, -2.25], dtype=np.float32)[rng.integers(0, 4, n)]
    utf8 = [[b"", b"x", b"xy"][x] for x in rng.integers(0, 3, n)]
    data = [("c_i64", "i64", rng.integers(-1, 2, n, dtype=np.int64) << 40), ("c_i32", "i32", rng.integers(-1, 2, n)),
            ("c_f64", "f64", f64), ("c_f32", "f32", f32), ("c_i16", "i16", rng.integers(-1, 1, n) * 300),
            ("c_i8", "i8", rng.integers(-1, 1, n) * 100), ("c_bool", "bool", rng.random(n) < 0.5),
            ("c_utf8", "utf8", utf8), ("c_more", "i64", rng.integers(0, 2, n, dtype=np.int64))]
    return [with_nulls(rng, name, dt, vals, forced_valid(rng, n, 0.02)) for name, dt, vals in data]


# ---------------------------------------------------------------------------------------------------------------
# D  Entropy and MutualInformation inputs
# ---------------------------------------------------------------------------------------------------------------
def _from_counts(rng, counts: np.ndarray) -> np.ndarray:
    """Shuffled group ids 0 .. G - 1, id g repeated counts[g] times."""
    return rng.permutation(np.repeat(np.arange(len(counts), dtype=np.int64), counts))


def entropy_cases(seed: int = 71) -> Dict[str, Chunk]:
    """name -> one chunk with the key column "x"."""
    rng = np.random.default_rng(seed)
    out: Dict[str, Chunk] = {}
    out["one-group"] = [HCol("x", "i64", np.full(1000, 7, dtype=np.int64), None)]
    ids = np.zeros(70_001, dtype=np.int64)
    ids[12_345] = 1
    out["dominant-group"] = [HCol("x", "i64", ids * 1_000_003 - 1, None)]
    for G, each in ((2, 500), (3, 333), (1000, 7), (65_537, 2)):
        ids = _from_counts(rng, np.full(G, each))
        if G == 1000:
            out[f"uniform-{G}"] = [HCol("x", "utf8", [b"v%d" % k for k in ids], None)]
        else:
            out[f"uniform-{G}"] = [HCol("x", "i64", ids * 0x10001 - 40_000, None)]
    zipf = np.maximum(1, 30_000 // np.arange(1, 30_001))
    out["zipf-30000"] = [HCol("x", "f64", _from_counts(rng, zipf).astype(np.float64) / 8 - 100.0, None)]
    n = 50_000
    out["nulls-30-percent"] = [with_nulls(rng, "x", "i32", rng.integers(-250, 250, n).astype(np.int32),
                                          forced_valid(rng, n, 0.3))]
    out["singletons-300000"] = [HCol("x", "i64", rng.permutation(300_000).astype(np.int64) * 1_000_003, None)]
    return out


def mi_cases(seed: int = 73) -> Dict[str, Chunk]:
    """name -> one chunk with the columns "x" and "y"."""
    rng = np.random.default_rng(seed)
    out: Dict[str, Chunk] = {}

    def product(ax, by, scale):
        cells = np.outer(ax, by).reshape(-1) * scale
        ids = _from_counts(rng, cells)
        return [HCol("x", "i64", (ids // len(by)) * 1_000_003, None), HCol("y", "i32", (ids % len(by)).astype(np.int32) - 4, None)]

    out["product-7x11-equal"] = product(np.ones(7, np.int64), np.ones(11, np.int64), 13)
    out["product-unequal-marginals"] = product(np.array([1, 2, 3, 5, 8]), np.array([1, 4, 9]), 3)
    n = 30_000
    x = (rng.zipf(1.3, n) % 300).astype(np.int64)
    valid = forced_valid(rng, n, 0.1)
    out["y-equals-x"] = [with_nulls(rng, "x", "i64", x, valid), with_nulls(rng, "y", "i64", x, valid)]
    x = rng.integers(0, 100, 20_000, dtype=np.int64)
    out["y-is-x-mod-3"] = [HCol("x", "i64", x, None), HCol("y", "i8", (x % 3).astype(np.int8), None)]
    n = 100_000
    out["near-independent-200x200"] = [HCol("x", "i32", rng.integers(0, 200, n).astype(np.int32), None),
                                       HCol("y", "i64", rng.integers(0, 200, n, dtype=np.int64) - 100, None)]
    n = 20_000
    x = rng.integers(0, 40, n, dtype=np.int64)
    y = ((x + rng.integers(0, 3, n)) % 10).astype(np.int16)
    out["nulls-in-either"] = [with_nulls(rng, "x", "i64", x, forced_valid(rng, n, 0.2)),
                              with_nulls(rng, "y", "i16", y, forced_valid(rng, n, 0.25))]
    n = 8000
    k = rng.integers(0, 60, n)
    out["string-x-i32"] = [with_nulls(rng, "x", "utf8", [b"name-%d" % v for v in k], forced_valid(rng, n, 0.05)),
                           HCol("y", "i32", ((k * 7 + rng.integers(0, 2, n)) % 9).astype(np.int32), None)]
    fpool = np.array([np.nan, -0.0, 0.0, 1.0, -1.0, 1e300])
    nan2 = np.array([0xFFF8_0000_0000_0001], dtype=np.uint64).view(np.float64)[0]   # a second NaN: the same group
    k = rng.integers(0, len(fpool), n)
    fx = fpool[k]
    fx[(k == 0) & (rng.random(n) < 0.5)] = nan2
    out["f64-x-i64"] = [with_nulls(rng, "x", "f64", fx, forced_valid(rng, n, 0.05)),
                        HCol("y", "i64", (k // 2 + rng.integers(0, 2, n)) << 33, None)]
    out["single-pair-row"] = [HCol("x", "i64", np.array([5], dtype=np.int64), None),
                              HCol("y", "i32", np.array([-5], dtype=np.int32), None)]
    return out
