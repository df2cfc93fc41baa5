"""Dataset match on the device: dq_freq_lookup_rows + dq_rows_match, matching.KeyedRows / DatasetMatch,
Check.doesDatasetMatch and its row-level form.

Every expected value comes from plain Python: a dict from the reference's key tuples (a tuple with a None makes no
key) to its payload tuples.  A probe row applies when the filter keeps it, is found when its key tuple has no None and
is in the dict, and matches when every compare value equals the dict's -- None equals None, None differs from any
value, floats by their bits with every NaN the same and -0.0 and 0.0 apart (as the grouping compares keys)."""
import ctypes
import math
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 2048          # kSplitters in deequ_amd/csrc/dq_probe.hip: the splitters the lookup searches in LDS
MAX_GRID = 2048   # kMatchMaxGrid (and kContainsMaxGrid): workgroups of 4 waves, one 64-row word per wave and step
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd
    from deequ_amd.matching import DatasetMatch, KeyedRows  # noqa: F401

    return deequ_amd


def table(data):
    """Table.from_pydict; a decimal column given as unscaled ints is built from those ints directly."""
    from deequ_amd.table import Table, column_from_numpy

    cols = []
    for name, (dtype, vals) in data.items():
        vals = list(vals)
        if dtype.startswith("decimal(") and all(v is None or isinstance(v, int) for v in vals):
            valid = np.array([v is not None for v in vals], dtype=bool)
            cols.append(column_from_numpy(name, dtype, [0 if v is None else v for v in vals], valid))
        else:
            cols.append(Table.from_pydict({name: (dtype, vals)}).columns[name])
    return Table(cols)


def canon(v):
    if isinstance(v, float):
        if math.isnan(v):
            return ("f", "nan")
        return ("f", struct.unpack("<Q", struct.pack("<d", v))[0])
    if isinstance(v, str):
        return v.encode("utf-8")
    return v


def ref_dict(keys, payload):
    """{key tuple: payload tuple} of the reference rows whose key has no None; the keys must be unique."""
    d = {}
    for k, p in zip(keys, payload):
        if None in k:
            continue
        ck = tuple(canon(v) for v in k)
        assert ck not in d
        d[ck] = tuple(canon(v) for v in p)
    return d


def model(ref, keys, vals, keep=None):
    """Per row (applies, found, matched, [differs per column])."""
    out = []
    for i, (k, v) in enumerate(zip(keys, vals)):
        a = True if keep is None else bool(keep[i])
        hit = ref.get(tuple(canon(x) for x in k)) if a and None not in k else None
        diff = [hit is not None and canon(x) != y for x, y in zip(v, hit)] if hit is not None else [False] * len(v)
        out.append((a, hit is not None, hit is not None and not any(diff), diff))
    return out


def bits_of(t, n):
    return np.unpackbits(t.cpu().numpy(), bitorder="little")[:n].astype(bool)


def filter_bitmap(keep):
    import torch

    n = len(keep)
    raw = np.zeros(((n + 63) // 64 + 1) * 8, dtype=np.uint8)
    packed = np.packbits(np.asarray(keep, dtype=bool), bitorder="little")
    raw[:len(packed)] = packed
    return torch.from_numpy(raw).cuda()


def cols_of(rows, k):
    return [[r[c] for r in rows] for c in range(k)]


def keyed(key_names, key_types, keys, col_names, col_types, payload):
    from deequ_amd.matching import KeyedRows

    data = {n: (t, c) for n, t, c in zip(key_names, key_types, cols_of(keys, len(key_names)))}
    data.update({n: (t, c) for n, t, c in zip(col_names, col_types, cols_of(payload, len(col_names)))})
    kr = KeyedRows.from_data(table(data), key_names, col_names)
    assert kr.num_keys == len(ref_dict(keys, payload)) == kr.payload.num_rows
    assert (kr.key_columns, kr.columns, kr.dtypes) == (tuple(key_names), tuple(col_names), tuple(col_types))
    assert kr.nbytes > 0
    return kr


def check_match(kr, ref, key_names, key_types, keys, col_names, col_types, vals, keep=None, mapping=None):
    """Match the probe rows against `kr` and compare the three bitmaps bit for bit, the tails, and every count."""
    data = {n: (t, c) for n, t, c in zip(key_names, key_types, cols_of(keys, len(key_names)))}
    data.update({n: (t, c) for n, t, c in zip(col_names, col_types, cols_of(vals, len(col_names)))})
    t = table(data)
    mapping = mapping or [(c, c) for c in col_names]
    f = None if keep is None else filter_bitmap(keep)
    r = kr.match_rows(t, key_names, mapping, f, want_found=True, want_applies=True, want_columns=True)
    want = model(ref, keys, vals, keep)
    n = len(keys)
    for name, k in (("applies", 0), ("found", 1), ("matched", 2)):
        assert bits_of(r[name], n).tolist() == [w[k] for w in want], name
        assert not np.unpackbits(r[name].cpu().numpy(), bitorder="little")[n:].any(), name
        assert r["num_" + name] == sum(w[k] for w in want), name
    assert r["mismatch"] == [sum(w[3][c] for w in want) for c in range(len(col_names))]
    # without the per-column counts a row stops at its first difference: the same bitmap
    r2 = kr.match_rows(t, key_names, mapping, f)
    assert bits_of(r2["matched"], n).tolist() == [w[2] for w in want]
    assert (r2["num_matched"], r2["num_found"], r2["num_applies"]) == (r["num_matched"], r["num_found"], r["num_applies"])
    assert r2["found"] is None and r2["applies"] is None and r2["mismatch"] is None
    return r, want


# ---- row and word edges -------------------------------------------------------------------------------------------

EDGE_KEYS = list(range(0, 3000, 3))
EDGE_REF = {(k,): (("f", struct.unpack("<Q", struct.pack("<d", k * 0.5))[0]),) for k in EDGE_KEYS}


@pytest.fixture(scope="module")
def edge_ref(dq):
    return keyed(["k"], ["i64"], [(k,) for k in EDGE_KEYS], ["v"], ["f64"], [(k * 0.5,) for k in EDGE_KEYS])


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 4 * 64 * MAX_GRID + 1])
def test_row_and_word_edges(dq, edge_ref, n, filtered):
    """The last word's tail is zero, a guard word after each bitmap stays, the grid loop wraps once at the last n."""
    import torch

    from deequ_amd import _lib as L
    from deequ_amd import matching
    from deequ_amd.table import Table, column_from_numpy

    rng = np.random.default_rng(n + 7 * filtered)
    k = rng.integers(-10, 3010, size=n)
    kvalid = rng.random(n) < 0.9
    v = k * 0.5
    v[rng.random(n) < 0.1] += 1.0          # a different value
    vvalid = rng.random(n) < 0.95          # a NULL against the reference's value
    keep = (rng.random(n) < 0.7) if filtered else None
    t = Table([column_from_numpy("k", "i64", k, kvalid), column_from_numpy("v", "f64", v, vvalid)])
    keys = [(int(a) if ok else None,) for a, ok in zip(k, kvalid)]
    vals = [(float(a) if ok else None,) for a, ok in zip(v, vvalid)]
    want = model(EDGE_REF, keys, vals, keep)
    f = None if keep is None else filter_bitmap(keep)
    group, _ = matching._lookup(edge_ref.key_set, t, ["k"], f)
    words = (n + 63) // 64
    bufs = [torch.full(((words + 1) * 8,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(3)]
    one = ctypes.c_int32 * 1
    views, pviews = (L.ColumnView * 1)(t.columns["v"].view()), (L.ColumnView * 1)(edge_ref.payload.columns["v"].view())
    counts = [ctypes.c_int64(-5) for _ in range(3)]
    mis = (ctypes.c_int64 * 1)(-5)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib.dq_rows_match(one(L.TYPE_F64), views, one(L.TYPE_F64), pviews, 1, n, edge_ref.payload.num_rows,
                                group.data_ptr(), None if f is None else f.data_ptr(), bufs[0].data_ptr(),
                                bufs[1].data_ptr(), bufs[2].data_ptr(), 0, stream, ctypes.byref(counts[0]),
                                ctypes.byref(counts[1]), ctypes.byref(counts[2]), mis))
    for buf, col, count in ((bufs[0], 2, counts[0]), (bufs[1], 1, counts[1]), (bufs[2], 0, counts[2])):
        raw = buf.cpu().numpy()
        assert (raw[words * 8:] == 0xFF).all(), "guard word touched"
        allbits = np.unpackbits(raw[:words * 8], bitorder="little")
        assert not allbits[n:].any(), "bits past n_rows"
        assert allbits[:n].astype(bool).tolist() == [w[col] for w in want]
        assert count.value == sum(w[col] for w in want)
    assert mis[0] == sum(w[3][0] for w in want)
    assert 0 < sum(w[2] for w in want) or n < 63


def test_no_rows(dq, edge_ref):
    r, _ = check_match(edge_ref, EDGE_REF, ["k"], ["i64"], [], ["v"], ["f64"], [])
    assert (r["num_matched"], r["num_found"], r["num_applies"], r["mismatch"]) == (0, 0, 0, [0])


# ---- group edges --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2, S, S + 1, 5000])
def test_group_edges_i64(dq, G):
    """group[r] is the rank of the key among the table's sorted distinct keys; the first and the last group and the
    keys just outside both ends."""
    keys = [(i - G // 2) * 7 for i in range(G)]
    rng = np.random.default_rng(G)
    order = rng.permutation(G)  # the reference in no particular order
    ref_keys = [(keys[i],) for i in order]
    ref_vals = [(keys[i] * 3 + 1,) for i in order]
    kr = keyed(["k"], ["i64"], ref_keys, ["v"], ["i64"], ref_vals)
    ref = ref_dict(ref_keys, ref_vals)
    probes = [keys[0], keys[-1], keys[0] - 1, keys[-1] + 1, keys[0] + 1, I64_MIN, I64_MAX] + keys + [k + 3 for k in keys]
    vals = [(0,) if abs(p) > 2 ** 40 else (p * 3 + 1 if i % 5 else p * 3 + 2,) for i, p in enumerate(probes)]
    vals[0], vals[1] = (keys[0] * 3 + 1,), (keys[-1] * 3 + 1,)
    r, want = check_match(kr, ref, ["k"], ["i64"], [(p,) for p in probes], ["v"], ["i64"], vals)
    # (the table sorts an i64 key by its 64 value bits, unsigned: the negative keys come after the others)
    rank = {k: i for i, k in enumerate(sorted(keys, key=lambda k: k & (2 ** 64 - 1)))}
    assert r["group"].cpu().tolist() == [rank.get(p, -1) for p in probes]
    assert [w[2] for w in want[:4]] == [True, True, False, False]
    assert sum(w[1] for w in want) == G + 2


@pytest.mark.parametrize("G", [2, S + 1])
def test_group_edges_hashed(dq, G):
    """A hashed key (i64, utf8): group[] is injective over the found keys and payload row group[r] holds r's
    reference row."""
    from tests.helpers import host_column

    ref_keys = [(i, f"s{i % 97}") for i in range(G)] + [(None, "s1"), (1, None)]
    ref_vals = [(f"payload-{i}", i * 2) for i in range(G)] + [("x", 0), ("y", 0)]
    kr = keyed(["a", "b"], ["i64", "utf8"], ref_keys, ["p", "q"], ["utf8", "i64"], ref_vals)
    ref = ref_dict(ref_keys, ref_vals)
    probes = ref_keys[:G] + [(G, "s0"), (-1, "s0"), (0, "s1"), (None, "s1"), (1, None)]
    vals = [(f"payload-{i}", i * 2) for i in range(G)] + [("payload-0", 0)] * 5
    r, want = check_match(kr, ref, ["a", "b"], ["i64", "utf8"], probes, ["p", "q"], ["utf8", "i64"], vals)
    group = r["group"].cpu().tolist()
    assert sorted(group[:G]) == list(range(G)) and group[G:] == [-1] * 5
    pv, _, _ = host_column(kr.payload.columns["p"], G)
    qv, _, _ = host_column(kr.payload.columns["q"], G)
    for i in range(G):
        assert (pv[group[i]], int(qv[group[i]])) == (f"payload-{i}".encode(), i * 2)
    assert all(w[2] for w in want[:G]) and not any(w[1] for w in want[G:])


# ---- NULL rules ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,a,b", [("i64", 5, 6), ("f64", 1.5, 2.5), ("utf8", "x", "y"), ("bool", True, False),
                                       ("decimal(20,4)", 10 ** 19, 10 ** 19 + 1), ("i8", -128, 127)])
def test_null_rules(dq, dtype, a, b):
    ref_keys = [(1,), (2,), (3,), (None,)]
    ref_vals = [(a,), (None,), (b,), (a,)]
    kr = keyed(["k"], ["i64"], ref_keys, ["v"], [dtype], ref_vals)
    ref = ref_dict(ref_keys, ref_vals)
    keys = [(1,), (1,), (1,), (2,), (2,), (3,), (None,), (None,), (4,)]
    vals = [(a,), (None,), (b,), (None,), (a,), (b,), (a,), (None,), (a,)]
    r, want = check_match(kr, ref, ["k"], ["i64"], keys, ["v"], [dtype], vals)
    # value/value, NULL/value, other value, NULL/NULL, value/NULL, value/value; a NULL key is not found and applies
    assert [w[2] for w in want] == [True, False, False, True, False, True, False, False, False]
    assert [w[1] for w in want] == [True] * 6 + [False] * 3
    assert (r["num_applies"], r["num_found"], r["num_matched"], r["mismatch"]) == (9, 6, 3, [3])


def test_garbage_under_null_slots_still_matches(dq):
    """Different bytes under the NULL slots of the two sides: NULL equals NULL whatever lies beneath."""
    from deequ_amd.matching import KeyedRows
    from deequ_amd.table import Table, column_from_numpy

    n = 130
    k = np.arange(n)
    valid = (k % 3 != 0)
    rv = np.where(valid, k * 2, 0x1111111111111111).astype(np.int64)
    pv = np.where(valid, k * 2, 0x2222222222222222).astype(np.int64)
    rf = np.where(valid, k * 0.25, np.nan)
    pf = np.where(valid, k * 0.25, -7.0)
    ref = Table([column_from_numpy("k", "i64", k), column_from_numpy("v", "i64", rv, valid),
                 column_from_numpy("w", "f64", rf, valid)])
    kr = KeyedRows.from_data(ref, "k")
    assert kr.columns == ("v", "w")
    probe = Table([column_from_numpy("k", "i64", k), column_from_numpy("v", "i64", pv, valid),
                   column_from_numpy("w", "f64", pf, valid)])
    r = kr.match_rows(probe, ["k"], [("v", "v"), ("w", "w")], want_columns=True)
    assert (r["num_matched"], r["num_found"], r["num_applies"], r["mismatch"]) == (n, n, n, [0, 0])
    assert bits_of(r["matched"], n).all()


# ---- types --------------------------------------------------------------------------------------------------------

def _pool_case(dq, dtype, pool, seed):
    """Reference row i holds pool[i]; the probe pairs every key with every pool value (and a NULL)."""
    ref_keys = [(i,) for i in range(len(pool))]
    ref_vals = [(v,) for v in pool]
    kr = keyed(["k"], ["i64"], ref_keys, ["v"], [dtype], ref_vals)
    ref = ref_dict(ref_keys, ref_vals)
    keys = [(i,) for i in range(len(pool)) for _ in range(len(pool) + 1)]
    vals = [(v,) for _ in range(len(pool)) for v in list(pool) + [None]]
    r, want = check_match(kr, ref, ["k"], ["i64"], keys, ["v"], [dtype], vals)
    return [w[2] for w in want]


def test_f64_special_values(dq):
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7FF0000000000123))[0]  # another NaN payload: the same value
    pool = [1.5, float("nan"), nan2, 0.0, -0.0, float("inf"), float("-inf"), 5e-324]
    got = _pool_case(dq, "f64", pool, 1)
    m = np.array(got).reshape(len(pool), len(pool) + 1)
    want = np.eye(len(pool), len(pool) + 1, dtype=bool)
    want[1, 2] = want[2, 1] = True  # the two NaNs are equal; +-0.0 and +-inf are not
    assert (m == want).all()


def test_f32_special_values(dq):
    nan2 = struct.unpack("<f", struct.pack("<I", 0x7F800123))[0]
    pool = [1.5, float("nan"), nan2, 0.0, -0.0, float("inf"), float("-inf")]
    m = np.array(_pool_case(dq, "f32", pool, 2)).reshape(len(pool), len(pool) + 1)
    want = np.eye(len(pool), len(pool) + 1, dtype=bool)
    want[1, 2] = want[2, 1] = True
    assert (m == want).all()


@pytest.mark.parametrize("dtype,lo,hi", [("i64", I64_MIN, I64_MAX), ("i32", -2 ** 31, 2 ** 31 - 1),
                                         ("i16", -2 ** 15, 2 ** 15 - 1), ("i8", -128, 127),
                                         ("date32", -2 ** 31, 2 ** 31 - 1), ("timestamp", I64_MIN, I64_MAX)])
def test_fixed_width_extremes(dq, dtype, lo, hi):
    pool = [lo, hi, lo + 1, hi - 1, -1, 0, 1]
    m = np.array(_pool_case(dq, dtype, pool, 3)).reshape(len(pool), len(pool) + 1)
    assert (m == np.eye(len(pool), len(pool) + 1, dtype=bool)).all()


def test_bool_at_word_edges(dq):
    """Bit-packed on both sides: rows 31, 32, 63, 64 of the probe against payload rows in another bit position."""
    n = 130
    ref_keys = [(i,) for i in range(n)]
    ref_vals = [(i % 3 == 0,) for i in range(n)]
    kr = keyed(["k"], ["i64"], ref_keys, ["v"], ["bool"], ref_vals)
    ref = ref_dict(ref_keys, ref_vals)
    keys = [((i * 37) % n,) for i in range(n)]  # probe row i reads payload row (37 i) mod n
    vals = [((k[0] % 3 == 0) != (i in (31, 32, 63, 64, 129)),) for i, k in enumerate(keys)]
    r, want = check_match(kr, ref, ["k"], ["i64"], keys, ["v"], ["bool"], vals)
    assert [i for i, w in enumerate(want) if not w[2]] == [31, 32, 63, 64, 129]


@pytest.mark.parametrize("dtype,pool", [("decimal(9,2)", [0, 1, -1, 99999, 10 ** 9 - 1, 1 - 10 ** 9]),
                                        ("decimal(20,4)", [0, 2 ** 64, 2 ** 64 + 1, -2 ** 64, 10 ** 20 - 1, 2 ** 65]),
                                        ("decimal(38,0)", [10 ** 37, 10 ** 37 + 2 ** 64, -10 ** 37, 10 ** 38 - 1,
                                                           1 - 10 ** 38, 2 ** 64, 2 ** 65, 0])])
def test_decimal(dq, dtype, pool):
    """Unscaled integers that differ only in the high word, or only in the low one."""
    m = np.array(_pool_case(dq, dtype, pool, 4)).reshape(len(pool), len(pool) + 1)
    assert (m == np.eye(len(pool), len(pool) + 1, dtype=bool)).all()


# ---- strings ------------------------------------------------------------------------------------------------------

STRINGS = ["", "a", "b", "x" * 300, "x" * 299 + "y", "x" * 299, "prefix", "prefi", "prefix-longer", "café", "z" * 8,
           "z" * 12, "z" * 9]


@pytest.mark.parametrize("ref_type,probe_type", [("utf8", "utf8"), ("utf8", "large_utf8"), ("large_utf8", "utf8"),
                                                 ("large_utf8", "large_utf8"), ("utf8", "dict_utf8"),
                                                 ("dict_utf8", "utf8")])
def test_strings(dq, ref_type, probe_type):
    """The empty string against NULL, values that differ in the last of 300 bytes, in length only, a prefix of the
    reference; both offset widths on either side; a dictionary-encoded column on either side; the chunk's last row
    against the last payload row."""
    n = len(STRINGS)
    ref_keys = [(i,) for i in range(n + 1)]
    ref_vals = [(None,)] + [(s,) for s in STRINGS]  # (the last payload row holds the last string)
    kr = keyed(["k"], ["i64"], ref_keys, ["s"], [ref_type], ref_vals) if ref_type != "dict_utf8" else None
    if kr is None:  # (a dictionary payload column is kept as its decoded column)
        from deequ_amd.matching import KeyedRows

        kr = KeyedRows.from_data(table({"k": ("i64", [k[0] for k in ref_keys]),
                                        "s": ("dict_utf8", [v[0] for v in ref_vals])}), "k")
        assert kr.dtypes == ("utf8",)
    ref = ref_dict(ref_keys, ref_vals)
    keys = [(i,) for i in range(n + 1) for _ in range(n + 1)]
    vals = [(v,) for _ in range(n + 1) for v in STRINGS + [None]]
    keys.append((n,))   # the last row of the chunk against the last payload row, and equal
    vals.append((STRINGS[-1],))
    data = {"k": ("i64", [k[0] for k in keys]), "s": (probe_type, [v[0] for v in vals])}
    t = table(data)
    r = kr.match_rows(t, ["k"], [("s", "s")], want_found=True, want_columns=True)
    want = model(ref, keys, vals)
    assert bits_of(r["matched"], len(keys)).tolist() == [w[2] for w in want]
    assert [w[2] for w in want[:-1]] == [rv[0] == v for rv in ref_vals for v in STRINGS + [None]]  # "" != NULL
    assert sum(w[2] for w in want[:-1]) == n + 1 and want[-1][2]
    assert r["group"].cpu().tolist()[-1] == kr.payload.num_rows - 1 == n
    assert r["mismatch"] == [sum(w[3][0] for w in want)] and r["num_found"] == len(keys)


# ---- counts -------------------------------------------------------------------------------------------------------

COUNT_NAMES, COUNT_TYPES = ["amount", "name", "day", "flag"], ["f64", "utf8", "date32", "bool"]


def _count_rows(n):
    return [(i * 0.5, f"name-{i}", i % 400, i % 2 == 0) for i in range(n)]


def test_counts_and_breakdown(dq):
    from deequ_amd.matching import DatasetMatch

    G, n = 700, 1000
    ref_keys = [(i,) for i in range(G)]
    ref_vals = _count_rows(G)
    kr = keyed(["id"], ["i64"], ref_keys, COUNT_NAMES, COUNT_TYPES, ref_vals)
    ref = ref_dict(ref_keys, ref_vals)
    keys = [(None,) if i % 50 == 7 else (i,) for i in range(n)]  # 700 .. 999 are missing, 14 of the found are NULL keys
    vals = [list(v) for v in _count_rows(n)]
    planted = {0: [3, 64, 65, 699], 1: [3, 100], 2: [200, 201, 202], 3: [3, 63, 699]}
    for c, rows in planted.items():
        for i in rows:
            v = vals[i][c]
            vals[i][c] = v + 1.0 if c == 0 else v + "!" if c == 1 else v + 1 if c == 2 else not v
    vals[300][1] = None  # a NULL against a value
    vals = [tuple(v) for v in vals]
    r, want = check_match(kr, ref, ["id"], ["i64"], keys, COUNT_NAMES, COUNT_TYPES, vals)
    assert r["mismatch"] == [4, 3, 3, 3]
    data = {"id": ("i64", [k[0] for k in keys])}
    data.update({nm: (dt, col) for nm, dt, col in zip(COUNT_NAMES, COUNT_TYPES, cols_of(vals, 4))})
    a = DatasetMatch("id", None, kr)
    b = a.breakdown(table(data))
    different = {i for rows in planted.values() for i in rows} | {300}
    assert b == {"matched": 700 - 14 - len(different), "key_missing": 300 + 14, "value_mismatch": len(different),
                 "applies": n, "mismatch_by_column": dict(zip(COUNT_NAMES, [4, 3, 3, 3]))}
    assert b["matched"] + b["value_mismatch"] + b["key_missing"] == b["applies"]
    # a renamed column: the dict form, named as the data names it
    data["label"] = data.pop("name")
    b2 = DatasetMatch("id", {"label": "name", "flag": "flag"}, kr).breakdown(table(data))
    assert b2["mismatch_by_column"] == {"label": 3, "flag": 3}


# ---- a found hash is compared by value ---------------------------------------------------------------------------

def test_forged_hash_is_key_missing(dq):
    """The forged image of test_refint_gpu.py's collision test: a group that keeps the hash of "value-a" and stores
    "value-b".  Looking "value-a" up finds the hash, compares the tuple, and gives -1: key_missing, no error."""
    from deequ_amd import matching
    from deequ_amd.matching import DatasetMatch, KeyedRows, KeySet

    vals = ["value-a", "other-1", "other-2", "other-3"]
    kr = keyed(["s"], ["utf8"], [(v,) for v in vals], ["p"], ["i64"], [(i,) for i in range(4)])
    image = kr.key_set.to_bytes()
    assert image.count(b"value-a") == 1
    forged = KeyedRows(KeySet.from_bytes(image.replace(b"value-a", b"value-b"), ["s"]), kr.payload)
    rows = ["value-a", "value-b", "other-1", "other-2", "other-3", None]
    t = table({"s": ("utf8", rows), "p": ("i64", [0, 0, 1, 2, 3, 0])})
    good, _ = matching._lookup(kr.key_set, t, ["s"])
    group, nf = matching._lookup(forged.key_set, t, ["s"])
    assert (good[:6] >= 0).cpu().tolist() == [True, False, True, True, True, False]
    assert group[:6].cpu().tolist() == [-1, -1] + good[2:5].cpu().tolist() + [-1] and nf == 3
    b = DatasetMatch("s", ["p"], forged).breakdown(t)
    assert (b["matched"], b["key_missing"], b["value_mismatch"], b["applies"]) == (3, 3, 0, 6)


# ---- refusals: before any launch ----------------------------------------------------------------------------------

def test_refusals(dq):
    from deequ_amd import DatasetMatch, KeyedRows, matching
    from deequ_amd.repository import deserialize_analyzer, serialize_analyzer

    ref = table({"k": ("i64", [1, 2, 3]), "v": ("i64", [10, 20, 30]), "d": ("decimal(10,2)", [100, 200, 300])})
    kr = KeyedRows.from_data(ref, "k")
    # a duplicate reference key (the message carries the count), a chunked reference, no compare column
    before = (matching.lookup_calls, matching.match_calls, matching.probe_calls)
    dup = table({"k": ("i64", [1, 2, 2, 3, 3, 3, None, None]), "v": ("i64", list(range(8)))})
    with pytest.raises(ValueError, match="2 keys of the reference occur on more than one"):
        KeyedRows.from_data(dup, "k")
    assert matching.match_calls == before[1]
    before = (matching.lookup_calls, matching.match_calls, matching.probe_calls)
    with pytest.raises(ValueError, match="one table, got 2 chunks"):
        KeyedRows.from_data([ref, ref], "k")
    with pytest.raises(ValueError, match="at least one column to compare"):
        KeyedRows.from_data(ref, ["k", "v", "d"])
    with pytest.raises(ValueError, match="at least one column to compare"):
        KeyedRows.from_data(ref, "k", [])
    wide = table({"k": ("i64", [1]), **{f"c{i}": ("i64", [i]) for i in range(17)}})
    kw = KeyedRows.from_data(wide, "k")
    after_build = (matching.lookup_calls, matching.match_calls, matching.probe_calls)
    assert after_build == (before[0] + 1, before[1], before[2])  # (the wide reference's own lookup)
    probe = table({"k": ("i64", [1, 2]), "k32": ("i32", [1, 2]), "v": ("i64", [10, 21]), "v32": ("i32", [10, 20]),
                   "d3": ("decimal(10,3)", [1000, 2000])})
    cases = [(DatasetMatch("k", {"v32": "v"}, kr), "column v32 to be i64.*found i32"),
             (DatasetMatch("k32", ["v"], kr), "column k32 to be i64.*found i32"),
             (DatasetMatch("k", {"d3": "d"}, kr), r"column d3 to be decimal\(10,2\).*found decimal\(10,3\)"),
             (DatasetMatch(["k", "v"], ["v"], kr), "2 columns .* key set over 1"),
             (DatasetMatch("k", ["nope"], kr), "does not include column nope"),
             (DatasetMatch("nope", ["v"], kr), "does not include column nope"),
             (DatasetMatch("k", None, kw), "compares 1 to 16 columns, got 17"),
             (deserialize_analyzer(serialize_analyzer(DatasetMatch("k", ["v"], kr))), "loaded from a metrics repository")]
    import re

    for a, text in cases:
        data = wide if a.reference is kw else probe
        m = a.calculate(data)
        assert m.value.isFailure and re.search(text, str(m.value.failed)), (str(a), m.value)
        with pytest.raises(Exception, match=text):
            a.breakdown(data)
    assert (matching.lookup_calls, matching.match_calls, matching.probe_calls) == after_build
    assert DatasetMatch("k", ["v"], kr).calculate(probe).value.get() == 0.5  # (and the good one runs)


# ---- end to end ---------------------------------------------------------------------------------------------------

def _feed(n=1000, seed=9):
    rng = np.random.default_rng(seed)
    cid = [None if rng.random() < 0.05 else int(rng.integers(0, 150)) for _ in range(n)]
    amount = [None if rng.random() < 0.05 else float(c if c is not None else 0) + (0.5 if rng.random() < 0.1 else 0.0)
              for c in cid]
    note = [None if c is None else (f"n{c % 13}" if rng.random() < 0.9 else "other") for c in cid]
    return cid, amount, note


MASTER_KEYS = [(i,) for i in range(0, 150, 3)] + [(None,)]
MASTER_VALS = [(float(i), f"n{i % 13}") for i in range(0, 150, 3)] + [(0.0, "x")]
MASTER = ref_dict(MASTER_KEYS, MASTER_VALS)


def _feed_table(cid, amount, note, lo=0, hi=None):
    return table({"cid": ("i64", cid[lo:hi]), "amount": ("f64", amount[lo:hi]), "note": ("utf8", note[lo:hi])})


def _expected(cid, amount, note, where=False):
    keep = None if not where else [a is not None and a > 0 for a in amount]
    return model(MASTER, [(c,) for c in cid], list(zip(amount, note)), keep)


@pytest.fixture(scope="module")
def master(dq):
    return keyed(["id"], ["i64"], MASTER_KEYS, ["amount", "note"], ["f64", "utf8"], MASTER_VALS)


def test_check_over_chunks_arrow_where_and_incremental(dq, master):
    pa = pytest.importorskip("pyarrow")
    from deequ_amd import (AnalysisRunner, Check, CheckLevel, CheckStatus, DatasetMatch, InMemoryStateProvider,
                           ReferentialIntegrity, VerificationSuite, matching)

    cid, amount, note = _feed()
    want, wantw = _expected(cid, amount, note), _expected(cid, amount, note, where=True)
    nm, na = sum(w[2] for w in want), sum(w[0] for w in want)
    wm, wa = sum(w[2] for w in wantw), sum(w[0] for w in wantw)
    nf = sum(w[1] for w in want)
    assert 0 < wm <= nm < nf < na and wa < na
    whole = _feed_table(cid, amount, note)
    cuts = [(0, 300), (300, 301), (301, None)]
    chunks = [_feed_table(cid, amount, note, lo, hi) for lo, hi in cuts]
    batches = [pa.record_batch({"cid": pa.array(cid[lo:hi], pa.int64()), "amount": pa.array(amount[lo:hi], pa.float64()),
                                "note": pa.array(note[lo:hi], pa.string())}) for lo, hi in cuts]
    cols = ["amount", "note"]
    check = (Check(CheckLevel.Error, "feed").doesDatasetMatch("cid", cols, master, lambda v: v == nm / na)
             .doesDatasetMatch("cid", cols, master, lambda v: v == wm / wa).where("amount > 0")
             .hasReferentialIntegrity("cid", master.key_set, lambda v: v == nf / na))
    plain, filtered = DatasetMatch("cid", cols, master), DatasetMatch("cid", cols, master, "amount > 0")
    for data, n_chunks in ((whole, 1), (chunks, 3), (batches, 3)):
        before = (matching.lookup_calls, matching.match_calls, matching.probe_calls)
        r = VerificationSuite().onData(data).addCheck(check).run()
        assert (matching.lookup_calls - before[0], matching.match_calls - before[1]) == (2 * n_chunks, 2 * n_chunks)
        assert matching.probe_calls - before[2] == n_chunks  # (the referential-integrity check beside them)
        assert r.status == CheckStatus.Success, [c.message for cr in r.checkResults.values() for c in cr.constraintResults]
        assert r.metrics[plain].value.get() == nm / na
        assert r.metrics[filtered].value.get() == wm / wa
        assert r.metrics[ReferentialIntegrity("cid", master.key_set)].value.get() == nf / na
        m = r.metrics[plain]
        assert (m.name, m.instance, m.entity.value) == ("DatasetMatch", "cid,amount,note", "Mutlicolumn")
    # an incremental run over two halves equals the whole; the saved states aggregate without data
    half, rest = InMemoryStateProvider(), InMemoryStateProvider()
    first, second = _feed_table(cid, amount, note, 0, 500), _feed_table(cid, amount, note, 500, None)
    for a in (plain, filtered):
        a.calculate(first, saveStatesWith=half)
    for a, ratio in ((plain, nm / na), (filtered, wm / wa)):
        assert a.calculate(second, aggregateWith=half).value.get() == ratio
        a.calculate(second, saveStatesWith=rest)
    ctx = AnalysisRunner.runOnAggregatedStates(whole, [plain, filtered], [half, rest])
    assert (ctx.metric(plain).value.get(), ctx.metric(filtered).value.get()) == (nm / na, wm / wa)
    # a where that keeps no row: the empty state
    assert DatasetMatch("cid", cols, master, "amount > 100000").calculate(whole).value.isFailure


@pytest.mark.parametrize("filteredRow", ["TRUE", "NULL"])
def test_failing_rows_are_the_missing_and_the_different(dq, master, filteredRow):
    from deequ_amd import Check, CheckLevel
    from deequ_amd.rowlevel import row_level_results

    cid, amount, note = _feed(500, seed=10)
    chunks = [_feed_table(cid, amount, note, 0, 200), _feed_table(cid, amount, note, 200, None)]
    check = (Check(CheckLevel.Error, "feed").doesDatasetMatch("cid", ["amount", "note"], master)
             .doesDatasetMatch("cid", ["amount", "note"], master).where("amount > 0"))
    res = row_level_results([check], chunks, filteredRow)
    assert not res.skipped
    plain, filtered = [str(c) for c in check.constraints]
    for name, where in ((plain, False), (filtered, True)):
        want = _expected(cid, amount, note, where)
        a, c = [w[0] for w in want], [w[2] for w in want]
        failing = [i for i in range(500) if a[i] and not c[i]]
        assert any(want[i][1] for i in failing) and any(not want[i][1] for i in failing)  # different, and missing
        got = res.failing_rows(name)
        rows = [(x, y, z) for t in got for x, y, z in zip(_host(t, "cid"), _host(t, "amount"), _host(t, "note"))]
        assert rows == [(cid[i], amount[i], note[i]) for i in failing]
        vals = res.as_bool(name)
        if filteredRow == "NULL" and where:
            assert (~np.ma.getmaskarray(vals)).tolist() == a
            assert np.ma.getdata(vals)[np.array(a)].tolist() == [c[i] for i in range(500) if a[i]]
        else:
            assert np.asarray(vals).tolist() == [c[i] or not a[i] for i in range(500)]


def _host(t, name):
    """A taken column as Python values: None for NULL, str for strings."""
    from tests.helpers import host_column

    vals, valid, _ = host_column(t.columns[name], t.num_rows)
    return [None if not ok else v.decode("utf-8") if isinstance(v, bytes) else v.item() for v, ok in zip(vals, valid)]
