"""Referential integrity on the device: dq_freq_contains_rows, matching.KeySet / ReferentialIntegrity,
Check.hasReferentialIntegrity and its row-level form.

Every expected value comes from plain Python: a set of tuples over the reference table's rows (a tuple with a None
makes no key), a probe tuple with a None is not contained, and a row applies when the filter keeps it.  Floats are
compared as the grouping compares them: by their bits, every NaN the same, -0.0 and 0.0 apart."""
import ctypes
import math
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 2048          # kSplitters in deequ_amd/csrc/dq_probe.hip: the splitters the probe kernel searches in LDS
MAX_GRID = 2048   # kContainsMaxGrid: workgroups of 4 waves, one 64-row word per wave and grid-loop step
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd
    from deequ_amd import matching  # noqa: F401

    return deequ_amd


def table(data):
    """Table.from_pydict; a decimal column given as unscaled ints (38 digits: beyond from_pydict's Decimal context)
    is built from those ints directly."""
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
        return ("f", 0x7FF8000000000000 if math.isnan(v) else struct.unpack("<Q", struct.pack("<d", v))[0])
    if isinstance(v, str):
        return v.encode("utf-8")
    return v


def key_set_of(ref_rows):
    return {tuple(canon(v) for v in t) for t in ref_rows if None not in t}


def model(ref_rows, probe_rows, keep=None):
    """(contained, applies) as lists of bool."""
    keys = key_set_of(ref_rows)
    applies = [True if keep is None else bool(keep[i]) for i in range(len(probe_rows))]
    contained = [a and None not in t and tuple(canon(v) for v in t) in keys for a, t in zip(applies, probe_rows)]
    return contained, applies


def bits_of(t, n):
    return np.unpackbits(t.cpu().numpy(), bitorder="little")[:n].astype(bool)


def filter_bitmap(keep):
    import torch

    n = len(keep)
    words = (n + 63) // 64
    raw = np.zeros((words + 1) * 8, dtype=np.uint8)
    packed = np.packbits(np.asarray(keep, dtype=bool), bitorder="little")
    raw[:len(packed)] = packed
    return torch.from_numpy(raw).cuda()


def columns_of(rows, names):
    return [[t[c] for t in rows] for c in range(len(names))]


def check_probe(ks, dtypes, names, ref_rows, probe_rows, keep=None, probe_dtypes=None):
    """Probe `probe_rows` against `ks` and compare both bitmaps bit for bit and both counts with the model."""
    pd = probe_dtypes or dtypes
    t = table({nm: (dt, col) for nm, dt, col in zip(names, pd, columns_of(probe_rows, names))})
    f = None if keep is None else filter_bitmap(keep)
    contained, applies, nc, na = ks.contains_rows(t, names, f, want_applies=True)
    want_c, want_a = model(ref_rows, probe_rows, keep)
    n = len(probe_rows)
    assert bits_of(contained, n).tolist() == want_c
    assert bits_of(applies, n).tolist() == want_a
    assert nc == sum(want_c) and na == sum(want_a)
    assert not np.unpackbits(contained.cpu().numpy(), bitorder="little")[n:].any()
    assert not np.unpackbits(applies.cpu().numpy(), bitorder="little")[n:].any()
    return want_c


def build(dq, dtypes, names, ref_rows):
    from deequ_amd.matching import KeySet

    ref = table({nm: (dt, col) for nm, dt, col in zip(names, dtypes, columns_of(ref_rows, names))})
    ks = KeySet.from_data(ref, names)
    assert ks.num_keys == len(key_set_of(ref_rows))
    return ks


# ---- search edges: a single i64 column --------------------------------------------------------------------------

def strided_keys(G, extremes):
    keys = [(i - G // 2) * 7 for i in range(G)]  # negative and positive, a gap of 6 between neighbours
    if extremes and G >= 2:
        keys[0], keys[-1] = I64_MIN, I64_MAX
    return keys


@pytest.mark.parametrize("extremes", [False, True])
@pytest.mark.parametrize("G", [0, 1, 2, S - 1, S, S + 1, 2 * S + 1, 70_000])
def test_search_edges_i64(dq, G, extremes):
    keys = strided_keys(G, extremes)
    ks = build(dq, ["i64"], ["k"], [(k,) for k in keys])
    # every key (the first, the last and every splitter keys[b * G // S] among them), both neighbours of every key in
    # value (every gap; below the minimum, above the maximum) and the extremes of the type
    probes = set(keys) | {k - 1 for k in keys} | {k + 1 for k in keys} | {k + 3 for k in keys}
    probes |= {I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX, 0, -1, 1}
    if keys:
        probes |= {min(keys) - 100, max(keys) + 100}
    probes = sorted(p for p in probes if I64_MIN <= p <= I64_MAX)
    rng = np.random.default_rng(G)
    probes = [probes[i] for i in rng.permutation(len(probes))]
    want = check_probe(ks, ["i64"], ["k"], [(k,) for k in keys], [(p,) for p in probes])
    assert sum(want) == G
    if G:  # the splitters and their neighbours in key order, named
        n_split = min(S, G)
        idx = sorted({j for b in range(n_split) for j in (b * G // n_split - 1, b * G // n_split, b * G // n_split + 1)
                      if 0 <= j < G})
        sorted_keys = sorted(keys)
        check_probe(ks, ["i64"], ["k"], [(k,) for k in keys], [(sorted_keys[j],) for j in idx])


# ---- row edges ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 64 * 4 * MAX_GRID + 1])
def test_row_edges(dq, n):
    """The last word's tail is zero, a guard word after each bitmap stays, the grid loop wraps once at the last n."""
    import torch

    from deequ_amd import _lib as L

    keys = list(range(0, 3000, 3))
    ks = build(dq, ["i64"], ["k"], [(k,) for k in keys])
    rng = np.random.default_rng(n + 1)
    vals = rng.integers(-10, 3010, size=n).tolist()
    valid = (rng.random(n) < 0.9).tolist()
    rows = [(v if ok else None,) for v, ok in zip(vals, valid)]
    keep = (rng.random(n) < 0.7).tolist()
    t = table({"k": ("i64", [r[0] for r in rows])})
    words = (n + 63) // 64
    bufs = [torch.full(((words + 1) * 8,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(2)]
    f = filter_bitmap(keep)
    types = (ctypes.c_int32 * 1)(L.TYPE_I64)
    views = (L.ColumnView * 1)(t.columns["k"].view())
    nc, na = ctypes.c_int64(-5), ctypes.c_int64(-5)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib.dq_freq_contains_rows(ks.table.handle, types, views, n, f.data_ptr(), bufs[0].data_ptr(),
                                        bufs[1].data_ptr(), stream, ctypes.byref(nc), ctypes.byref(na)))
    want_c, want_a = model([(k,) for k in keys], rows, keep)
    for buf, want, count in ((bufs[0], want_c, nc.value), (bufs[1], want_a, na.value)):
        raw = buf.cpu().numpy()
        assert (raw[words * 8:] == 0xFF).all(), "guard word touched"
        allbits = np.unpackbits(raw[:words * 8], bitorder="little")
        assert not allbits[n:].any(), "bits past n_rows"
        assert allbits[:n].astype(bool).tolist() == want
        assert count == sum(want)


# ---- NULLs and filters --------------------------------------------------------------------------------------------

REF3 = [(i, f"s{i % 7}", i % 5) for i in range(40)] + [(None, "s1", 1), (3, None, 3), (4, "s4", None)]
TYPES3, NAMES3 = ["i64", "utf8", "date32"], ["a", "b", "c"]


def test_nulls_in_key_columns(dq):
    ks = build(dq, TYPES3, NAMES3, REF3)
    hit = (5, "s5", 0)
    assert hit in REF3
    rows = [hit, (None, "s5", 0), (5, "s5", None), (None, None, None), (5, None, 0), hit, (5, "s6", 0),
            (None, "s1", 1), (3, None, 3), (4, "s4", None)]  # (the reference's own NULL rows made no key)
    want = check_probe(ks, TYPES3, NAMES3, REF3, rows)
    assert want == [True, False, False, False, False, True, False, False, False, False]
    # an all-NULL chunk: nothing contained, every row in the denominator
    nulls = [(None, None, None)] * 130
    t = table({nm: (dt, col) for nm, dt, col in zip(NAMES3, TYPES3, columns_of(nulls, NAMES3))})
    _, _, nc, na = ks.contains_rows(t, NAMES3, None, want_applies=True)
    assert (nc, na) == (0, 130)
    check_probe(ks, TYPES3, NAMES3, REF3, nulls)


@pytest.mark.parametrize("keep", ["none", "all", "alternate"])
def test_filter(dq, keep):
    keys = list(range(0, 400, 2))
    ks = build(dq, ["i64"], ["k"], [(k,) for k in keys])
    rows = [(None if i % 11 == 0 else i,) for i in range(333)]
    mask = {"none": [False] * 333, "all": [True] * 333, "alternate": [i % 2 == 0 for i in range(333)]}[keep]
    check_probe(ks, ["i64"], ["k"], [(k,) for k in keys], rows, mask)


# ---- types --------------------------------------------------------------------------------------------------------

N_TYPES = 2000


def _mix(rng, pool, n=N_TYPES, null_rate=0.05):
    return [None if rng.random() < null_rate else pool[int(rng.integers(len(pool)))] for _ in range(n)]


def test_f64_special_values(dq):
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7FF0000000000123))[0]  # another NaN payload: the same key
    ref = [(1.5,), (float("nan"),), (0.0,), (float("inf"),), (-2.25,), (None,)]
    ks = build(dq, ["f64"], ["x"], ref)
    rng = np.random.default_rng(1)
    pool = [1.5, float("nan"), nan2, 0.0, -0.0, float("inf"), float("-inf"), -2.25, 2.25, 1e300]
    rows = [(v,) for v in _mix(rng, pool)]
    check_probe(ks, ["f64"], ["x"], ref, rows)
    want = model(ref, [(nan2,), (-0.0,), (float("-inf"),), (0.0,)])[0]
    assert want == [True, False, False, True]
    # the other sign of zero and of infinity as keys
    ref2 = [(-0.0,), (float("-inf"),)]
    ks2 = build(dq, ["f64"], ["x"], ref2)
    check_probe(ks2, ["f64"], ["x"], ref2, rows)


@pytest.mark.parametrize("dtype,lo,hi", [("i32", -2 ** 31, 2 ** 31 - 1), ("i16", -2 ** 15, 2 ** 15 - 1),
                                         ("i8", -128, 127), ("date32", -2 ** 31, 2 ** 31 - 1),
                                         ("timestamp", I64_MIN, I64_MAX)])
def test_fixed_width_types(dq, dtype, lo, hi):
    rng = np.random.default_rng(len(dtype))
    span = min(hi, 200)
    ref = [(v,) for v in [lo, hi, -1, 0, 5] + rng.integers(-span, span, size=60).tolist()] + [(None,)]
    ks = build(dq, [dtype], ["x"], ref)
    pool = [lo, hi, lo + 1, hi - 1, -1, 0, 1, 5, 6] + rng.integers(-span, span, size=100).tolist()
    check_probe(ks, [dtype], ["x"], ref, [(v,) for v in _mix(rng, pool)])


def test_bool(dq):
    rng = np.random.default_rng(3)
    rows = [(v,) for v in _mix(rng, [True, False])]
    for ref in ([(True,), (None,)], [(False,)], [(True,), (False,)], [(None,)]):
        ks = build(dq, ["bool"], ["x"], ref)
        check_probe(ks, ["bool"], ["x"], ref, rows)


@pytest.mark.parametrize("dtype", ["decimal(10,2)", "decimal(38,0)"])
def test_decimal(dq, dtype):
    from decimal import Decimal

    rng = np.random.default_rng(4)
    if dtype == "decimal(10,2)":
        pool = [Decimal("0.00"), Decimal("-0.01"), Decimal("99999999.99"), Decimal("-99999999.99"), Decimal("1.10"),
                Decimal("1.11"), Decimal("12.34")]
    else:  # unscaled integers that differ only in the high word, or only in the low one
        pool = [10 ** 37, 10 ** 37 + 1, -10 ** 37, 10 ** 38 - 1, 1 - 10 ** 38, 2 ** 64, 2 ** 64 + 1, 2 ** 65, 1, 0, -1]
    ref = [(v,) for v in pool[::2]] + [(None,)]
    ks = build(dq, [dtype], ["x"], ref)
    assert ks.dtypes == (dtype,)
    check_probe(ks, [dtype], ["x"], ref, [(v,) for v in _mix(rng, pool)])


STRINGS = ["", "a", "b", "x" * 300, "x" * 299 + "y", "x" * 299, "prefix", "prefi", "prefix-longer", "same-head-A",
           "same-head-B", "café", "z"]


@pytest.mark.parametrize("ref_type,probe_type", [("utf8", "utf8"), ("utf8", "large_utf8"), ("large_utf8", "utf8"),
                                                 ("utf8", "dict_utf8")])
def test_strings(dq, ref_type, probe_type):
    """The empty string, one byte, 300 bytes, strings that differ in the last byte only, prefixes of one another; the
    other offset width on either side; a dictionary-encoded primary column against a plain-string key set."""
    rng = np.random.default_rng(5)
    ref = [(s,) for s in STRINGS[::2]] + [(None,)]
    ks = build(dq, [ref_type], ["s"], ref)
    rows = [(v,) for v in _mix(rng, STRINGS)]
    want = check_probe(ks, [ref_type], ["s"], ref, rows, probe_dtypes=[probe_type])
    assert 0 < sum(want) < len(rows)


def test_tuple_i64_utf8_date32(dq):
    rng = np.random.default_rng(6)
    ks = build(dq, TYPES3, NAMES3, REF3)
    rows = [(None if rng.random() < 0.05 else int(rng.integers(0, 45)),
             None if rng.random() < 0.05 else f"s{int(rng.integers(0, 8))}",
             None if rng.random() < 0.05 else int(rng.integers(0, 6))) for _ in range(N_TYPES)]
    rows[:40] = [t for t in REF3[:40]]
    want = check_probe(ks, TYPES3, NAMES3, REF3, rows)
    assert sum(want) >= 40


# ---- a found hash is compared by value ---------------------------------------------------------------------------

def test_equal_hash_different_value_is_not_contained(dq):
    """dq_freq_from_bytes checks an image's structure and does not re-hash (dq_freq_image.cpp: magic, sizes, ascending
    keys, offsets), so an image whose group keeps the hash of "value-a" and stores "value-b" loads: probing "value-a"
    finds the hash and must compare the tuple -- not contained; so is "value-b" (its hash is no key); the untouched
    groups are contained.  A kernel that trusts the hash reports "value-a" as contained."""
    from deequ_amd.matching import KeySet

    vals = ["value-a", "other-1", "other-2", "other-3"]
    ks = build(dq, ["utf8"], ["s"], [(v,) for v in vals])
    rows = [("value-a",), ("value-b",), ("other-1",), ("other-2",), ("other-3",), (None,)]
    t = table({"s": ("utf8", [r[0] for r in rows])})
    assert bits_of(ks.contains_rows(t, ["s"])[0], 6).tolist() == [True, False, True, True, True, False]
    image = ks.to_bytes()
    assert image.count(b"value-a") == 1
    forged = KeySet.from_bytes(image.replace(b"value-a", b"value-b"), ["s"])
    assert forged.num_keys == 4
    got, _, nc, na = forged.contains_rows(t, ["s"], None, want_applies=True)
    assert bits_of(got, 6).tolist() == [False, False, True, True, True, False]
    assert (nc, na) == (3, 6)


# ---- refusals: before any launch ----------------------------------------------------------------------------------

def _raw_call(L, handle, types, views, n, contained):
    import torch

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return L.lib.dq_freq_contains_rows(handle, types, views, n, None, contained.data_ptr(), None, stream, None, None)


def test_refusals(dq):
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.grouping import build_frequencies
    from deequ_amd.matching import KeySet

    guard = torch.full((16,), 0xFF, dtype=torch.uint8, device="cuda")
    # a hashed table that is not self-contained: the merge of two tables of which one has no store
    a = build_frequencies(table({"s": ("utf8", ["p", "q"])}), ["s"])
    b = build_frequencies(table({"s": ("utf8", ["q", "r"])}), ["s"])
    a.materialize()
    merged = a.frequencies.merged(b.frequencies)
    assert not merged.self_contained()
    probe = table({"s": ("utf8", ["p"])})
    views = (L.ColumnView * 1)(probe.columns["s"].view())
    assert _raw_call(L, merged.handle, None, views, 1, guard) == L.DQ_E_STATE
    assert "does not own its values" in L.lib.dq_last_error().decode()
    # a type mismatch (no widening), a decimal scale mismatch: DQ_E_INVALID naming the column and both codes
    ks = KeySet.from_data(table({"k": ("i64", [1, 2, 3])}), ["k"])
    p32 = table({"k": ("i32", [1, 2, 3])})
    views = (L.ColumnView * 1)(p32.columns["k"].view())
    assert _raw_call(L, ks.table.handle, (ctypes.c_int32 * 1)(L.TYPE_I32), views, 3, guard) == L.DQ_E_INVALID
    assert f"column 0 has type {L.TYPE_I32}, the table's has {L.TYPE_I64}" in L.lib.dq_last_error().decode()
    from decimal import Decimal

    kd = KeySet.from_data(table({"d": ("decimal(10,2)", [Decimal("1.00")])}), ["d"])
    pd = table({"d": ("decimal(10,3)", [Decimal("1.000")])})
    views = (L.ColumnView * 1)(pd.columns["d"].view())
    code = L.decimal_type(10, 3)
    assert _raw_call(L, kd.table.handle, (ctypes.c_int32 * 1)(code), views, 1, guard) == L.DQ_E_INVALID
    assert f"column 0 has type {code}, the table's has {L.decimal_type(10, 2)}" in L.lib.dq_last_error().decode()
    # the same refusals through the Python layer, naming the column and both types; an arity mismatch
    with pytest.raises(Exception, match="column k to be i64.*found i32"):
        ks.contains_rows(p32, ["k"])
    with pytest.raises(Exception, match=r"column d to be decimal\(10,2\).*found decimal\(10,3\)"):
        kd.contains_rows(pd, ["d"])
    two = table({"k": ("i64", [1]), "j": ("i64", [1])})
    with pytest.raises(ValueError, match="2 columns .* key set over 1"):
        ks.contains_rows(two, ["k", "j"])
    # n_rows >= 2^31 with a 1-row buffer: rejected on the argument alone
    views = (L.ColumnView * 1)(table({"k": ("i64", [1])}).columns["k"].view())
    assert _raw_call(L, ks.table.handle, None, views, 2 ** 31, guard) == L.DQ_E_INVALID
    assert "n_rows < 2^31" in L.lib.dq_last_error().decode()
    assert (guard.cpu().numpy() == 0xFF).all(), "a refused call wrote"


# ---- end to end ---------------------------------------------------------------------------------------------------

def _orders(n=1000, seed=9):
    rng = np.random.default_rng(seed)
    cid = [None if rng.random() < 0.05 else int(rng.integers(0, 150)) for _ in range(n)]
    amount = [None if rng.random() < 0.05 else round(float(rng.normal()), 2) for _ in range(n)]
    note = [f"n{i % 13}" for i in range(n)]
    return cid, amount, note


def _orders_table(cid, amount, note, lo=0, hi=None):
    return table({"cid": ("i64", cid[lo:hi]), "amount": ("f64", amount[lo:hi]), "note": ("utf8", note[lo:hi])})


CUSTOMERS = [(i,) for i in range(0, 150, 3)] + [(None,)]


def _ratio(cid, amount=None, where=False):
    keep = None if not where else [a is not None and a > 0 for a in amount]
    c, a = model(CUSTOMERS, [(v,) for v in cid], keep)
    return sum(c), sum(a), c, a


def test_check_over_chunks_where_and_incremental(dq):
    from deequ_amd import Check, CheckLevel, CheckStatus, InMemoryStateProvider, VerificationSuite, matching
    from deequ_amd.matching import KeySet, ReferentialIntegrity

    cid, amount, note = _orders()
    ks = KeySet.from_data(table({"id": ("i64", [c[0] for c in CUSTOMERS])}), "id")
    whole = _orders_table(cid, amount, note)
    chunks = [_orders_table(cid, amount, note, 0, 300), _orders_table(cid, amount, note, 300, 301),
              _orders_table(cid, amount, note, 301, None)]
    nc, na, _, _ = _ratio(cid)
    wc, wa, _, _ = _ratio(cid, amount, where=True)
    assert 0 < wc < nc and wa < na
    check = (Check(CheckLevel.Error, "orders").hasReferentialIntegrity("cid", ks, lambda v: v == nc / na)
             .hasReferentialIntegrity("cid", ks, lambda v: v == wc / wa).where("amount > 0"))
    plain, filtered = ReferentialIntegrity("cid", ks), ReferentialIntegrity("cid", ks, "amount > 0")
    for data, n_chunks in ((whole, 1), (chunks, 3)):
        before = matching.probe_calls
        r = VerificationSuite().onData(data).addCheck(check).run()
        assert matching.probe_calls - before == n_chunks * 2  # chunks x analyzers
        assert r.status == CheckStatus.Success, [c.message for cr in r.checkResults.values() for c in cr.constraintResults]
        assert r.metrics[plain].value.get() == nc / na
        assert r.metrics[filtered].value.get() == wc / wa
        m = r.metrics[plain]
        assert (m.name, m.instance, m.entity.value) == ("ReferentialIntegrity", "cid", "Column")
    # an incremental run over two halves equals the whole
    half = InMemoryStateProvider()
    first, second = _orders_table(cid, amount, note, 0, 500), _orders_table(cid, amount, note, 500, None)
    for a in (plain, filtered):
        a.calculate(first, saveStatesWith=half)
    for a, want in ((plain, nc / na), (filtered, wc / wa)):
        assert a.calculate(second, aggregateWith=half).value.get() == want
    # a where that keeps no row, and empty data: the empty state, as Compliance's
    from deequ_amd import Compliance

    none = ReferentialIntegrity("cid", ks, "amount > 1000").calculate(whole)
    like = Compliance("c", "cid >= 0", "amount > 1000").calculate(whole)
    assert none.value.isFailure and like.value.isFailure
    assert type(none.value.failed) is type(like.value.failed)
    # a where outside the GPU grammar
    bad = ReferentialIntegrity("cid", ks, "upper(note) = 'N1'").calculate(whole)
    assert bad.value.isFailure and "UnsupportedOnGpuPath" in type(bad.value.failed).__name__ + str(bad.value.failed)


@pytest.mark.parametrize("filteredRow", ["TRUE", "NULL"])
def test_failing_rows_are_the_orphans(dq, filteredRow):
    from deequ_amd import Check, CheckLevel
    from deequ_amd.matching import KeySet
    from deequ_amd.rowlevel import row_level_results

    cid, amount, note = _orders(500, seed=10)
    ks = KeySet.from_data(table({"id": ("i64", [c[0] for c in CUSTOMERS])}), "id")
    chunks = [_orders_table(cid, amount, note, 0, 200), _orders_table(cid, amount, note, 200, None)]
    check = (Check(CheckLevel.Error, "orders").hasReferentialIntegrity("cid", ks)
             .hasReferentialIntegrity("cid", ks).where("amount > 0"))
    res = row_level_results([check], chunks, filteredRow)
    assert not res.skipped
    plain, filtered = [str(c) for c in check.constraints]
    for name, where in ((plain, False), (filtered, True)):
        _, _, c, a = _ratio(cid, amount, where)
        orphans = [i for i in range(500) if a[i] and not c[i]]
        got = res.failing_rows(name)
        rows = [(x, y, z) for t in got for x, y, z in zip(_host(t, "cid"), _host(t, "amount"), _host(t, "note"))]
        assert rows == [(cid[i], amount[i], note[i]) for i in orphans]
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
    out = []
    for v, ok in zip(vals, valid):
        out.append(None if not ok else v.decode("utf-8") if isinstance(v, bytes) else v.item())
    return out


def test_arrow_and_bytes_round_trip(dq):
    pa = pytest.importorskip("pyarrow")
    from deequ_amd import AnalysisRunner, matching
    from deequ_amd.matching import KeySet, ReferentialIntegrity

    ref = pa.record_batch({"id": pa.array([1, 2, None, 5], pa.int64()), "code": pa.array(["a", "b", "c", None])})
    ks = KeySet.from_data(ref, ["id", "code"])
    assert (ks.num_keys, ks.columns, ks.dtypes) == (2, ("id", "code"), ("i64", "utf8"))
    rows = [(1, "a"), (2, "b"), (2, "a"), (None, "c"), (5, None), (1, "a")]
    batch = pa.record_batch({"k": pa.array([r[0] for r in rows], pa.int64()), "c": pa.array([r[1] for r in rows])})
    a = ReferentialIntegrity(["k", "c"], ks)
    before = matching.probe_calls
    ctx = AnalysisRunner.onData(batch).addAnalyzer(a).run()
    assert matching.probe_calls - before == 1
    m = ctx.metric(a)
    assert m.value.get() == 3 / 6 and m.entity.value == "Mutlicolumn" and m.instance == "k,c"
    # to_bytes -> from_bytes: the same bitmap
    back = KeySet.from_bytes(ks.to_bytes(), ks.columns)
    assert (back.num_keys, back.dtypes) == (ks.num_keys, ks.dtypes)
    t = table({"k": ("i64", [r[0] for r in rows]), "c": ("utf8", [r[1] for r in rows])})
    one, two = ks.contains_rows(t, ["k", "c"]), back.contains_rows(t, ["k", "c"])
    assert bits_of(one[0], 6).tolist() == bits_of(two[0], 6).tolist() == [True, True, False, False, False, True]


def test_arithmetic_where_metric_and_failing_rows(dq):
    """A `where` with arithmetic (its operand is a derived column the run attaches) on the metric path and on the
    row-level path, beside another constraint of the same call."""
    from deequ_amd import Check, CheckLevel, VerificationSuite
    from deequ_amd.matching import KeySet, ReferentialIntegrity
    from deequ_amd.rowlevel import row_level_results

    cid, amount, note = _orders(600, seed=11)
    ks = KeySet.from_data(table({"id": ("i64", [c[0] for c in CUSTOMERS])}), "id")
    chunks = [_orders_table(cid, amount, note, 0, 250), _orders_table(cid, amount, note, 250, None)]
    keep = [a is not None and a * 2 > 0.5 for a in amount]
    c, a = model(CUSTOMERS, [(v,) for v in cid], keep)
    assert 0 < sum(c) < sum(a) < 600
    where = "amount * 2 > 0.5"
    check = (Check(CheckLevel.Error, "orders").hasReferentialIntegrity("cid", ks, lambda v: v == sum(c) / sum(a))
             .where(where).isComplete("note"))
    r = VerificationSuite().onData(chunks).addCheck(check).run()
    assert r.metrics[ReferentialIntegrity("cid", ks, where)].value.get() == sum(c) / sum(a)
    assert r.status.name == "Success"
    for filteredRow in ("TRUE", "NULL"):
        res = row_level_results([check], chunks, filteredRow)
        assert not res.skipped
        name = str(check.constraints[0])
        got = res.failing_rows(name)
        rows = [(x, y, z) for t in got for x, y, z in zip(_host(t, "cid"), _host(t, "amount"), _host(t, "note"))]
        assert rows == [(cid[i], amount[i], note[i]) for i in range(600) if a[i] and not c[i]]
        assert res.outcome(str(check.constraints[1])).num_pass == 600
        assert all([c[0] for c in t.schema] == ["cid", "amount", "note"] for t in got), "a derived column leaked"


def test_bool_inside_a_hashed_tuple(dq):
    """A (bool, utf8) key: the probe's bit-packed boolean column is compared with the store's byte per value."""
    rng = np.random.default_rng(12)
    ref = [(True, "a"), (False, "b"), (True, "c"), (None, "d"), (False, None)]
    ks = build(dq, ["bool", "utf8"], ["flag", "s"], ref)
    rows = [(None if rng.random() < 0.05 else bool(rng.integers(2)),
             None if rng.random() < 0.05 else "abcde"[int(rng.integers(5))]) for _ in range(N_TYPES)]
    want = check_probe(ks, ["bool", "utf8"], ["flag", "s"], ref, rows)
    assert 0 < sum(want) < len(rows)
    assert model(ref, [(True, "a"), (False, "a"), (False, "b"), (True, "b"), (True, "d"), (False, "d")])[0] == \
        [True, False, True, False, False, False]
    check_probe(ks, ["bool", "utf8"], ["flag", "s"], ref,
                [(True, "a"), (False, "a"), (False, "b"), (True, "b"), (True, "d"), (False, "d")])
