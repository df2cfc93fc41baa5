"""Exact-count tests of the grouping pass (deequ_amd/csrc/dq_group.hip) at the sizes and key shapes its other tests do
not reach.  Every case compares build_frequencies(...).frequencies.export() and summary() with the numpy reference
(tests/group_ref.py ref_table) of the same host arrays (tests/group_cases.py): for one fixed-width column the keys
must be the reference's value bits in ascending order with its counts; for strings and tuples (hashed keys) the counts
must be the reference's multiset.  Null slots carry non-zero payloads (every third one all-ones).

What each block reaches (functions of dq_group.hip):

* multi-tile compaction -- one chunk of 2048 * 2048 + 2048 + 1 rows.  The launch grid of group_compact is capped at
  2048 workgroups of 2048 rows (freq_build_impl), so workgroup 0 loops to a full second tile, workgroup 1 to a tile of one row
  (the last row) and no other workgroup loops: the tile loop and the reuse of wave_n / tile_base behind the barrier
  that ends a tile, and the carry of k_and / k_or across tiles.  Unhashed keys ("w": ~50 000 wide values, the
  dictionary form declines and the table is sorted; "r": values below 300, end_bit = 9) take the prefetch (`fetch`) with
  its guard `t0 + tstride < n` true for exactly these two workgroups; row 2048 * 2048, the first row of the second
  tile, is the only row with its value and must come out as a group of count 1.  (One way to see that the test
  watches the prefetch: with `if (t0 + tstride < n)` replaced by `if (false)` in a scratch build, workgroup 0's second
  tile repeats its first tile's values and these cases fail.)  Hashed keys: ("l", "i") with ~3000 pairs -- more than
  kDictMax, so sorted also by default, then checked by verify_compacted with stride 2 in a second grid-stride
  iteration (grid_for caps at 8192 * 256 threads); ("d", "e") with 700 frequent pairs and no rare one takes the
  dictionary form by default with two iterations of dict_count (2048 workgroups * 1024 keys) and must equal
  the sort's table; ("m", "j") with ~1.4 M pairs is checked in sorted order, verify_runs's second grid-stride
  iteration.  The unhashed tables cut into two chunks at 2048 * 2048 + 7 (the first chunk's workgroup 0 loops
  to a 7-row tile) must equal the one-chunk tables.
* bit-range edges -- end_bit (freq_build_impl) comes from the AND / OR of all appended keys: all keys equal (differ == 0,
  end_bit = 1), two keys differing in one bit b (end_bit = b + 1, the digit boundaries 8 / 16 / 24 / 32 / 48 and bit
  63 among them) under non-zero common high bits, 256 and 257 consecutive values above 1 << 40 (end_bit 8 and 9),
  sign-extended negative i32 / i8 among positive ones (end_bit = 64), 0.0 and -0.0 (bit 63 alone), NaNs of several
  payloads and signs (one canonical key), and a wide key that only one of two chunks holds, in both chunk orders
  (the AND / OR must accumulate across launches).
* strided representative search -- verify_compacted's sample stride is above 1 only for more than 2048
  groups: 5000 pairs (stride 3) and exactly 65 536 pairs in 530 000 rows (kCompactedMaxGroups and the
  8 * G <= nv edge, stride 32) must build without a collision report and with exact counts; 20 000 strings squeezed
  into 4096 hash keys (stride 2) must be refused as a collision.
* ragged sizes -- row counts around a validity word, a wave, a block and a tile (31 .. 4097) with nulls forced at
  rows 0, 31, 32 and n - 1, a column without a validity bitmap, and an all-null column (nv == 0).
* chunk shapes -- 64 chunks of 0 / 1 / 63 / 64 / 65 / 700 rows, zero-row chunks first, last and in between (skipped by freq_build_impl).
* column limit -- kMaxGroupCols = 8 columns of eight types in one key; 9 are refused (freq_build_impl).
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import dq_oracle as O
from tests import group_cases as C
from tests import group_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import deequ_amd

    return deequ_amd


def _build(data, names):
    from deequ_amd.grouping import build_frequencies

    fr = build_frequencies(data, names)
    keys, counts = fr.frequencies.export()
    return fr, np.asarray(keys).copy(), np.asarray(counts).copy()


def _assert_table(built, ref: R.RefTable, num_rows: int, what):
    fr, keys, counts = built
    s = fr.frequencies.summary(fr.numRows)
    assert fr.numRows == num_rows, what
    assert (s.num_groups, s.num_unique, s.num_values) == (ref.num_groups, ref.num_unique, ref.num_values), what
    assert len(keys) == ref.num_groups and np.all(keys[1:] > keys[:-1]), what  # distinct keys, ascending
    if ref.keys is not None:
        assert np.array_equal(keys, ref.keys), what
        assert np.array_equal(counts, ref.counts), what
    else:
        assert np.array_equal(np.sort(counts), ref.counts), what


def _check(case, names, data=None):
    data = C.to_device_case(case) if data is None else data
    ref = R.ref_table(*C.key_columns(case, names))
    built = _build(data, names)
    _assert_table(built, ref, C.rows(case), names)
    return ref, built


# ---------------------------------------------------------------------------------------------------------------
# 1. multi-tile compaction
# ---------------------------------------------------------------------------------------------------------------
class _MultiTile:
    def __init__(self):
        self.chunk = C.multi_tile()
        self.table = C.to_device(self.chunk)
        self.refs = {}

    def ref(self, names) -> R.RefTable:
        key = tuple(names)
        if key not in self.refs:
            self.refs[key] = R.ref_table(*C.key_columns([self.chunk], names))
        return self.refs[key]


@pytest.fixture(scope="module")
def multi_tile(dq):
    return _MultiTile()


@pytest.mark.parametrize("col,lone_value", [("w", 0x0123_4567_89AB_CDE0), ("r", 299)])
def test_multi_tile_unhashed(multi_tile, monkeypatch, col, lone_value):
    monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    n = C.MULTI_TILE_ROWS
    by_name = {c.name: c for c in multi_tile.chunk}
    assert n == 2048 * 2048 + 2048 + 1 and by_name[col].valid[n - 1] and by_name[col].valid[C.FULL_GRID]
    assert by_name[col].values[C.FULL_GRID] == lone_value
    ref = multi_tile.ref([col])
    assert ref.counts[ref.keys == np.uint64(lone_value)].tolist() == [1]  # the second tile's first row: its own group
    one = _build(multi_tile.table, [col])
    _assert_table(one, ref, n, col)
    if col == "r":
        assert int(ref.keys.max()).bit_length() == 9 and len(ref.keys) == 300
    # the same rows as two chunks, cut 7 rows into workgroup 0's second tile
    halves = C.split([by_name[col]], [C.FULL_GRID + 7])
    two = _build([C.to_device(h) for h in halves], [col])
    _assert_table(two, ref, n, col)
    assert np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])


@pytest.mark.parametrize("mode", ["0", None])
def test_multi_tile_hashed_few_thousand_pairs(multi_tile, monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    else:
        monkeypatch.setenv("DQ_GROUP_DICT", mode)
    ref = multi_tile.ref(["l", "i"])
    assert 2900 <= ref.num_groups <= 3001 and ref.num_unique >= 1 and 8 * ref.num_groups <= ref.num_values
    _assert_table(_build(multi_tile.table, ["l", "i"]), ref, C.MULTI_TILE_ROWS, mode)


def test_multi_tile_hashed_dictionary_form(multi_tile, monkeypatch):
    ref = multi_tile.ref(["d", "e"])
    # what the default needs to take the form and to loop in dict_count: 16 samples per key, > 2048 * 1024 keys
    assert ref.num_groups == 700 and ref.counts.min() > 1000 and ref.num_values > 2048 * 1024
    monkeypatch.setenv("DQ_GROUP_DICT", "0")
    sort = _build(multi_tile.table, ["d", "e"])
    monkeypatch.delenv("DQ_GROUP_DICT")
    form = _build(multi_tile.table, ["d", "e"])
    _assert_table(sort, ref, C.MULTI_TILE_ROWS, "sort")
    _assert_table(form, ref, C.MULTI_TILE_ROWS, "dictionary")
    assert np.array_equal(sort[1], form[1]) and np.array_equal(sort[2], form[2])


def test_multi_tile_hashed_many_pairs(multi_tile, monkeypatch):
    monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    ref = multi_tile.ref(["m", "j"])
    assert 1_300_000 <= ref.num_groups <= 1_600_000 and ref.num_values > 8192 * 256
    _assert_table(_build(multi_tile.table, ["m", "j"]), ref, C.MULTI_TILE_ROWS, "m, j")


# ---------------------------------------------------------------------------------------------------------------
# 2. the sort's bit range
# ---------------------------------------------------------------------------------------------------------------
_BIT_EDGES = C.bit_edges()


@pytest.mark.parametrize("name", list(_BIT_EDGES))
def test_bit_range_edges(dq, monkeypatch, name):
    monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    case = _BIT_EDGES[name]
    ref, _ = _check(case, ["k"])
    differ = int(np.bitwise_or.reduce(ref.keys) ^ np.bitwise_and.reduce(ref.keys))
    expect = {"all-equal": 0, "f64-nans": 0, "f64-zeros": 1 << 63, "base-plus-256": 255, "base-plus-257": 511}
    for prefix, bits in expect.items():  # the inputs are what their names say
        if name.startswith(prefix):
            assert differ == bits, (name, hex(differ))
    if name.startswith("flip-bit-"):
        assert differ == 1 << int(name.rsplit("-", 1)[1]) and ref.num_groups == 2
    if name.endswith("-signed") or name.startswith("wide-key"):
        assert differ.bit_length() == (64 if name.endswith("-signed") else 41)
    if name.startswith(("all-equal", "f64-nans")):
        assert ref.num_groups == 1


# ---------------------------------------------------------------------------------------------------------------
# 3. the strided representative search of verify_compacted
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,distinct,nulls", [(60_000, 5000, 1500), (530_000, 65_536, 4000)])
def test_strided_representative_search(dq, monkeypatch, n, distinct, nulls):
    monkeypatch.setenv("DQ_GROUP_DICT", "0")
    monkeypatch.delenv("DQ_TEST_GROUP_HASH_MASK", raising=False)
    case = [C.strided(n, distinct, nulls)]
    ref, _ = _check(case, ["l", "i"])
    # the compaction-order check runs (:1116-1117), its stride is above 1
    assert ref.num_groups == distinct and 8 * distinct <= ref.num_values == n - nulls
    assert -(-distinct // 2048) == {5000: 3, 65_536: 32}[distinct]


def test_strided_search_reports_collisions(dq, monkeypatch):
    from deequ_amd import _lib as L
    from deequ_amd.grouping import build_frequencies

    case = [C.many_strings()]
    data = C.to_device_case(case)
    monkeypatch.setenv("DQ_GROUP_DICT", "0")
    monkeypatch.setenv("DQ_TEST_GROUP_HASH_MASK", "fff")  # at most 4096 keys for 20 000 strings: stride 2
    with pytest.raises(L.DQError) as e:
        build_frequencies(data, ["s"])
    assert "collision" in str(e.value)
    monkeypatch.delenv("DQ_TEST_GROUP_HASH_MASK")
    ref, _ = _check(case, ["s"], data)  # without the mask: the exact table (sorted-order check: G > nv / 8)
    assert ref.num_groups == 20_000


# ---------------------------------------------------------------------------------------------------------------
# 4. ragged sizes and null edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.RAGGED_SIZES)
def test_ragged_sizes_and_null_edges(dq, monkeypatch, n):
    monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    chunk = C.ragged(n)
    data = C.to_device(chunk)
    assert data.columns["p"].validity is None and data.columns["k"].validity is not None
    for names in (["k"], ["s", "i"], ["p"], ["s"], ["p", "k"]):
        _check([chunk], names, data)
    ref, (fr, keys, counts) = _check([chunk], ["z"], data)  # all rows null
    s = fr.frequencies.summary(fr.numRows)
    assert (s.num_values, s.num_groups, len(keys), len(counts)) == (0, 0, 0, 0)
    ref, _ = _check([chunk], ["z", "p"], data)
    assert ref.num_groups == 0


def test_all_null_column_through_the_runner(dq):
    """Every analyzer over an all-null key gives what the oracle's state gives: the empty-state failure, or
    CountDistinct's 0 and UniqueValueRatio's NaN."""
    n = 257
    chunk = C.ragged(n)
    data = C.to_device(chunk)
    ocols = {c.name: O.OColumn(c.dtype, c.values, np.ones(n, bool) if c.valid is None else c.valid) for c in chunk}
    analyzers = [dq.Uniqueness("z"), dq.Distinctness("z"), dq.CountDistinct("z"), dq.UniqueValueRatio("z"),
                 dq.Entropy("z"), dq.MutualInformation("z", "p"), dq.Uniqueness(["p", "z"])]
    ctx = dq.AnalysisRunner.onData(data).addAnalyzers(analyzers).run()
    for a in analyzers:
        kind = type(a).__name__
        state = O.compute_state((kind, a.columns[0] if kind == "Entropy" else a.columns), ocols, n)
        m = ctx.metric(a)
        if state is None:
            assert m.value.isFailure and "Empty state" in str(m.value.failed), (a, m)
        else:
            got, want = m.value.get(), state.metricValue()
            assert got == want or (got != got and want != want), (a, got, want)
    assert sum(1 for a in analyzers if ctx.metric(a).value.isFailure) == 5


# ---------------------------------------------------------------------------------------------------------------
# 5. chunk shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [["f"], ["s", "l"]])
def test_many_chunks_with_empty_ones(dq, monkeypatch, names):
    monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    case = C.chunk_shapes()
    sizes = [len(ch[0].values) for ch in case]
    assert len(case) == 64 and sizes[0] == 0 and sizes[-1] == 0 and sizes.count(0) >= 3
    assert set(sizes) == {0, 1, 63, 64, 65, 700}
    ref, chunked = _check(case, names)
    whole = _build(C.to_device(C.concat(case)), names)
    _assert_table(whole, ref, C.rows(case), names)
    assert np.array_equal(chunked[1], whole[1]) and np.array_equal(chunked[2], whole[2])


# ---------------------------------------------------------------------------------------------------------------
# 6. the column limit
# ---------------------------------------------------------------------------------------------------------------
def test_eight_key_columns_and_the_ninth(dq, monkeypatch):
    from deequ_amd import _lib as L
    from deequ_amd.grouping import build_frequencies

    monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    chunk = C.nine_columns()
    data = C.to_device(chunk)
    assert [data.columns[c].dtype for c in C.EIGHT] == ["i64", "i32", "f64", "f32", "i16", "i8", "bool", "utf8"]
    ref, _ = _check([chunk], C.EIGHT, data)
    assert ref.num_groups > 500
    with pytest.raises(L.DQError) as e:
        build_frequencies(data, C.EIGHT + ["c_more"])
    assert "1..8 grouping columns" in str(e.value)
