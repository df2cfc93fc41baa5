"""The grouping scratch arena (deequ_amd/csrc/dq_arena.h, used by dq_group.hip) across entry points in one process.

Every grouping entry point opens a frame on its device's slot list and takes its buffers in sequence, so slot k is a
compaction buffer in one call, a sort temporary in the next and eight bytes of a summary after that.  `sequence()`
runs the entry points one after the other on one device and stream -- a hashed (string, i64) table of 70 001 rows in
two chunks (9 sort tiles of 8192 keys, 35 compaction tiles of 2048 rows), dq_freq_top, an exact-key table of 3 rows,
dq_freq_summarize, two materialised string tables merged, dq_freq_take_values, dq_freq_mutual_information of a
stored two-column table, then a table of 200 003 rows (every slot grows after the small calls) -- and at the end the
first table must summarise and export exactly as it did at the start.  Every result is compared with the numpy /
mpmath reference (tests/group_ref.py) of the same host arrays (tests/group_cases.py); Entropy and MutualInformation
within twice the derived rounding bound, as tests/test_group_metrics_exact_gpu.py asks.

The second test runs the same sequence in a child process with DQ_GROUP_DICT=1, where the first table (1500 tuples)
takes the dictionary form and the large one (30 000 tuples) declines it after the sample: dict_table's takes are
then part of both frames.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import group_cases as C
from tests import group_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

MARGIN = 2.0  # over the derived bound (tests/test_group_metrics_exact_gpu.py)


def _tuples(n: int, distinct: int, seed: int, cut: int):
    """(s: utf8, l: i64) rows over `distinct` tuples, ~5 % nulls in each column, as two chunks cut at row `cut`."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, distinct, n)
    pool = rng.integers(-(1 << 63), (1 << 63) - 1, distinct, dtype=np.int64)
    s = [b"value-%06d-%s" % (j % (distinct // 3 + 1), b"z" * (j % 23)) for j in pick]
    chunk = [C.with_nulls(rng, "s", "utf8", s, C.forced_valid(rng, n, 0.05, keep=(0, n - 1))),
             C.with_nulls(rng, "l", "i64", pool[pick], C.forced_valid(rng, n, 0.05, keep=(0, n - 1)))]
    return C.split(chunk, [cut])


def _strings(n: int, lo: int, hi: int, seed: int):
    rng = np.random.default_rng(seed)
    s = [b"group-%05d-%s" % (j, b"q" * (j % 47)) for j in rng.integers(lo, hi, n)]
    return [[C.with_nulls(rng, "s", "utf8", s, C.forced_valid(rng, n, 0.1, keep=(0,)))]]


def _pairs(n: int, seed: int):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 40, n).astype(np.int64) * (1 << 35)
    y = ((x >> 35) % 5 + rng.integers(0, 3, n)).astype(np.int32)
    return [[C.with_nulls(rng, "x", "i64", x, C.forced_valid(rng, n, 0.05)), C.with_nulls(rng, "y", "i32", y, None)]]


def _build(case, names):
    from deequ_amd.grouping import build_frequencies

    return build_frequencies(C.to_device_case(case), names)


def _table(fr):
    keys, counts = fr.frequencies.export()
    s = fr.frequencies.summary(fr.numRows)
    return np.asarray(keys).copy(), np.asarray(counts).copy(), (s.num_groups, s.num_unique, s.num_values, s.entropy)


def _assert_table(fr, ref: R.RefTable, num_rows: int, what):
    keys, counts, (groups, unique, values, entropy) = _table(fr)
    assert fr.numRows == num_rows, what
    assert (groups, unique, values) == (ref.num_groups, ref.num_unique, ref.num_values), what
    assert len(keys) == ref.num_groups and np.all(keys[1:] > keys[:-1]), what
    if ref.keys is not None:
        assert np.array_equal(keys, ref.keys) and np.array_equal(counts, ref.counts), what
    else:
        assert np.array_equal(np.sort(counts), ref.counts), what
    value, bound = R.ref_entropy(ref.counts, num_rows)
    ratio = R.error_ratio(entropy, value, bound)
    print(f"{what}: entropy |error| / bound {ratio:.3f}")
    assert ratio <= MARGIN, (what, entropy, bound, ratio)


def sequence():
    from deequ_amd import _lib as L

    # 1. a hashed table over (string, i64): 70 001 rows in two chunks
    first_case = _tuples(70_001, 1500, 5, cut=33_333)
    first_ref = R.ref_table(*C.key_columns(first_case, ["s", "l"]))
    assert first_ref.num_values > 7 * 8192 and first_ref.num_groups == 1500
    first = _build(first_case, ["s", "l"])
    _assert_table(first, first_ref, 70_001, "first")
    before = _table(first)
    # 2. dq_freq_top: the ten largest counts, each beside its own key
    keys, cnts, reps = (ctypes.c_uint64 * 10)(), (ctypes.c_int64 * 10)(), (ctypes.c_uint64 * 10)()
    got = ctypes.c_int32()
    L.check(L.lib.dq_freq_top(first.frequencies.handle, 10, keys, cnts, reps, ctypes.byref(got)))
    assert got.value == 10 and list(cnts) == first_ref.counts[::-1][:10].tolist()
    count_of = dict(zip(before[0].tolist(), before[1].tolist()))
    assert [count_of[k] for k in keys] == list(cnts)
    # 3. an exact-key table over 3 i32 rows
    tiny_case = [[C.HCol("k", "i32", np.array([7, -2, 7], np.int32), None)]]
    _assert_table(_build(tiny_case, ["k"]), R.ref_table(*C.key_columns(tiny_case, ["k"])), 3, "tiny")
    # 4. the first table's summary again, after other frames used the slots
    assert _table(first)[2] == before[2]
    # 5. two materialised string tables, merged
    a_case, b_case = _strings(3001, 0, 900, 7), _strings(2500, 600, 1400, 11)
    merged = _build(a_case, ["s"]).sum(_build(b_case, ["s"]))
    both = [C.concat([a_case[0], b_case[0]])]
    both_ref = R.ref_table(*C.key_columns(both, ["s"]))
    _assert_table(merged, both_ref, 5501, "merged")
    # 6. dq_freq_take_values: every group's string with its count
    mkeys, mcounts, _ = _table(merged)
    stored = dict(zip(merged.frequencies.take_values(mkeys, 0), mcounts.tolist()))
    col = both[0][0]
    want, want_counts = np.unique(np.array([v for v, ok in zip(col.values, col.valid) if ok], dtype=object),
                                  return_counts=True)
    assert stored == dict(zip(want.tolist(), want_counts.tolist()))
    # 7. MutualInformation of a stored two-column table
    pair_case = _pairs(4099, 13)
    pair_ref = R.ref_table(*C.key_columns(pair_case, ["x", "y"]))
    pairs = _build(pair_case, ["x", "y"]).materialize()
    _assert_table(pairs, pair_ref, 4099, "pairs")
    value, bound = R.ref_mi(pair_ref.joint, 4099)
    ratio = R.error_ratio(pairs.frequencies.mutual_information(4099), value, bound)
    print(f"pairs: mutual information |error| / bound {ratio:.3f}")
    assert ratio <= MARGIN, (value, bound, ratio)
    # 8. growth after the small calls: 200 003 rows, 30 000 tuples
    big_case = _tuples(200_003, 30_000, 17, cut=100_000)
    _assert_table(_build(big_case, ["s", "l"]), R.ref_table(*C.key_columns(big_case, ["s", "l"])), 200_003, "big")
    # 9. the first table is what it was
    after = _table(first)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and after[2] == before[2]


def test_slots_are_reused_across_entry_points(monkeypatch):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    sequence()


def test_slots_with_the_dictionary_form():
    code = "import sys; sys.path.insert(0, %r); from tests import test_group_arena_gpu as T; T.sequence(); print('ok')" % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DQ_GROUP_DICT="1"), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
