"""The grouping reference (tests/group_ref.py) checked on the CPU, on the inputs of the GPU edge tests
(tests/group_cases.py) at their small sizes:

* counts: ref_table's groups, counts and per-column marginals equal the oracle's row-by-row frequencies
  (oracle/dq_oracle.py frequencies), key by key for a single fixed-width column;
* bound condition: the oracle's float64 Entropy / MutualInformation of the same tables, and of every input of
  test_group_metrics_exact_gpu.py, lie within 1 x bound of the 50-digit value.  The GPU tests allow 2 x bound; an
  honest double evaluation in another summation order has to fit inside the bound itself, or the derivation is wrong;
* self-checks of the 50-digit values: a uniform table of G groups has entropy ln G, an exact product table has
  mutual information 0, y = x gives the entropy of x -- to 40 digits.
"""
from __future__ import annotations

import functools
import struct

import mpmath
import numpy as np
import pytest

from oracle import dq_oracle as O
from tests import group_cases as C
from tests import group_ref as R


def _oracle_columns(case):
    whole = C.concat(case) if len(case) > 1 else case[0]
    n = C.rows(case)
    return {c.name: O.OColumn(c.dtype, c.values, np.ones(n, bool) if c.valid is None else c.valid) for c in whole}, n


def _oracle_key(dtype: str, bits: int):
    """A reference key (value bits) in the form of the oracle's _group_key."""
    if dtype == "f64":
        v = struct.unpack("<d", struct.pack("<Q", bits))[0]
        return ("f", b"nan" if v != v else struct.pack("<d", v))
    if dtype == "f32":
        v = struct.unpack("<f", struct.pack("<I", bits))[0]
        return ("f", b"nan" if v != v else struct.pack("<f", v))
    return ("i", bits - (1 << 64) if bits >= 1 << 63 else bits)


@functools.lru_cache(maxsize=None)
def _small_inputs():
    """(id, case, key column sets) of every generator of the GPU edge tests, at a size the oracle's loop takes."""
    out = [("multi-tile", [C.multi_tile(n=4099, lone=2048, wide=50, tuples=60, many=3000, few=20)], C.MULTI_TILE_KEYS)]
    out += [(f"bits-{name}", case, [["k"]]) for name, case in C.bit_edges(n=600).items()]
    out.append(("strided", [C.strided(3000, 250, 60)], [["l", "i"]]))
    out.append(("many-strings", [C.many_strings(1500, 500)], [["s"]]))
    out += [(f"ragged-{n}", [C.ragged(n)], [["k"], ["s", "i"], ["p"], ["z"]]) for n in C.RAGGED_SIZES]
    out.append(("chunk-shapes", C.chunk_shapes(), [["f"], ["s", "l"]]))
    out.append(("eight-columns", [C.nine_columns(600)], [C.EIGHT]))
    return out


def _freq_from_ref(ref: R.RefTable) -> dict:
    if ref.joint is not None:
        x, y, c = ref.joint
        return {(int(a), int(b)): int(n) for a, b, n in zip(x, y, c)}
    return {(g,): int(n) for g, n in enumerate(ref.counts)}


def _fixed_order_sum(terms: np.ndarray) -> float:
    """The float64 sum of the terms in the order of summary_part / summary_final (mi_part / mi_final): thread t of
    block b adds the terms b*256 + t, + nb*256, ... in turn, the block's 256 sums fold in halves, the nb partials are
    added in order."""
    G = len(terms)
    nb = R.launched_blocks(G)
    chain = -(-G // (nb * 256))
    padded = np.zeros(chain * nb * 256, dtype=np.float64)
    padded[:G] = terms
    acc = np.zeros((nb, 256), dtype=np.float64)
    for step in padded.reshape(chain, nb, 256):
        acc = acc + step
    s = 128
    while s >= 1:
        acc = acc[:, :s] + acc[:, s:2 * s]
        s >>= 1
    total = 0.0
    for part in acc[:, 0].tolist():
        total += part
    return total


def _float64_terms(op: str, ref: R.RefTable, num_rows: int) -> np.ndarray:
    """The oracle's expression of every group's term (dq_oracle.py GroupingMetricState.metricValue), in float64."""
    n = float(num_rows)
    if op == "Entropy":
        p = ref.counts.astype(np.float64) / n
        return -p * np.log(p)
    x, y, c = ref.joint
    a, b = np.zeros(int(x.max()) + 1, np.int64), np.zeros(int(y.max()) + 1, np.int64)
    np.add.at(a, x, c)
    np.add.at(b, y, c)
    pxy = c.astype(np.float64) / n
    return pxy * np.log(pxy / ((a[x].astype(np.float64) / n) * (b[y].astype(np.float64) / n)))


def _check_bound(op: str, freq: dict, ref: R.RefTable, num_rows: int, what):
    """Float64 evaluations of the table lie within 1 x bound of the 50-digit value: the oracle's terms added in the
    kernels' fixed order, inside the very bound the GPU tests use (doubled there); and the oracle's own value, whose
    ``sum`` adds the G terms one after the other, inside the same derivation's bound for that order (a term passes
    through up to G - 1 additions; see tests/group_ref.py on why the kernels' depth does not hold for it)."""
    ref_of = (lambda **kw: R.ref_mi(ref.joint, num_rows, **kw)) if op == "MutualInformation" else \
             (lambda **kw: R.ref_entropy(ref.counts, num_rows, **kw))
    G = ref.num_groups
    ratios = []
    for got, (value, bound) in ((_fixed_order_sum(_float64_terms(op, ref, num_rows)), ref_of()),
                                (O.GroupingMetricState(op, freq, num_rows).metricValue(),
                                 ref_of(additions=max(R.depth(G), G - 1)))):
        ratio = R.error_ratio(got, value, bound) if bound > 0 else (0.0 if got == 0 else float("inf"))
        assert ratio <= 1.0, (what, op, got, mpmath.nstr(value, 25), bound, ratio)
        ratios.append(ratio)
    return ratios


@pytest.mark.parametrize("index", range(len(_small_inputs())), ids=[i[0] for i in _small_inputs()])
def test_reference_counts_equal_the_oracle(index):
    name, case, key_sets = _small_inputs()[index]
    ocols, n = _oracle_columns(case)
    for names in key_sets:
        freq = O.frequencies(ocols, names, n)
        cols, valid = C.key_columns(case, names)
        ref = R.ref_table(cols, valid)
        assert ref.num_values == sum(freq.values()), (name, names)
        assert ref.num_groups == len(freq) and ref.num_unique == sum(1 for c in freq.values() if c == 1), (name, names)
        assert sorted(ref.counts.tolist()) == sorted(freq.values()), (name, names)
        if ref.keys is not None:  # one fixed-width column: the very keys, ascending
            assert np.all(ref.keys[1:] > ref.keys[:-1])
            mine = {(_oracle_key(cols[0][0], int(k)),): int(c) for k, c in zip(ref.keys, ref.counts)}
            assert mine == freq, (name, names)
        for c in range(len(names)):
            marginal: dict = {}
            for key, count in freq.items():
                marginal[key[c]] = marginal.get(key[c], 0) + count
            assert ref.marginals[c].tolist() == sorted(marginal.values()), (name, names, c)
        # the bound condition on the same tables (the oracle's own frequencies, its own summation order)
        if freq and len(names) == 1:
            _check_bound("Entropy", freq, ref, n, (name, names))
        if freq and len(names) == 2:
            _check_bound("MutualInformation", freq, ref, n, (name, names))


@functools.lru_cache(maxsize=None)
def _entropy_cases():
    return C.entropy_cases()


@functools.lru_cache(maxsize=None)
def _mi_cases():
    return C.mi_cases()


@pytest.mark.parametrize("name", list(_entropy_cases()))
def test_oracle_entropy_within_the_bound(name):
    chunk = _entropy_cases()[name]
    n = C.rows([chunk])
    ref = R.ref_table(*C.key_columns([chunk], ["x"]))
    if n <= 100_000:  # (the larger tables' counts are np.unique's as well; the oracle's loop is not run over them)
        freq = O.frequencies(_oracle_columns([chunk])[0], ["x"], n)
        assert sorted(freq.values()) == sorted(ref.counts.tolist())
    _check_bound("Entropy", _freq_from_ref(ref), ref, n, name)


@pytest.mark.parametrize("name", list(_mi_cases()))
def test_oracle_mutual_information_within_the_bound(name):
    chunk = _mi_cases()[name]
    n = C.rows([chunk])
    ref = R.ref_table(*C.key_columns([chunk], ["x", "y"]))
    freq = O.frequencies(_oracle_columns([chunk])[0], ["x", "y"], n)
    assert sorted(freq.values()) == sorted(ref.counts.tolist())
    _check_bound("MutualInformation", freq, ref, n, name)
    _check_bound("MutualInformation", _freq_from_ref(ref), ref, n, name)


def test_value_bits_rules():
    """fixed_bits in dq_freq_table.h: NaN canonical, -0.0 and 0.0 distinct, integers sign-extended, a bool 0 / 1."""
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    assert set(R.value_bits("f64", nans.view(np.float64)).tolist()) == {0x7FF8000000000000}
    assert R.value_bits("f64", np.array([0.0, -0.0, np.inf])).tolist() == [0, 1 << 63, 0x7FF0000000000000]
    nans32 = np.array([0x7FC00000, 0xFFC00001, 0x7F800001], dtype=np.uint32)
    assert set(R.value_bits("f32", nans32.view(np.float32)).tolist()) == {0x7FC00000}
    assert R.value_bits("f32", np.array([-0.0, np.inf], dtype=np.float32)).tolist() == [0x80000000, 0x7F800000]
    for dt in ("i64", "i32", "i16", "i8"):
        assert R.value_bits(dt, np.array([-1, 1, -128])).tolist() == [(1 << 64) - 1, 1, (1 << 64) - 128]
    assert R.value_bits("bool", np.array([True, False])).tolist() == [1, 0]
    ref = R.ref_table([("i8", np.array([-1, 3, -1, 3, 3, 0], dtype=np.int8))], [np.array([1, 1, 1, 1, 1, 0], bool)])
    assert ref.keys.tolist() == [3, (1 << 64) - 1] and ref.counts.tolist() == [3, 2]  # unsigned order
    assert (ref.num_values, ref.num_groups, ref.num_unique) == (5, 2, 0)
    empty = R.ref_table([("i64", np.array([4, 5])), ("utf8", [b"a", b"b"])], [np.zeros(2, bool), None])
    assert (empty.num_values, empty.num_groups, empty.counts.tolist()) == (0, 0, [])


@pytest.mark.parametrize("G", [1, 2, 3, 1000, 65_537])
def test_entropy_of_a_uniform_table_is_ln_G(G):
    for each in (1, 9):
        value, bound = R.ref_entropy(np.full(G, each), G * each)
        assert R.agrees(value, R.ln(G)), (G, each)
        assert bound > 0


def test_mutual_information_reference_identities():
    ax, by = np.array([1, 2, 3, 5, 8]), np.array([1, 4, 9])
    x, y = (v.reshape(-1) for v in np.meshgrid(np.arange(5), np.arange(3), indexing="ij"))
    for scale in (1, 3):
        cells = np.outer(ax, by).reshape(-1) * scale
        value, bound = R.ref_mi((x, y, cells), int(cells.sum()))
        assert R.agrees(value, 0), mpmath.nstr(value, 20)
        assert 5 * R.U <= bound < 6 * R.U  # 5 u sum pxy, and no |t| to add to it
    # y = x: the entropy of x, also when num_rows counts null rows
    counts = np.array([5, 1, 1, 17, 300])
    ids = np.arange(len(counts))
    for n in (int(counts.sum()), 1000):
        value, _ = R.ref_mi((ids, ids, counts), n)
        assert R.agrees(value, R.ref_entropy(counts, n)[0])
    # depth of the fixed-order reduction: chain + 8 tree levels + the partials
    assert [R.depth(G) for G in (1, 256, 257, 300_000, 1 << 20)] == [10, 10, 11, 2 + 8 + 1024, 4 + 8 + 1024]
