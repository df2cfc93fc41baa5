"""Plain numpy / mpmath reference of the grouping pass (deequ_amd/csrc/dq_group.hip), independent of the oracle and of
the product: the exact frequency table of a set of key columns, and Entropy / MutualInformation as 50-digit values
with a derived bound on what the kernels' double arithmetic may lose.

The frequency table
-------------------
``ref_table(cols, valid)`` counts the rows whose key columns are all non-null (FrequencyBasedAnalyzer.computeFrequencies,
GroupingAnalyzers.scala:44-82).  A fixed-width value's key is its value bits under the rules of ``value_bits``
(``fixed_bits`` in dq_freq_table.h): any f64 / f32 NaN becomes the canonical NaN, -0.0 and 0.0 stay distinct,
integers are sign-extended to 64 bits, a bool is 0 or 1.  For one fixed-width column the table is what ``FreqTable.export()`` must
return: the keys as uint64 in ascending unsigned order and their int64 counts.  Strings and tuples are grouped by a
hash on the device, which this file does not predict: their counts come back as a sorted list (a multiset), together
with each column's marginal counts.

Entropy and MutualInformation: value and bound
----------------------------------------------
Both values are sums over the groups, evaluated with mpmath at 50 digits from the integer counts (ln of an integer is
memoised, so a table of many groups with few distinct counts is cheap).  ``bound`` is the first-order bound of the
rounding error of the double algorithm in ``summary_part`` / ``summary_final`` and ``mi_part`` / ``mi_final``
(dq_group.hip), with u = 2**-53 the unit roundoff; every |delta| below is at most u.

Entropy, one group of count c among N rows, p = c / N, t = -p ln p.  The kernel computes
    ph = fl(c / N) = p (1 + d1)                      (c and N are exact doubles; the quotient is rounded once)
    Lh = log(ph) (1 + e),  |e| <= k_log u            (the device's log)
    th = fl(-ph Lh) = -ph Lh (1 + d2)
With ln ph = ln p + d1 to first order,
    th - t = -p d1 (ln p + 1) + t (e + d2),   so   |th - t| <= u [ p |ln p + 1| + (k_log + 1) |t| ].
The bound used is u [ p |ln p + 1| + (k_log + 2) |t| ]: the further u |t| is spare (it also covers the term being
added into its accumulator by a fused multiply-add or by a separate rounded product).

MutualInformation, one joint group of count c with marginals a and b, pxy = c / N, r = pxy / ((a / N)(b / N)),
t = pxy ln r.  The kernel computes
    q = fl(c / N) = pxy (1 + d1),  fl(a / N) (1 + d2),  fl(b / N) (1 + d3),  their product (1 + d4),
    rh = fl(q / product) = r (1 + h),  h = d1 - d2 - d3 - d4 + d5,  |h| <= 5 u     (four quotients and the product)
    Lh = log(rh) (1 + e),  th = fl(q Lh) = q Lh (1 + d6)
With ln rh = ln r + h,
    th - t = pxy h + t (d1 + e + d6),   so   |th - t| <= u [ 5 pxy + (k_log + 2) |t| ].
The first part does not vanish where t does: for independent columns every r is 1, the truth is 0, and what is left
is the 5 u pxy per group (5 u in all, as the pxy sum to at most 1).

k_log.  The ROCm installation the project builds with carries no accuracy table of its device math library (ocml ships
as bitcode only), so k_log = 2 is ASSUMED.  It enters as a relative error of k_log u of the logarithm; one unit in the
last place of L is at most 2 u |L|, so k_log = 2 admits a log that is accurate to one ulp.

Summation.  Block b of nb = min(1024, ceil(G / 256)) blocks gives each of its 256 threads the groups b*256 + thread,
+ nb*256, ...: a chain of at most ceil(G / (nb 256)) additions; the block's tree adds 8 levels; ``summary_final`` /
``mi_final`` add the nb partials in order.  A computed term therefore passes through at most
    depth = ceil(G / (nb 256)) + 8 + nb
additions, each of which rounds a partial sum no larger than the sum of |t|, so the summation loses at most
    depth u sum |t|
to first order.  The bound is the sum of the per-term bounds plus this.  Second-order terms and the growth of partial
sums beyond sum |t| are what the GPU tests' factor 2 is for; a double evaluation in the same order on the host has to
fit inside the bound itself (tests/test_group_ref_host.py).  The summation term belongs to the order of summation: an
evaluation that adds the G terms one after the other (the oracle's ``sum``) passes its first term through G - 1
additions, far more than `depth` for thousands of groups, and its observed error (about sqrt(G) u sum |t|) does exceed
the kernels' bound there.  ``additions=`` evaluates the same derivation for such an order.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import mpmath
import numpy as np

U = 2.0 ** -53
K_LOG = 2  # assumed: see the module docstring
DPS = 50

_INT = {"i64": np.int64, "i32": np.int32, "i16": np.int16, "i8": np.int8, "date32": np.int32, "timestamp": np.int64}
STRING = ("utf8", "large_utf8")


def value_bits(dtype: str, values) -> np.ndarray:
    """uint64 grouping key of every value of a fixed-width column (fixed_bits in dq_freq_table.h)."""
    if dtype == "f64":
        b = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).copy()
        b[(b & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)] = np.uint64(0x7FF8000000000000)
        return b
    if dtype == "f32":
        b = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).copy()
        b[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0x7FC00000)
        return b.astype(np.uint64)
    if dtype == "bool":
        return np.asarray(values, dtype=bool).astype(np.uint64)
    if dtype in _INT:
        return np.ascontiguousarray(values, dtype=_INT[dtype]).astype(np.int64).view(np.uint64)
    raise ValueError(f"not a fixed-width grouping type: {dtype}")


@dataclass
class RefTable:
    keys: Optional[np.ndarray]     # one fixed-width column: uint64 value bits, ascending; else None
    counts: np.ndarray             # int64: in key order (one fixed-width column), else sorted ascending
    marginals: List[np.ndarray]    # per key column: the sorted counts of its values over the grouped rows
    num_values: int                # rows with every key column non-null
    joint: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]  # two columns: (x id, y id, count) per joint group

    @property
    def num_groups(self) -> int:
        return int(len(self.counts))

    @property
    def num_unique(self) -> int:
        return int((self.counts == 1).sum())


def _ids(dtype: str, values, sel: np.ndarray) -> np.ndarray:
    """Dense ids (0 .. distinct - 1) of the selected rows' values of one column."""
    if dtype in STRING:
        picked = np.empty(int(sel.sum()), dtype=object)
        picked[:] = [values[i] for i in np.flatnonzero(sel)]
        return np.unique(picked, return_inverse=True)[1].reshape(-1) if len(picked) else np.zeros(0, np.int64)
    return np.unique(value_bits(dtype, values)[sel], return_inverse=True)[1].reshape(-1)


def ref_table(cols: Sequence[Tuple[str, object]], valid: Sequence[Optional[np.ndarray]]) -> RefTable:
    """cols: (dtype, values) per key column -- a numpy array, or a list of bytes for a string column (entries of
    null rows are ignored); valid: per column a bool array, or None for a column without nulls."""
    n = len(cols[0][1])
    sel = np.ones(n, dtype=bool)
    for v in valid:
        if v is not None:
            sel &= np.asarray(v, dtype=bool)
    nv = int(sel.sum())
    if len(cols) == 1 and cols[0][0] not in STRING:
        keys, counts = np.unique(value_bits(cols[0][0], cols[0][1])[sel], return_counts=True)
        counts = counts.astype(np.int64)
        return RefTable(keys, counts, [np.sort(counts)], nv, None)
    ids = [_ids(dt, vals, sel) for dt, vals in cols]
    marginals = [np.sort(np.bincount(i).astype(np.int64)) if nv else np.zeros(0, np.int64) for i in ids]
    comb = ids[0].astype(np.int64)
    for i in ids[1:]:  # both factors are below the row count, so the product stays far below 2^63
        comb = np.unique(comb * (int(i.max()) + 1 if nv else 1) + i, return_inverse=True)[1].reshape(-1).astype(np.int64)
    first, counts = (np.unique(comb, return_index=True, return_counts=True)[1:] if nv
                     else (np.zeros(0, np.int64), np.zeros(0, np.int64)))
    counts = counts.astype(np.int64)
    joint = (ids[0][first], ids[1][first], counts.copy()) if len(cols) == 2 else None
    return RefTable(None, np.sort(counts), marginals, nv, joint)


def launched_blocks(G: int) -> int:
    """nb of dq_freq_summarize / mi_from_groups: min(kSumBlocks = 1024, ceil(G / 256))."""
    return max(1, min(1024, (G + 255) // 256))


def depth(G: int) -> int:
    nb = launched_blocks(G)
    return -(-G // (nb * 256)) + 8 + nb


class _Ln:
    """ln of positive integers at the working precision, each computed once."""

    def __init__(self):
        self.seen = {}

    def __call__(self, k: int):
        v = self.seen.get(k)
        if v is None:
            v = self.seen[k] = mpmath.log(mpmath.mpf(k))
        return v


def ref_entropy(counts, num_rows: int, k_log: int = K_LOG, additions: Optional[int] = None):
    """(value, bound): sum over the groups of -(c / N) ln(c / N) (Entropy.scala:29-41) at 50 digits, and the
    first-order rounding bound of the kernels' double evaluation (module docstring).  `additions`: the number of
    additions a term passes through at most, for an evaluation in another order than the kernels' (default: depth(G))."""
    counts = np.asarray(counts, dtype=np.int64)
    G = len(counts)
    with mpmath.workdps(DPS):
        ln, N, u = _Ln(), mpmath.mpf(int(num_rows)), mpmath.mpf(U)
        value = sum_abs = per_term = mpmath.mpf(0)
        for c, mult in zip(*np.unique(counts[counts != 0], return_counts=True)):
            p = mpmath.mpf(int(c)) / N
            lnp = ln(int(c)) - ln(int(num_rows))
            t = -p * lnp
            value += int(mult) * t
            sum_abs += int(mult) * abs(t)
            per_term += int(mult) * u * (p * abs(lnp + 1) + (k_log + 2) * abs(t))
        bound = per_term + (depth(G) if additions is None else additions) * u * sum_abs
        return value, float(bound)


def ref_mi(joint, num_rows: int, k_log: int = K_LOG, additions: Optional[int] = None):
    """(value, bound) of MutualInformation (MutualInformation.scala:53-56) from the joint groups (x id, y id, count):
    sum of (c / N) ln((c / N) / ((a / N)(b / N))), a and b the marginal counts summed from the joint counts;
    `additions` as for ref_entropy."""
    x, y, c = (np.asarray(v, dtype=np.int64) for v in joint)
    G = len(c)
    if G:
        a = np.zeros(int(x.max()) + 1, np.int64)
        np.add.at(a, x, c)
        b = np.zeros(int(y.max()) + 1, np.int64)
        np.add.at(b, y, c)
        triples = np.stack([c, a[x], b[y]], axis=1)
    else:
        triples = np.zeros((0, 3), np.int64)
    with mpmath.workdps(DPS):
        ln, N, u = _Ln(), mpmath.mpf(int(num_rows)), mpmath.mpf(U)
        value = sum_abs = per_term = mpmath.mpf(0)
        rows, mults = np.unique(triples, axis=0, return_counts=True) if G else (triples, [])
        for (ci, ai, bi), mult in zip(rows.tolist(), mults):
            pxy = mpmath.mpf(ci) / N
            t = pxy * (ln(ci) + ln(int(num_rows)) - ln(ai) - ln(bi))
            value += int(mult) * t
            sum_abs += int(mult) * abs(t)
            per_term += int(mult) * u * (5 * pxy + (k_log + 2) * abs(t))
        bound = per_term + (depth(G) if additions is None else additions) * u * sum_abs
        return value, float(bound)


def ln(k: int):
    """ln k at 50 digits."""
    with mpmath.workdps(DPS):
        return mpmath.log(mpmath.mpf(int(k)))


def error_ratio(got: float, value, bound: float) -> float:
    """|got - value| / bound, the difference taken at 50 digits."""
    with mpmath.workdps(DPS):
        return float(abs(mpmath.mpf(got) - value) / mpmath.mpf(bound))


def agrees(value, other, digits: int = 40) -> bool:
    """value == other to `digits` significant digits (absolutely, where other is 0)."""
    with mpmath.workdps(DPS):
        scale = abs(other) if other != 0 else mpmath.mpf(1)
        return abs(value - other) <= scale * mpmath.mpf(10) ** -digits
