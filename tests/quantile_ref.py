"""A plain reference of the quantile select and of the quantile state's digest (test_quantile_ref_host.py,
test_quantile_edges_gpu.py).

It shares no formulation with the kernel (dq_quantile.hip's order keys) or with the oracle's key transform: doubles
are ordered by java.lang.Double.compare written out as a comparator over Python floats -- numeric < / > first, then
-0.0 < 0.0 by the sign, every NaN (whatever its payload or sign) equal to every other NaN and above everything else
-- with no look at a double's bits.  Integers are Python ints.  The sorted list is indexed by rank directly.
"""
from __future__ import annotations

import functools
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np


def compare_f64(a: float, b: float) -> int:
    """java.lang.Double.compare(a, b) as -1 / 0 / 1."""
    if a < b:
        return -1
    if a > b:
        return 1
    a_nan, b_nan = a != a, b != b
    if a_nan or b_nan:  # (neither < nor > held: at least one NaN)
        return 0 if a_nan and b_nan else (1 if a_nan else -1)
    if a == 0.0 and b == 0.0:  # equal numbers: only the zeros differ, by sign
        sa, sb = math.copysign(1.0, a), math.copysign(1.0, b)
        return -1 if sa < sb else (1 if sa > sb else 0)
    return 0


def ordered(values, valid) -> list:
    """The non-null values in ascending order: Python floats (Double.compare) or Python ints."""
    v = np.asarray(values)
    keep = np.asarray(valid, dtype=bool)
    if v.dtype.kind == "f":
        return sorted((float(x) for x in v[keep].astype(np.float64)), key=functools.cmp_to_key(compare_f64))
    return sorted(int(x) for x in v[keep])


def select_ordered(srt: list, quantiles: Sequence[float], relative_error: float) -> Optional[List[float]]:
    """QuantileSummaries.query's rank rule over an `ordered` list."""
    n = len(srt)
    if n == 0:
        return None
    out = []
    for q in quantiles:
        if q <= relative_error:
            r = 1
        elif q >= 1 - relative_error:
            r = n
        else:
            r = min(n, max(1, math.ceil(q * n)))
        out.append(float(srt[r - 1]))
    return out


def select(values, valid, quantiles: Sequence[float], relative_error: float) -> Optional[List[float]]:
    """The order statistic each quantile answers: rank 1 if q <= err, rank n if q >= 1 - err, else ceil(q n) clamped
    to [1, n]; None when nothing is valid."""
    return select_ordered(ordered(values, valid), quantiles, relative_error)


def digest_ordered(srt: list, rel: float) -> Tuple[int, List[Tuple[float, int, int]]]:
    n = len(srt)
    if n == 0:
        return 0, []
    e = 0.0 if rel == 0.0 else 1 / (1 / rel)
    s = max(1, math.floor(2 * e * n))
    ranks = list(range(1, n + 1, s))
    if ranks[-1] != n:
        ranks.append(n)
    out, prev = [], 0
    for r in ranks:
        out.append((float(srt[r - 1]), r - prev, 0))
        prev = r
    return n, out


def digest(values, valid, rel: float) -> Tuple[int, List[Tuple[float, int, int]]]:
    """(n, [(value, g, 0), ...]) at ranks 1, 1 + s, ..., n with s = max(1, floor(2 e n)), e = 1 / (1 / rel); g is
    the gap to the rank before."""
    return digest_ordered(ordered(values, valid), rel)


def same(a: float, b: float) -> bool:
    """Bit-exact up to the NaN payload: NaN matches NaN, zeros match by sign."""
    if a != a or b != b:
        return a != a and b != b
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)


def same_samples(got, want) -> bool:
    got, want = list(got), list(want)
    return len(got) == len(want) and all(same(a[0], b[0]) and tuple(a[1:]) == tuple(b[1:]) for a, b in zip(got, want))
