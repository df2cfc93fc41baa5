"""The defining rule of segmented metrics, restated without the device: split the rows by the tuple of the segment
columns (a NULL in any of them: the single segment None), then compute each analyzer on each part as the ordinary
analyzers define it.  Pure Python; float sums are math.fsum.

A part is a list of rows; an analyzer is described by `kind` and per-row lists cut to the part:
  values  the column's values (None: NULL);  where / pred  SQL three-valued outcomes True / False / None per row
  (where None: no filter).  metric() returns ("ok", value) or ("empty",) -- the analyzer's empty-state failure.
"""
import math
from fractions import Fraction


def split(keys):
    """{key tuple or None: [row numbers ascending]} of per-row key tuples (a None inside a tuple: a NULL key)."""
    parts = {}
    for r, k in enumerate(keys):
        k = tuple(k) if isinstance(k, (tuple, list)) else (k,)
        parts.setdefault(None if any(v is None for v in k) else k, []).append(r)
    return parts


def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def float_sum(xs):
    """The sum of doubles as an order-independent reference: NaN if any NaN or both infinities, an infinity if one
    sign of it occurs, else fsum."""
    if any(x != x for x in xs):
        return math.nan
    pos, neg = any(x == math.inf for x in xs), any(x == -math.inf for x in xs)
    if pos or neg:
        return math.nan if pos and neg else (math.inf if pos else -math.inf)
    return math.fsum(xs)


def exact_sd(xs):
    """The population standard deviation of finite doubles from exact rational arithmetic, and m2."""
    f = [Fraction(x) for x in xs]
    mean = sum(f) / len(f)
    m2 = sum((x - mean) ** 2 for x in f)
    return math.sqrt(m2 / len(f)), float(m2)


def spark_order_sd(xs):
    """Spark's CentralMomentAgg over the rows in order on one partition (the update of tests/test_moments_adversarial's
    Spark column): the metric sqrt(m2 / n)."""
    n = avg = m2 = 0.0
    for x in xs:
        n += 1.0
        delta = x - avg
        dn = delta / n
        avg += dn
        m2 += delta * (delta - dn)
    return math.sqrt(m2 / n)


def metric(kind, n_rows, values=None, where=None, pred=None, integral=False):
    applies = [True] * n_rows if where is None else [w is True for w in where]
    where_known = where is None or any(w is not None for w in where)
    if kind == "Size":
        if where is None:
            return ("ok", float(n_rows))
        return ("ok", float(sum(applies))) if where_known else ("empty",)
    if kind == "Completeness":
        if not where_known or n_rows == 0:
            return ("empty",)
        cnt = sum(applies)
        return ("ok", math.nan if cnt == 0 else sum(1 for v, a in zip(values, applies) if a and v is not None) / cnt)
    if kind == "Compliance":
        if not where_known or not any(a and p is not None for p, a in zip(pred, applies)):
            return ("empty",)
        cnt = sum(applies)
        return ("ok", math.nan if cnt == 0 else sum(1 for p, a in zip(pred, applies) if a and p is True) / cnt)
    xs = [v for v, a in zip(values, applies) if a and v is not None]
    if not xs:
        return ("empty",)
    if kind in ("Sum", "Mean"):
        s = float(_wrap64(sum(int(x) for x in xs))) if integral else float_sum([float(x) for x in xs])
        return ("ok", s if kind == "Sum" else s / len(xs))
    xs = [float(x) for x in xs]
    if kind == "StandardDeviation":
        if any(not math.isfinite(x) for x in xs):
            return ("ok", math.nan)
        return ("ok", exact_sd(xs)[0])
    nan = [x for x in xs if x != x]
    rest = [x for x in xs if x == x]
    if kind == "Minimum":
        if not rest:
            return ("ok", math.nan)
        m = min(rest)
        return ("ok", -0.0 if m == 0.0 and any(x == 0.0 and math.copysign(1.0, x) < 0 for x in rest) else m)
    if kind == "Maximum":
        if nan:
            return ("ok", math.nan)
        m = max(rest)
        return ("ok", 0.0 if m == 0.0 and any(x == 0.0 and math.copysign(1.0, x) > 0 for x in rest) else m)
    raise ValueError(kind)


def sum_bound(xs):
    """|any-order double sum - fsum| <= n 2^-53 sum|x| over the n finite values."""
    xs = [float(x) for x in xs]
    if not xs or any(not math.isfinite(x) for x in xs):
        return 0.0
    return len(xs) * 2.0 ** -53 * math.fsum(abs(x) for x in xs)
