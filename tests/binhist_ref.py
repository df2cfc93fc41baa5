"""Independent reference for binned histograms: numpy only, nothing of deequ_amd.binning's slot logic.

slot_counts(values, valid, edges, kind) -> int64[k + 3] in the order [below, bin 0 .. bin k-1, above, nan]:
  * integers become binary64 with astype(float64) (round to nearest-even), decimals with float(Decimal) (correctly
    rounded), f32 with astype(float64) (exact);
  * the bin is np.searchsorted(edges, x, side="right") - 1, with x == e[k] moved into the last bin;
  * below / above / NaN by explicit masks; NULL rows (valid False) are dropped.
row_slots gives the same per row (-1: NULL), for building the column of labels a binning UDF would return.
default_labels(edges) are hand-formatted here by a Java-Double.toString restatement of this file's own.
"""
from decimal import Decimal

import numpy as np


def to_f64(values, kind="f64"):
    """values: a numpy array (f64 / f32 / integer kinds) or, kind == "decimal", a list of decimal.Decimal."""
    if kind == "decimal":
        return np.array([float(Decimal(v)) for v in values], dtype=np.float64)
    return np.asarray(values).astype(np.float64)


def row_slots(values, valid, edges, kind="f64"):
    """Per row the slot index (0 below, 1 + i bin i, k + 1 above, k + 2 nan), -1 for a NULL row."""
    e = np.asarray(edges, dtype=np.float64)
    k = len(e) - 1
    x = to_f64(values, kind)
    nan = np.isnan(x)
    below = ~nan & (x < e[0])
    above = ~nan & (x > e[k])
    inside = ~(nan | below | above)
    idx = np.searchsorted(e, x[inside], side="right") - 1
    idx[idx == k] = k - 1  # x == e[k]: the last bin is closed on the right
    slots = np.empty(len(x), dtype=np.int64)
    slots[inside] = idx + 1
    slots[below] = 0
    slots[above] = k + 1
    slots[nan] = k + 2
    if valid is not None:
        slots[~np.asarray(valid, dtype=bool)] = -1  # NULLs dropped
    return slots


def slot_counts(values, valid, edges, kind="f64"):
    s = row_slots(values, valid, edges, kind)
    return np.bincount(s[s >= 0], minlength=len(edges) + 2).astype(np.int64)


def java_double(d):
    """java.lang.Double.toString for the finite doubles the tests use as edges."""
    d = float(d)
    if d == 0.0:
        return "0.0"
    if 1e-3 <= abs(d) < 1e7:
        r = repr(d)
        return r if "." in r else r + ".0"
    mant, exp = np.format_float_scientific(d, unique=True, trim="0", exp_digits=1).split("e")
    if "." not in mant:
        mant += ".0"
    return f"{mant}E{int(exp)}"


def default_labels(edges):
    s = [java_double(x) for x in edges]
    k = len(s) - 1
    return ([f"< {s[0]}"] + [f"[{s[i]}, {s[i + 1]})" for i in range(k - 1)] + [f"[{s[k - 1]}, {s[k]}]"]
            + [f"> {s[k]}", "NaN"])


def distribution(counts, labels, n_rows, max_detail_bins=1000):
    """(values: {label: (absolute, ratio)}, numberOfBins) as Histogram's metric: groups of equal label merged, empty
    ones dropped, NULLs (n_rows minus the counted rows) under "NullValue", the max_detail_bins largest kept (the
    tests avoid ties at the cut)."""
    groups = {}
    for lab, c in zip(labels, counts):
        if int(c):
            groups[lab] = groups.get(lab, 0) + int(c)
    nulls = int(n_rows) - int(np.sum(counts))
    if nulls:
        groups["NullValue"] = groups.get("NullValue", 0) + nulls
    bins = len(groups)
    top = sorted(groups.items(), key=lambda kv: -kv[1])[:max_detail_bins]
    return {lab: (c, c / n_rows) for lab, c in top}, bins
