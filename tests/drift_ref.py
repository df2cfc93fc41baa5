"""An independent CPU reference of the distribution distances (deequ_amd/drift.py), over Python dicts {tuple: count}.

Written from the semantics include/dqscan.h states, not from the kernel:

    N = the sum of a dict's counts;  p = count_a / N_a,  q = count_b / N_b,  0 for a group a dict lacks
    linf = max |p - q|                       per group in numpy float64: the value the device must match bit for bit
    tv   = 1/2 sum |p - q|                   math.fsum of the float64 terms
    js   = 1/2 sum [p ln(p/m) + q ln(q/m)]   m = (p + q) / 2, a zero p (q) contributing 0; math.fsum
    ks   = max_x |F_a(x) - F_b(x)|           F = an exact integer cumulative count, divided once, in numpy float64

A dict's keys are tuples of canonical values: canon() maps a float to ("f", its bits) -- every NaN one key, -0.0 and
0.0 two -- and a str to its UTF-8 bytes, so Python's own equality (nan != nan, 0.0 == -0.0) never decides a group.
"""
import math
import struct
from collections import Counter

import numpy as np

F64_NAN = 0x7FF8000000000000
F32_NAN = 0x7FC00000


def canon(v, f32=False):
    if isinstance(v, float):
        if f32:
            bits = struct.unpack("<I", struct.pack("<f", v))[0]
            return ("f", F32_NAN if math.isnan(v) else bits)
        return ("f", F64_NAN if math.isnan(v) else struct.unpack("<Q", struct.pack("<d", v))[0])
    if isinstance(v, str):
        return v.encode("utf-8")
    return v


def freq(rows, f32=False):
    """{tuple: count} of rows (tuples, or single values); a row with a None is no part of the distribution."""
    out = Counter()
    for r in rows:
        t = r if isinstance(r, tuple) else (r,)
        if None not in t:
            out[tuple(canon(v, f32) for v in t)] += 1
    return dict(out)


def distances(a: dict, b: dict) -> dict:
    """linf / tv / js, the join's integer counts, and linf_groups: every (group, side) that attains linf (side 0: a
    group of a, 1: of b alone) -- the device breaks ties by key word, which this reference does not know."""
    na, nb = np.float64(sum(a.values())), np.float64(sum(b.values()))
    groups = list(a) + [g for g in b if g not in a]
    diffs, terms = [], []
    for g in groups:
        p = np.float64(a[g]) / na if g in a else np.float64(0.0)
        q = np.float64(b[g]) / nb if g in b else np.float64(0.0)
        diffs.append(np.abs(p - q))
        m = (p + q) / np.float64(2.0)
        t = 0.0
        if p > 0:
            t += float(p) * math.log(float(p / m))
        if q > 0:
            t += float(q) * math.log(float(q / m))
        terms.append(t)
    linf = max(diffs)
    return {
        "linf": float(linf), "tv": 0.5 * math.fsum(float(d) for d in diffs), "js": 0.5 * math.fsum(terms),
        "common": sum(1 for g in a if g in b), "only_a": sum(1 for g in a if g not in b),
        "only_b": sum(1 for g in b if g not in a),
        "count_only_a": sum(c for g, c in a.items() if g not in b),
        "count_only_b": sum(c for g, c in b.items() if g not in a),
        "union": len(groups),
        "linf_groups": {(g, 0 if g in a else 1) for g, d in zip(groups, diffs) if d == linf},
    }


def tolerance(union: int) -> float:
    """The absolute bound on tv and js: 16 (G + 1) 2^-53 -- about 8 roundings per term on a magnitude <= max(p, q),
    non-negative terms, and a summation error of at most G 2^-53 times a total <= 2."""
    return 16.0 * (union + 1) * 2.0 ** -53


def _float_rank(bits: int, width: int) -> int:
    """A float's place in the order from its bits (sign-magnitude): numerically, with -0.0 immediately below 0.0,
    -inf and +inf in their places and the canonical NaN (sign clear, above +inf's bits) greatest."""
    sign = 1 << (width - 1)
    return -(bits & (sign - 1)) - 1 if bits & sign else bits


def ks(a: dict, b: dict, float_width: int = 64) -> float:
    """The two-sample Kolmogorov-Smirnov statistic of two single-column dicts: integers order numerically, floats
    (canonical ("f", bits) values of float_width bits) by _float_rank."""
    import bisect

    def rank(g):
        v = g[0]
        return _float_rank(v[1], float_width) if isinstance(v, tuple) else v

    na, nb = np.float64(sum(a.values())), np.float64(sum(b.values()))
    pa = sorted((rank(g), c) for g, c in a.items())
    pb = sorted((rank(g), c) for g, c in b.items())
    xa, xb = [r for r, _ in pa], [r for r, _ in pb]
    cum_a = [0] + list(np.cumsum([c for _, c in pa], dtype=np.int64))  # exact integer cumulative counts
    cum_b = [0] + list(np.cumsum([c for _, c in pb], dtype=np.int64))
    best = np.float64(0.0)
    for x in sorted(set(xa) | set(xb)):
        fa = np.float64(cum_a[bisect.bisect_right(xa, x)]) / na
        fb = np.float64(cum_b[bisect.bisect_right(xb, x)]) / nb
        best = max(best, np.abs(fa - fb))
    return float(best)
