"""Reference for arithmetic operands of predicates: the Spark 2.2 (non-ANSI) rules restated on Python ints and
numpy.float32 / float64, one value at a time.  It does not call the library.

A value is (type, v): type one of i8 i16 i32 i64 f32 f64, v a Python int / numpy.float32 / numpy.float64, or None for
NULL.  A decimal literal is ("dec", text) until an operator places it beside a Float / Double operand.

  types      Byte < Short < Int < Long < Float < Double
  literals   integer: Int if it fits, else Long; with an exponent: Double; with a point: decimal, cast to Double next to
             a Float / Double operand, refused (Unsupported) anywhere else
  + - * %    both sides cast to the wider type = the result type; integral results wrap at that width; Float results
             are rounded to binary32 after each operation (numpy.float32 arithmetic), Double to binary64; no FMA
  /          both sides cast to Double; divisor == 0 (either zero): NULL
  %          zero divisor: NULL; integral: truncated remainder (sign of the dividend); Float / Double: fmod
  unary -    keeps the type, wraps
  NULL       any NULL operand gives NULL

Java knows one NaN (doubleToLongBits): `same` compares two results bit for bit except that every NaN equals every NaN.
"""
from __future__ import annotations

import numpy as np

RANK = ["i8", "i16", "i32", "i64", "f32", "f64"]
BITS = {"i8": 8, "i16": 16, "i32": 32, "i64": 64}
NP = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
# the library's type codes (include/dqscan.h enum dq_type) and instruction codes (enum dq_expr_op)
TYPE_NAME = {1: "f64", 2: "i64", 3: "i32", 6: "f32", 7: "i16", 8: "i8"}
OP_COL, OP_LIT, OP_CAST, OP_NEG = 1, 2, 3, 4
OP_SYM = {5: "+", 6: "-", 7: "*", 8: "/", 9: "%"}


class Unsupported(Exception):
    pass


def wrap(v: int, t: str) -> int:
    b = BITS[t]
    v &= (1 << b) - 1
    return v - (1 << b) if v >> (b - 1) else v


def literal(text: str):
    if "e" in text.lower():
        return ("f64", np.float64(float(text)))
    if "." in text:
        return ("dec", text)
    v = int(text)
    if not -(1 << 63) <= v < (1 << 63):
        raise Unsupported(text)
    return ("i32", v) if -(1 << 31) <= v < (1 << 31) else ("i64", v)


def cast(x, t: str):
    """Widening cast of a value to type t."""
    ft, v = x
    if ft == t or v is None:
        return (t, v)
    assert RANK.index(t) > RANK.index(ft), (ft, t)
    if t in BITS:
        return (t, v)
    if ft in BITS:  # integral -> Float / Double: one rounding ((float) long in Java)
        return (t, np.int64(v).astype(NP[t]))
    return (t, np.float64(v))  # Float -> Double, exact


def _place(x, other):
    if x[0] != "dec":
        return x
    if other[0] not in ("f32", "f64"):
        raise Unsupported("decimal arithmetic")
    return ("f64", np.float64(float(x[1])))  # (float() of the digits is the correctly rounded value)


def neg(x):
    if x[0] == "dec":
        raise Unsupported("decimal arithmetic")
    t, v = x
    if v is None:
        return x
    return (t, wrap(-v, t)) if t in BITS else (t, -v)


def binary(op: str, x, y):
    x, y = _place(x, y), _place(y, x)
    t = "f64" if op == "/" else RANK[max(RANK.index(x[0]), RANK.index(y[0]))]
    (_, a), (_, b) = cast(x, t), cast(y, t)
    if a is None or b is None:
        return (t, None)
    if op in "/%" and b == 0:
        return (t, None)
    with np.errstate(all="ignore"):
        if t in BITS:
            if op == "%":
                r = abs(a) % abs(b)
                r = -r if a < 0 else r
            else:
                r = a + b if op == "+" else a - b if op == "-" else a * b
            return (t, wrap(r, t))
        f = NP[t]
        a, b = f(a), f(b)
        r = a + b if op == "+" else a - b if op == "-" else a * b if op == "*" else a / b if op == "/" else np.fmod(a, b)
        return (t, f(r))


def eval_postfix(instrs, literals, cols):
    """A postfix program on one row.  instrs: (op, arg, type code); literals: (type code, value); cols: the row's
    values in program-column order.  Only the stack order is taken from the program: CAST instructions and the types
    the instructions state are ignored, the types follow from the operands by the rules above."""
    st = []
    for op, arg, _ in instrs:
        if op == OP_COL:
            st.append(cols[arg])
        elif op == OP_LIT:
            t, v = literals[arg]
            st.append((TYPE_NAME[t], np.float64(v) if TYPE_NAME[t] == "f64" else int(v)))
        elif op == OP_CAST:
            pass
        elif op == OP_NEG:
            st.append(neg(st.pop()))
        else:
            b = st.pop()
            a = st.pop()
            st.append(binary(OP_SYM[op], a, b))
    assert len(st) == 1
    return st[0]


def rows(fn, *columns):
    """fn over rows.  columns: (type, numpy array, valid bool array or None); returns (type, numpy values with 0 in
    NULL rows, valid bool array)."""
    n = len(columns[0][1])
    out_t, vals, ok = None, [], np.zeros(n, bool)
    for r in range(n):
        args = []
        for t, a, valid in columns:
            v = None if valid is not None and not valid[r] else (int(a[r]) if t in BITS else a[r])
            args.append((t, v))
        t, v = fn(*args)
        out_t = t
        ok[r] = v is not None
        vals.append(0 if v is None else v)
    if out_t is None:  # no row: the type of NULL operands
        out_t = fn(*[(t, None) for t, _, _ in columns])[0]
    return out_t, np.array(vals, dtype=NP[out_t]), ok


def same(t: str, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: equal bit for bit, or both NaN."""
    a, b = np.asarray(a, NP[t]), np.asarray(b, NP[t])
    if t in BITS:
        return a == b
    u = np.uint32 if t == "f32" else np.uint64
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))
