"""A plain-Python restatement of RowLevelSchemaValidator (schema/RowLevelSchemaValidator.scala:25-282) as Spark 2.2
evaluates it: one function per per-value rule and one for toCNF.  It is the checker of tests/test_schema_host.py and
tests/test_schema_gpu.py and shares no code with deequ_amd/csrc/dq_schema.h: the rules are written here with Python
integers, `re` and three-valued booleans (None = SQL NULL).

A schema is a list of dicts: {"kind": "int" | "decimal" | "timestamp" | "string", "name", "nullable", and per kind
"min" / "max" (int: values, string: lengths), "precision" / "scale", "mask", "matches"}.  A row is a dict
name -> bytes | None.
"""
from __future__ import annotations

import datetime
import re

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
FIELD_CAP = 10 ** 15  # a timestamp field saturates here (fields of more than 9 digits are outside the pinned domain)

_INT = re.compile(rb"([+-]?)([0-9]*)(?:\.[0-9]*)?")
_DEC = re.compile(rb"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?)([0-9]+))?")


def to_int(b: bytes):
    """Cast(c, IntegerType) = UTF8String.toInt: raw bytes, [+-]digits[.digits], the fraction dropped; None = NULL."""
    m = _INT.fullmatch(b)
    if not b or b in (b"+", b"-") or not m:
        return None
    v = int(m.group(2) or b"0")
    if m.group(1) == b"-":
        v = -v
    return v if INT_MIN <= v <= INT_MAX else None


def to_decimal(b: bytes, p: int, s: int):
    """Cast(c, DecimalType(p, s)): new BigDecimal(text), setScale(s, HALF_UP), NULL past p digits.  The unscaled
    integer, or None."""
    m = _DEC.fullmatch(b)
    if not m:
        return None
    sign, ip, fp, fp2, esign, ed = m.groups()
    frac = fp2 if ip is None else (fp or b"")
    exp = 0
    if ed is not None:
        ed = ed.lstrip(b"0")
        if len(ed) > 10:  # BigDecimal: too many nonzero exponent digits
            return None
        exp = int(ed or b"0") * (-1 if esign == b"-" else 1)
    scale = len(frac) - exp
    if not INT_MIN <= scale <= INT_MAX:  # "Scale out of range"
        return None
    digits = int((ip or b"") + frac)
    if digits == 0:
        return 0
    k = s - scale
    if k >= 0:
        if k > 40:
            return None  # at least 10^40
        u = digits * 10 ** k
    elif -k > len(str(digits)) + 1:
        u = 0
    else:
        q, r = divmod(digits, 10 ** -k)
        u = q + (1 if 2 * r >= 10 ** -k else 0)  # ROUND_HALF_UP on the magnitude
    if u >= 10 ** p:
        return None
    return -u if sign == b"-" else u


_FIELDS = {"y": "year", "M": "month", "d": "day", "H": "hour", "m": "minute", "s": "second"}


def compile_mask(mask: str):
    """The supported SimpleDateFormat subset as a list of ("lit", ch) / (field, None); None when outside it."""
    out, i, prev_field, fields = [], 0, False, 0
    while i < len(mask):
        c = mask[i]
        if c == "'":
            if mask[i + 1:i + 2] == "'":
                out.append(("lit", "'"))
                i += 2
                prev_field = False
                continue
            i += 1
            while True:
                if i >= len(mask):
                    return None  # unterminated quote
                if mask[i] == "'":
                    if mask[i + 1:i + 2] == "'":
                        out.append(("lit", "'"))
                        i += 2
                        continue
                    i += 1
                    break
                if not 0x20 <= ord(mask[i]) < 0x7F:
                    return None
                out.append(("lit", mask[i]))
                i += 1
            prev_field = False
        elif c.isascii() and c.isalpha():
            j = i
            while j < len(mask) and mask[j] == c:
                j += 1
            if c not in _FIELDS or (c == "y" and j - i < 3) or (c == "M" and j - i > 2) or prev_field:
                return None
            out.append((_FIELDS[c], None))
            fields += 1
            prev_field = True
            i = j
        elif c.isdigit() or not 0x20 <= ord(c) < 0x7F:
            return None
        else:
            out.append(("lit", c))
            prev_field = False
            i += 1
    return out if fields and len(out) <= 64 else None


def _days_from_civil(y: int, m: int) -> int:
    """Days from 1970-01-01 to y-m-01, proleptic Gregorian."""
    if 1 <= y <= 9999:
        return datetime.date(y, m, 1).toordinal() - datetime.date(1970, 1, 1).toordinal()
    # outside datetime's range: the 400-year cycle has 146097 days
    cycles, yy = divmod(y - 2000, 400)
    return cycles * 146097 + datetime.date(2000 + yy, m, 1).toordinal() - datetime.date(1970, 1, 1).toordinal()


def parse_timestamp(b: bytes, mask: str):
    """unix_timestamp(c, mask).cast(TimestampType) in UTC: (fields, microseconds as a wrapped int64), or None for
    a ParseException.  fields: name -> (value, digits) of every parsed field (for the pinned-domain test)."""
    els = compile_mask(mask)
    assert els is not None, mask
    f = {"year": 1970, "month": 1, "day": 1, "hour": 0, "minute": 0, "second": 0}
    seen = {}
    i = 0
    for kind, lit in els:
        if kind == "lit":
            if i >= len(b) or b[i] != ord(lit):
                return None
            i += 1
            continue
        while i < len(b) and b[i] in b" \t":
            i += 1
        m = re.compile(rb"(-?)([0-9]+)(?:E(-?)([0-9]+))?").match(b, i)
        if not m:
            return None
        i = m.end()
        v = min(int(m.group(2)), FIELD_CAP)
        ndig = len(m.group(2)) + len(m.group(4) or b"")
        if m.group(4) is not None:
            for _ in range(min(int(m.group(4)), 32)):
                v = v // 10 if m.group(3) else min(v * 10, FIELD_CAP)
        f[kind] = -v if m.group(1) else v
        seen[kind] = (f[kind], ndig)
    months = f["year"] * 12 + f["month"] - 1
    y, m0 = divmod(months, 12)
    days = _days_from_civil(y, m0 + 1) + f["day"] - 1
    secs = days * 86400 + f["hour"] * 3600 + f["minute"] * 60 + f["second"]
    us = (secs * 1_000_000) & ((1 << 64) - 1)
    return seen, us - (1 << 64) if us >> 63 else us


def timestamp_pinned(b: bytes, mask: str) -> bool:
    """Whether the value of a parsed timestamp is promised: every field of at most 9 digits and the date on or
    after 1582-10-15 (the proleptic Gregorian calendar is Java's there)."""
    r = parse_timestamp(b, mask)
    if r is None:
        return False
    seen, us = r
    if any(nd > 9 for _, nd in seen.values()):
        return False
    return us >= (datetime.date(1582, 10, 15).toordinal() - datetime.date(1970, 1, 1).toordinal()) * 86400 * 10 ** 6


def char_count(b: bytes) -> int:
    """length(c): UTF-8 characters."""
    return len(b.decode("utf-8"))


def matches(b: bytes, pattern: str) -> bool:
    """regexp_extract(c, p, 0) != "": the first find() is non-empty (java.util.regex classes are ASCII)."""
    m = re.search(pattern, b.decode("utf-8"), re.ASCII)
    return bool(m) and m.group(0) != ""


# ------------------------------------------------------------------------------------------- three-valued logic
def and3(a, b):
    if a is False or b is False:
        return False
    return None if a is None or b is None else True


def or3(a, b):
    if a is True or b is True:
        return True
    return None if a is None or b is None else False


def cast_value(d: dict, v):
    """castExpression of a definition on a source value: the cast value (None = NULL)."""
    if v is None:
        return None
    if d["kind"] == "int":
        return to_int(v)
    if d["kind"] == "decimal":
        return to_decimal(v, d["precision"], d["scale"])
    if d["kind"] == "timestamp":
        r = parse_timestamp(v, d["mask"])
        return None if r is None else r[1]
    return v


def cnf(schema, row):
    """toCNF (:225-281) of one row: True, False or None."""
    m = True
    for d in schema:
        v = row[d["name"]]
        is_null = v is None
        if not d.get("nullable", True):
            m = and3(m, not is_null)                                     # :230-232
        if d["kind"] == "int":
            x = None if is_null else to_int(v)
            m = and3(m, or3(is_null, x is not None))                    # :243
            if d.get("min") is not None:                                 # :246: colIsNull.isNull is FALSE
                m = and3(m, or3(False, None if x is None else x >= d["min"]))
            if d.get("max") is not None:
                m = and3(m, or3(is_null, None if x is None else x <= d["max"]))  # :250
        elif d["kind"] == "decimal":
            m = and3(m, or3(is_null, (not is_null) and to_decimal(v, d["precision"], d["scale"]) is not None))  # :256
        elif d["kind"] == "timestamp":
            m = and3(m, or3(is_null, (not is_null) and parse_timestamp(v, d["mask"]) is not None))  # :275-276
        else:
            n = None if is_null else char_count(v)
            if d.get("min") is not None:
                m = and3(m, or3(is_null, None if n is None else n >= d["min"]))  # :261
            if d.get("max") is not None:
                m = and3(m, or3(is_null, None if n is None else n <= d["max"]))  # :265
            if d.get("matches") is not None:
                m = and3(m, or3(is_null, None if is_null else matches(v, d["matches"])))  # :270
    return m


def validate(schema, columns, rows):
    """validate (:183-206) over rows (dicts): (valid rows cast, invalid rows untouched), each a list of dicts in
    source order."""
    last = {d["name"]: d for d in schema}  # castExpressions.toMap: a later definition of a name wins
    valid, invalid = [], []
    for row in rows:
        m = cnf(schema, row)
        if m is True:
            valid.append({c: cast_value(last[c], row[c]) if c in last else row[c] for c in columns})
        elif m is False:
            invalid.append(dict(row))
    return valid, invalid


# ------------------------------------------------------------------------------------------- adversarial pools
def int_pool():
    return [b"0", b"7", b"+7", b"-7", b"+", b"-", b"+-1", b"--1", b"-0", b"2147483647", b"2147483648", b"-2147483648",
            b"-2147483649", b"+2147483647", b"+2147483648", b"1.", b"1.x", b".5", b"-.5", b".", b"-.", b"1.9", b"-1.9",
            b"1.2.3", b" 1", b"1 ", b"", b" ", b"\t1", b"1e5", b"N/A", b"0x10", b"00000000000000000012", b"21474836470",
            b"99999999999999999999", b"-99999999999999999999", b"214748364.99", b"12a", "１".encode(), b"1\x00",
            b"123", b"456", b"999999", b"-9", b"-100000", b"1000", b"1001", b"-10", b"-11"]


def decimal_pool():
    c = [b"1.234", b"1.235", b"-1.235", b"-1.234", b"1.2349999999999999999999999999999999999999", b"1.2350000000000000000001",
         b"99999999.994", b"99999999.995", b"-99999999.995", b"9999999.995", b"0.995", b"0.994", b".995", b"-.995",
         b"9" * 38, b"9" * 39, b"-" + b"9" * 38, b"0." + b"9" * 38, b"0." + b"9" * 60, b"0." + b"4" * 60,
         b"1." + b"0" * 60, b"0." + b"0" * 59 + b"1", b"12345678." + b"5" * 60, b"0e999999999", b"0e-999999999",
         b"0.000e999999999", b"1e9999999999", b"1e-9999999999", b"1e09999999999", b"1e99999999999", b"0e99999999999",
         b"1e00000000000000000001", b"1e-00000000000000000001", b"0e9999999999", b"1e2147483647", b"1.5e-2147483647",
         b"1e", b"1e+", b"1e-", b".", b"", b"+", b"-", b"NaN", b"Infinity", b"1d", b"1f", b"0x1p3", b"1.", b"+.5", b"-.5",
         b"+1.", b"1.e2", b".5e1", b"e5", b".e5", b"1e5", b"1E5", b"1e+5", b"1e-5", b"1e7", b"1e8", b"12e6", b"12.5e-1",
         b"1..5", b"1.5.", b" 1", b"1 ", b"1_0", b"1,0", b"--1", b"+-1", b"299.000", b"1295", b"###", b"-19.99",
         b"-99.99", b"n/a", "１".encode(), b"0", b"-0", b"-0.001", b"-0.005", b"0.005", b"0.0049", b"5e-3", b"49e-4",
         b"00000000000000000000000000000000000000000012.5", b"1" + b"0" * 7, b"1" + b"0" * 8, b"99999999", b"100000000"]
    return c


def timestamp_pool():
    return [b"2012-07-22 22:59:59", b"2012-07-22 22:21:59", b"N/A", b"yesterday night", b"", b"2012-07-22  22:59:59",
            b"2012-07-22 \t22:59:59", b"  2012-07-22 22:59:59", b"2012- 07-22 22:59:59", b"2012-13-45 25:61:61",
            b"-1-07-22 22:59:59", b"+1-07-22 22:59:59", b"2012--7-22 22:59:59", b"12E1-07-22 22:59:59",
            b"2012E-07-22 22:59:59", b"2012-07-22 22:59:59E", b"2012-07-22 22:59:59 and more", b"2012-07-22 22:59:59Z",
            b"2012-07-22 22:59", b"2012-07-22 22:59:", b"2012-07-22", b"2012/07/22 22:59:59", b"2012-07-22T22:59:59",
            b"2012-07-22 22.59.59", b"1970-01-01 00:00:00", b"1969-12-31 23:59:59", b"1582-10-15 00:00:00",
            b"1582-10-14 00:00:00", b"0001-01-01 00:00:00", b"9999-12-31 23:59:59", b"2012-00-00 00:00:00",
            b"2012-7-2 3:4:5", b"02012-007-022 022:059:059", b"2012-07-22 22:59:5x", b"2012-07-22 22:59:x5",
            b"2000-02-29 12:00:00", b"1900-02-29 12:00:00", b"2012-07-22 24:00:00", b"2012-07-22 22:59:-1",
            b"1234567890-07-22 22:59:59", b"2012-07-22 22:59:59E2", b"2012-07-22 22:59:5E1", b"2012-07-22 22:59:50E-1",
            "２０１２-07-22 22:59:59".encode(), b"2012-07-22\t22:59:59", b"2012 -07-22 22:59:59"]


QUOTED_MASK = "yyyy.MM.dd 'at' HH'h'mm''ss"


def quoted_timestamp_pool():
    return [b"2012.07.22 at 22h59'59", b"2012.07.22 at 22h59'5", b"2012.07.22 AT 22h59'59", b"2012.07.22 at 22h59 59",
            b"2012.07.22 at22h59'59", b"2012.07.22 at  22h59'59", b"2012.07.22 at 22 h59'59", b"2012-07-22 at 22h59'59",
            b"2012.07.22 at 22h59'", b"2012.07.22 at 22h59''59", b" 2012. 07. 22 at 22h 59' 59"]


def string_pool():
    return [b"", b"a", b"ab", b"abc", b"abcd", b"abcde", b"abcdef", "é".encode(), "éa".encode(), "ééé".encode(),
            "éééé".encode(), "ééééé".encode(), "éééééé".encode(), "日本語".encode(), "日本語テキ".encode(), "日本語テキス".encode(),
            "😀".encode(), "😀😀😀".encode(), "😀😀😀😀😀".encode(), "a😀é日b".encode(), "a😀é日bc".encode(),
            b"hello", b"Hello", b"hello123", b"hello world", b"hello_-x", b"Spa" + b"a" * 50 + b"m", b"&&%%%/&/&/&asdaf",
            b"H.", b"Hello World", b"abc de", b"ABC", b"a-b", b"a b", b"12345", b"     ", b"\t"]


MAIN_MASK = "yyyy-MM-dd HH:mm:ss"
NAME_REGEX = "^[a-z0-9_\\-\\s]+$"


def mixed_schema():
    """One column per kind (and `extra`, which the schema does not name, passes through)."""
    return [{"kind": "int", "name": "id", "nullable": True, "min": -10, "max": 1000000},
            {"kind": "decimal", "name": "amount", "precision": 10, "scale": 2, "nullable": True},
            {"kind": "timestamp", "name": "created", "mask": MAIN_MASK, "nullable": False},
            {"kind": "string", "name": "name", "nullable": True, "min": 1, "max": 11, "matches": NAME_REGEX}]


MIXED_COLUMNS = ["id", "extra", "amount", "created", "name"]


def mixed_rows(n: int, seed: int = 11):
    """n rows over the adversarial pools: per column mostly values its rule accepts, a few NULLs, the rest any pool
    value, so that rows of all three outcomes occur."""
    import random

    rng = random.Random(seed)
    sch = {d["name"]: d for d in mixed_schema()}
    pools = {"id": int_pool(), "amount": decimal_pool(), "created": timestamp_pool(), "name": string_pool()}
    good = {c: [v for v in p if cnf([dict(sch[c], nullable=True)], {c: v}) is True] for c, p in pools.items()}
    rows = []
    for i in range(n):
        row = {"extra": None if i % 7 == 3 else b"x%d" % i}
        for c, p in pools.items():
            r = rng.random()
            row[c] = None if r < 0.04 else rng.choice(good[c]) if r < 0.85 else rng.choice(p)
        rows.append(row)
    return rows
