"""RowLevelSchemaValidator's rules on the CPU: the plain-Python restatement (tests/schema_ref.py) reproduces the
seven cases of the reference's RowLevelSchemaValidatorTest (tests/golden/schema_validator_kats.json), and
dq_schema_check_host -- deequ_amd/csrc/dq_schema.h, the rules the verdict kernel runs, over host bytes -- equals the
restatement on an adversarial list per rule and on mixed rows of all three outcomes.  The same header is also driven
stand-alone under ASan + UBSan (tools/schema_rules_check.cpp).  tests/test_schema_gpu.py runs the lists on the device.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import schema_ref as R
from tests.conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"


def load_kats():
    with open(os.path.join(ROOT, "tests", "golden", "schema_validator_kats.json")) as f:
        return json.load(f)["cases"]


def kat_rows(case):
    return [{c: None if v is None else v.encode() for c, v in zip(case["columns"], row)} for row in case["rows"]]


def render(d, v):
    """A cast value as the KAT file writes it."""
    if v is None:
        return None
    if d is not None and d["kind"] == "decimal":
        sign, u, s = "-" if v < 0 else "", str(abs(v)).rjust(d["scale"] + 1, "0"), d["scale"]
        return sign + (u[:-s] + "." + u[-s:] if s else u)
    return v.decode() if isinstance(v, bytes) else v


def check_kat(case, valid, invalid, n_valid, n_invalid):
    """The assertions of one reference case over valid / invalid rows (dicts of rendered values)."""
    assert (n_valid, n_invalid) == (case["numValidRows"], case["numInvalidRows"]) == (len(valid), len(invalid))
    if "valid" in case:
        got = {r[case["valid"]["column"]] for r in valid}
        assert len(got) == n_valid and set(case["valid"]["contains"]) <= got, got
    if "invalid" in case:
        got = {r[case["invalid"]["column"]] for r in invalid}
        assert set(case["invalid"].get("contains", [])) <= got and not set(case["invalid"].get("excludes", [])) & got
    if "disjoint" in case:
        assert not {r[case["disjoint"]] for r in valid} & {r[case["disjoint"]] for r in invalid}
    if "invalidPrefixCounts" in case:
        pc = dict(case["invalidPrefixCounts"])
        col = pc.pop("column")
        for prefix, count in pc.items():
            assert sum(1 for r in invalid if r[col].startswith(prefix)) == count


@pytest.mark.parametrize("case", load_kats(), ids=lambda c: c["lines"])
def test_restatement_reproduces_kat(case):
    last = {d["name"]: d for d in case["schema"]}
    valid, invalid = R.validate(case["schema"], case["columns"], kat_rows(case))
    check_kat(case, [{c: render(last.get(c), v) for c, v in r.items()} for r in valid],
              [{c: render(None, v) for c, v in r.items()} for r in invalid], len(valid), len(invalid))


# ---------------------------------------------------------------------------------- dq_schema_check_host via ctypes
def make_defs(L, schema, columns):
    arr = (L.SchemaColumn * max(1, len(schema)))()
    for c, d in zip(arr, schema):
        c.kind = {"string": L.SCHEMA_STRING, "int": L.SCHEMA_INT, "decimal": L.SCHEMA_DECIMAL,
                  "timestamp": L.SCHEMA_TIMESTAMP}[d["kind"]]
        c.column, c.nullable = columns.index(d["name"]), 1 if d.get("nullable", True) else 0
        if d.get("min") is not None:
            c.has_min, c.min_value = 1, d["min"]
        if d.get("max") is not None:
            c.has_max, c.max_value = 1, d["max"]
        c.precision, c.scale = d.get("precision", 0), d.get("scale", 0)
        text = d.get("mask") if d["kind"] == "timestamp" else d.get("matches")
        c.text = None if text is None else text.encode("utf-8")
    return arr


def host_check(schema, columns, rows):
    """dq_schema_check_host: (verdicts as True / False / None, per definition the cast values or None)."""
    from deequ_amd import _lib as L

    plan = ctypes.c_void_p()
    L.check(L.lib.dq_schema_plan_create(make_defs(L, schema, columns), len(schema), ctypes.byref(plan)))
    try:
        n, nc, nd = len(rows), len(columns), len(schema)
        keep, data, offs, valid = [], (ctypes.c_void_p * nc)(), (ctypes.c_void_p * nc)(), (ctypes.c_void_p * nc)()
        for i, c in enumerate(columns):
            vals = [r[c] for r in rows]
            d = np.frombuffer(b"".join(v or b"" for v in vals) + b"\0", dtype=np.uint8).copy()
            o = np.zeros(n + 1, dtype=np.int64)
            np.cumsum([len(v or b"") for v in vals], out=o[1:])
            ok = np.array([v is not None for v in vals] + [True], dtype=np.uint8)
            keep += [d, o, ok]
            data[i], offs[i], valid[i] = d.ctypes.data, o.ctypes.data, ok.ctypes.data
        verdict = np.zeros(n + 1, dtype=np.uint8)
        widths = {"int": 4, "decimal": 16, "timestamp": 8, "string": 1}
        cv = [np.zeros((n + 1) * widths[d["kind"]], dtype=np.uint8) for d in schema]
        cok = [np.zeros(n + 1, dtype=np.uint8) for _ in schema]
        pv, pk = (ctypes.c_void_p * max(1, nd))(), (ctypes.c_void_p * max(1, nd))()
        for i in range(nd):
            pv[i], pk[i] = cv[i].ctypes.data, cok[i].ctypes.data
        L.check(L.lib.dq_schema_check_host(plan, data, offs, valid, nc, n, verdict.ctypes.data, pv, pk))
    finally:
        L.lib.dq_schema_plan_destroy(plan)
    casts = []
    for d, v, k in zip(schema, cv, cok):
        w = widths[d["kind"]]
        out = []
        for r in range(n):
            if not k[r] or d["kind"] == "string":
                out.append(None)
            else:
                out.append(int.from_bytes(v[r * w:(r + 1) * w].tobytes(), "little", signed=True))
        casts.append(out)
    return [{0: False, 1: True, 2: None}[int(x)] for x in verdict[:n]], casts


RULES = {
    "int": (R.int_pool, [{"kind": "int", "name": "c"}, {"kind": "int", "name": "c", "min": -10, "max": 1000},
                         {"kind": "int", "name": "c", "nullable": False, "min": 124},
                         {"kind": "int", "name": "c", "max": -2147483648}]),
    "decimal": (R.decimal_pool, [{"kind": "decimal", "name": "c", "precision": p, "scale": s}
                                 for p, s in ((10, 2), (3, 3), (38, 0), (38, 38), (5, 0), (1, 0), (38, 19), (9, 2))]),
    "timestamp": (R.timestamp_pool, [{"kind": "timestamp", "name": "c", "mask": R.MAIN_MASK},
                                     {"kind": "timestamp", "name": "c", "mask": "yyyy-MM-dd", "nullable": False}]),
    "timestamp_quoted": (R.quoted_timestamp_pool, [{"kind": "timestamp", "name": "c", "mask": R.QUOTED_MASK}]),
    "string": (R.string_pool, [{"kind": "string", "name": "c", "min": 3, "max": 5},
                               {"kind": "string", "name": "c", "matches": R.NAME_REGEX},
                               {"kind": "string", "name": "c", "nullable": False, "min": 1, "matches": "[a-c]+"},
                               {"kind": "string", "name": "c", "max": 0}]),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_pool_is_not_vacuous(rule):
    """On the restatement alone: the rule's first schema accepts at least 10% and rejects at least 10% of its pool."""
    pool, schemas = RULES[rule]
    got = [R.cnf([schemas[0]], {"c": v}) for v in pool()]
    assert got.count(True) >= 0.1 * len(got) and got.count(False) >= 0.1 * len(got), (got.count(True), len(got))


def test_cnf_pool_has_all_three_outcomes():
    got = [R.cnf(R.mixed_schema(), r) for r in R.mixed_rows(4097)]
    assert min(got.count(True), got.count(False), got.count(None)) >= 20, (got.count(True), got.count(False), got.count(None))
    assert [R.cnf(R.mixed_schema(), r) for r in R.mixed_rows(63)].count(True) >= 6


def test_restatement_anchors():
    """The restatement against values written by hand."""
    assert R.to_int(b"-2147483648") == -(1 << 31) and R.to_int(b"2147483648") is None and R.to_int(b"1.") == 1
    assert R.to_int(b"1.x") is None and R.to_int(b".5") == 0 and R.to_int(b" 1") is None and R.to_int(b"+") is None
    assert R.to_decimal(b"1.234", 10, 2) == 123 and R.to_decimal(b"1.235", 10, 2) == 124
    assert R.to_decimal(b"-1.235", 10, 2) == -124 and R.to_decimal(b"99999999.995", 10, 2) is None
    assert R.to_decimal(b"0.995", 3, 3) == 995 and R.to_decimal(b"1", 3, 3) is None and R.to_decimal(b"0.9995", 3, 3) is None
    assert R.to_decimal(b"9" * 38, 38, 0) == 10 ** 38 - 1 and R.to_decimal(b"9" * 38 + b".5", 38, 0) is None
    assert R.to_decimal(b"0e999999999", 10, 2) == 0 and R.to_decimal(b"0e9999999999", 10, 2) is None
    assert R.to_decimal(b"1e09999999999", 10, 2) is None and R.to_decimal(b"1e00000000001", 10, 2) == 1000
    assert R.to_decimal(b"1e99999999999", 10, 2) is None
    assert R.to_decimal(b"1.", 10, 2) == 100 and R.to_decimal(b"+.5", 10, 2) == 50
    for bad in (b".", b"", b"+", b"1e", b"NaN", b"1d"):
        assert R.to_decimal(bad, 10, 2) is None, bad
    ts = lambda b, m=R.MAIN_MASK: (lambda r: None if r is None else r[1])(R.parse_timestamp(b, m))
    assert ts(b"2012-07-22 22:59:59") == 1342997999 * 10 ** 6  # 15543 days + 82799 s
    assert ts(b"2012-13-45 25:61:61") == ts(b"2013-02-15 02:02:01")  # lenient: every field rolls over
    assert ts(b"2012-07-22  22:59:59") == ts(b"2012-07-22 22:59:59") and ts(b"2012-07-22 \t22:59:59") is not None
    assert ts(b"+1-07-22 22:59:59") is None and ts(b"-1-07-22 22:59:59") is not None
    assert ts(b"12E1-07-22 22:59:59") == ts(b"0120-07-22 22:59:59") and ts(b"2012-07-22 22:59:59E") == ts(b"2012-07-22 22:59:59")
    assert ts(b"2012E-07-22 22:59:59") is None and ts(b"2012-07-22 22:59") is None and ts(b"2012/07/22 22:59:59") is None
    assert ts(b"2012-07-22 22:59:59 and more") == ts(b"2012-07-22 22:59:59")
    assert ts(b"2012.07.22 at 22h59'59", R.QUOTED_MASK) == ts(b"2012-07-22 22:59:59")
    assert R.timestamp_pinned(b"1582-10-15 00:00:00", R.MAIN_MASK) and not R.timestamp_pinned(b"1582-10-14 00:00:00", R.MAIN_MASK)
    assert not R.timestamp_pinned(b"1234567890-07-22 22:59:59", R.MAIN_MASK)
    assert R.char_count("日本語".encode()) == 3 and not R.matches(b"", ".*") and R.matches(b"hello world", R.NAME_REGEX)
    q = {"kind": "int", "name": "c", "min": 0}
    assert R.cnf([q], {"c": None}) is None and R.cnf([dict(q, nullable=False)], {"c": None}) is False
    assert R.cnf([{"kind": "int", "name": "c", "max": 0}], {"c": None}) is True


@pytest.mark.parametrize("rule", sorted(RULES))
def test_host_rules_equal_restatement(rule):
    pool, schemas = RULES[rule]
    values = pool() + [None]
    rows = [{"c": v} for v in values]
    for d in schemas:
        verdicts, casts = host_check([d], ["c"], rows)
        for v, got, cast in zip(values, verdicts, casts[0]):
            assert got is R.cnf([d], {"c": v}), (d, v, got)
            if d["kind"] != "string":
                assert cast == R.cast_value(d, v), (d, v, cast)


def test_host_cnf_equals_restatement():
    """The mixed schema (one definition per kind, a pass-through column) over rows of all three outcomes, plus the
    definition order reversed and a column named twice."""
    rows = R.mixed_rows(1500)
    for schema in (R.mixed_schema(), R.mixed_schema()[::-1],
                   R.mixed_schema() + [{"kind": "string", "name": "id", "nullable": True, "max": 3}]):
        verdicts, _ = host_check(schema, R.MIXED_COLUMNS, rows)
        assert verdicts == [R.cnf(schema, r) for r in rows]
    assert host_check([], ["c"], [{"c": None}, {"c": b"x"}])[0] == [True, True]  # foldLeft's seed: TRUE


BAD_MASKS = ["yy-MM-dd", "yyyyMMdd", "yyyy-MMM-dd", "yyyy-MM-dd a", "yyyy-MM-dd HH:mm:ss.SSS", "yyyy-MM-dd'T", "2012",
             "---", "", "yyyy-MM-dd hh:mm", "yyyy-MM-dd HH:mm:ss z", "yyyy-MM-dd G", "yyyy1MM", "yyyyéMM", "EEE, yyyy"]
GOOD_MASKS = [R.MAIN_MASK, R.QUOTED_MASK, "yyyy", "d/M/yyyy", "yyyyy.MM", "'on' yyyy-MM-dd", "HH:mm", "yyyy''MM"]


def test_refusals_come_from_plan_create():
    from deequ_amd import _lib as L

    def create(d):
        plan = ctypes.c_void_p()
        st = L.lib.dq_schema_plan_create(make_defs(L, [d], ["c"]), 1, ctypes.byref(plan))
        if st == L.DQ_OK:
            L.lib.dq_schema_plan_destroy(plan)
        return st

    for m in BAD_MASKS:
        assert R.compile_mask(m) is None, m
        assert create({"kind": "timestamp", "name": "c", "mask": m}) == L.DQ_E_UNSUPPORTED, m
        assert L.lib.dq_last_error(), m
    for m in GOOD_MASKS:
        assert R.compile_mask(m) is not None, m
        assert create({"kind": "timestamp", "name": "c", "mask": m}) == L.DQ_OK, m
    for p in (r"(a)\1", r"(?=a)b", r"\bword", "a*"):  # outside the DFA subset / can match the empty string
        assert create({"kind": "string", "name": "c", "matches": p}) == L.DQ_E_UNSUPPORTED, p
    assert create({"kind": "decimal", "name": "c", "precision": 39, "scale": 0}) == L.DQ_E_INVALID
    assert create({"kind": "decimal", "name": "c", "precision": 5, "scale": 6}) == L.DQ_E_INVALID


def test_rules_under_sanitizers(tmp_path):
    """deequ_amd/csrc/dq_schema.h in a stand-alone program built with ASan + UBSan (no recovery), over the
    adversarial lists -- whose answers must again equal the restatement -- and over random byte strings."""
    exe = tmp_path / "schema_rules_check"
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "deequ_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "schema_rules_check.cpp")], check=True)
    hx = lambda b: b.hex() or "-"
    reqs, want = [], []
    for b in R.int_pool():
        reqs.append(f"I {hx(b)}")
        v = R.to_int(b)
        want.append("N" if v is None else f"V {v}")
    for b in R.decimal_pool():
        for p, s in ((10, 2), (3, 3), (38, 0), (38, 38)):
            reqs.append(f"D {p} {s} {hx(b)}")
            v = R.to_decimal(b, p, s)
            want.append("N" if v is None else "V %016x %016x" % ((v >> 64) & (2 ** 64 - 1), v & (2 ** 64 - 1)))
    for mask, pool in ((R.MAIN_MASK, R.timestamp_pool()), (R.QUOTED_MASK, R.quoted_timestamp_pool())):
        for b in pool:
            reqs.append(f"T {mask.encode().hex()} {hx(b)}")
            r = R.parse_timestamp(b, mask)
            want.append("N" if r is None else f"V {r[1]}")
    for m in BAD_MASKS:
        if m:
            reqs.append(f"T {m.encode().hex()} -")
            want.append("U")
    for b in R.string_pool():
        reqs.append(f"C {hx(b)}")
        want.append(f"V {R.char_count(b)}")
    reqs.append("R 5 20000")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], input="\n".join(reqs) + "\n", capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(reqs) and lines[-1].startswith("R ")
    for q, w, g in zip(reqs, want, lines):
        assert g == w, (q, w, g)
