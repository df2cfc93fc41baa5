"""The column-pass variant table (deequ_amd/csrc/dq_device.h kVariants) and the planner's choice of variant.

CPU only.  The table, printed by a host build of the header (tests/variant_check.cpp), names variants 0..31 exactly
as deequ_amd._lib.VARIANT_NAMES does (timer 16 + v of dq_plan_kernel_time, bench.py's kernel names, profiles/).
The planner pin: for every column type and every combination of needs (none / stats / HLL / stats + HLL /
DataType / HLL + DataType) the `column pass: variant N` lines of dq_plan_explain equal
tests/golden/plan_variants.json, recorded from the build before the planner chose variants through the table; so do
the plans whose tasks leave the column pass (a Correlation group's fused moments, the compiled predicate pass's
fused HLL tasks)."""
from __future__ import annotations

import json
import os
import subprocess

import deequ_amd as dq
from deequ_amd import _lib as L
from deequ_amd.runner import explain
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_variants.json")
DTYPES = ["f64", "f32", "i64", "i32", "i16", "i8", "date32", "timestamp", "bool", "utf8", "large_utf8",
          "decimal(10,2)", "decimal(38,6)"]
NEEDS = {
    "none": lambda c: [dq.Completeness(c)],
    "stats": lambda c: [dq.Mean(c)],
    "hll": lambda c: [dq.ApproxCountDistinct(c)],
    "stats+hll": lambda c: [dq.Mean(c), dq.ApproxCountDistinct(c)],
    "dtype": lambda c: [dq.DataType(c)],
    "hll+dtype": lambda c: [dq.ApproxCountDistinct(c), dq.DataType(c)],
}


def _lines(analyzers, schema, keep=("column pass:",)):
    """The explain text's lines that start with one of `keep`, or the planner's refusal."""
    try:
        text = explain(analyzers, schema)
    except L.DQError as e:
        return [f"refused ({e.status}): {e.message}"]
    return [ln for ln in text.splitlines() if ln.startswith(keep)]


def plan_cases():
    """case name -> explain lines, from the library deequ_amd loaded."""
    out = {}
    for t in DTYPES:
        for need, make in NEEDS.items():
            out[f"{t} {need}"] = _lines(make("x"), [("x", t, True)])
    # a Correlation group takes its columns' stats-only tasks of the same `where` out of the column pass (numeric
    # kinds only: the decimal's stays), not a stats + HLL task, not one under another `where`
    schema = [("x", "f64", True), ("y", "i16", True), ("d", "decimal(10,2)", True), ("w", "i32", True)]
    keep = ("column pass:", "pair pass:")
    w = "w > 0"
    out["pair fusion"] = _lines([dq.Correlation("x", "y", where=w), dq.Mean("x", where=w), dq.Mean("y", where=w)],
                                schema, keep)
    out["pair fusion, other tasks stay"] = _lines(
        [dq.Correlation("x", "y", where=w), dq.Correlation("x", "d", where=w), dq.Mean("x", where=w),
         dq.ApproxCountDistinct("y", where=w), dq.Mean("y", where=w), dq.Mean("d", where=w), dq.Mean("w", where=w),
         dq.Mean("x")], schema, keep)
    # the compiled predicate pass hashes the HLL-only tasks (no `where`) of its f64 / i64 / i32 columns
    schema = [("a", "f64", True), ("b", "i64", True), ("c", "i32", True), ("e", "f32", True)]
    comp = [dq.Compliance("p", "a > 0 AND b > 0 AND c > 0 AND e > 0")]
    keep = ("column pass:", "predicate pass:")
    out["jit fusion"] = _lines(comp + [dq.ApproxCountDistinct(c) for c in "abce"], schema, keep)
    out["jit fusion, other tasks stay"] = _lines(
        comp + [dq.ApproxCountDistinct("a", where="b > 1"), dq.ApproxCountDistinct("b"), dq.Mean("b"),
                dq.ApproxCountDistinct("c")], schema, keep)
    return out


def test_table_names_match_python(tmp_path):
    exe = tmp_path / "variant_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "variant_check.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    rows = [ln.split() for ln in out if not ln.startswith("find")]
    assert [int(r[0]) for r in rows] == list(range(32))
    assert {int(r[0]): r[5] for r in rows} == L.VARIANT_NAMES
    assert list(L.VARIANT_NAMES) == list(range(32))
    # no two variants share a description; a description no variant has is -1
    assert len({tuple(r[1:5]) for r in rows}) == 32
    finds = [ln.split()[1:] for ln in out if ln.startswith("find")]
    assert finds == [[str(v), str(v)] for v in range(32)] + [["none", "-1"]]
    # the fields against the names (kind codes: dq_device.h ColKind)
    kinds = {"validity": 0, "f64": 1, "i64": 2, "i32": 3, "utf8": 4, "large_utf8": 5, "f32": 6, "i16": 7, "i8": 8,
             "bool": 9, "d128": 10}
    for v, kind, stats, hll, dtype, name in rows:
        prefix = next(k for k in sorted(kinds, key=len, reverse=True) if name.startswith(k))
        assert int(kind) == kinds[prefix], name
        rest = name[len(prefix):]
        assert (stats, dtype) == (str(int("_stats" in rest)), str(int("_dtype" in rest))), name
        assert hll == str(int("_hll" in rest or name == "bool")), name


def test_planner_variants_match_golden():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert "parent commit" in golden["recorded_from"]
    got = plan_cases()
    assert sorted(got) == sorted(golden["cases"])
    for name, lines in got.items():
        assert lines == golden["cases"][name], name
