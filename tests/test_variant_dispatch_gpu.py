"""Every column-pass variant through the generated dispatch (dq_kernels.hip launch_column_scan over the rows of
dq_device.h kVariants): for each of the 32 variants the smallest plan that selects it -- one nullable column
(~10 % NULLs) of the variant's kind, the analyzers its name spells, a `where` on a second column (all but the
validity variant) -- scans chunks of 1 and 2049 rows (one full 2048-row workgroup iteration plus a one-row tail: the
full-block and the clipped path).

Asserted: every metric equals the oracle's (counts, min / max, DataType counts and HLL words exact; fp64 sums and
moments 1e-12 relative, as tests/test_types_gpu.py and tests/test_decimal_gpu.py compare them), and the plan's
timers show 2 launches of variant v (timer 16 + v) and none of any other variant: the dispatch reached the
instantiation the table names.  The four string-HLL variants run again with DQ_STR_PATH=long (read at plan
creation), so their LONG instantiations are launched too.  The strings include lengths 0, 23, 24, 28, 29 and 120:
the fast path, the deferred queue and the rare path.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from deequ_amd._lib import VARIANT_NAMES
from oracle import dq_oracle as O

pytestmark = pytest.mark.gpu

CHUNKS = (1, 2049)
N = sum(CHUNKS)
WHERE = "w > 0"
# the column type a variant's name starts with (validity reads no values: any column)
KIND_DTYPE = {"validity": "i32", "large_utf8": "large_utf8", "utf8": "utf8", "f64": "f64", "f32": "f32", "i64": "i64",
              "i32": "i32", "i16": "i16", "i8": "i8", "bool": "bool", "d128": "decimal(28,10)"}
STR_HLL = [v for v, nm in VARIANT_NAMES.items() if "utf8" in nm and "hll" in nm]


@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import deequ_amd

    return deequ_amd


def _case(v):
    """(column dtype, analyzer names, `where`) of the smallest plan that selects variant v, from its name.  (A
    Completeness under a `where` is two predicate counters, not a column task: the validity variant runs bare.)"""
    name = VARIANT_NAMES[v]
    kind = next(k for k in KIND_DTYPE if name.startswith(k))  # ("large_utf8" / "utf8": in that order)
    rest = name[len(kind):]
    ops = []
    if "_stats" in rest:
        ops += ["Mean", "StandardDeviation", "Minimum", "Maximum", "Sum"]
    if "_hll" in rest or kind == "bool":
        ops += ["ApproxCountDistinct"]
    if "_dtype" in rest:
        ops += ["DataType"]
    return (KIND_DTYPE[kind], ops, WHERE) if ops else (KIND_DTYPE[kind], ["Completeness"], None)


@functools.lru_cache(maxsize=None)
def _host(dtype):
    """{x: the column under test, w: the `where` column} for the oracle; row 0 (the one-row chunk) is selected."""
    from tests.test_decimal_gpu import dec_values
    from tests.test_types_gpu import _values

    rng = np.random.default_rng(len(dtype) * 1000 + sum(map(ord, dtype)))
    if "utf8" in dtype:
        lens = rng.integers(0, 41, N)
        lens[::2] = np.resize(np.array([0, 23, 24, 28, 29, 120, 7, 16, 25, 63]), len(lens[::2]))
        pool = [b"12", b"-7", b"3.5", b"true", b"false", b"x", b"1e5", b""]  # every DataType class
        vals = []
        for i in range(N):
            if i % 7 == 3:
                vals.append(pool[i % len(pool)])
            else:
                vals.append(rng.integers(0, 256, int(lens[i]), dtype=np.uint8).tobytes())
    elif O.decimal_ps(dtype):
        vals = dec_values(*O.decimal_ps(dtype), N, rng)
    else:
        vals = _values(dtype, N, rng)
        if dtype in ("f64", "f32"):  # signed zeros and the bounds of DataType's plain-decimal range (all finite:
            vals[rng.integers(0, N, 40)] = rng.choice(np.array([-0.0, 0.0, 1e-3, 1e7]), 40)  # the moments stay numbers)
    valid = rng.random(N) >= 0.1
    w = rng.integers(-3, 10, N).astype(np.int32)
    wvalid = rng.random(N) >= 0.05
    valid[0] = wvalid[0] = True
    w[0] = 1
    if "utf8" in dtype:
        vals = [x if ok else None for x, ok in zip(vals, valid)]
    odtype = "utf8" if dtype == "large_utf8" else dtype  # (the oracle knows one string type: the offsets' width is layout)
    return {"x": O.OColumn(odtype, vals, valid), "w": O.OColumn("i32", w, wvalid)}


@functools.lru_cache(maxsize=None)
def _reference(dtype, op, where):
    return O.compute_state((op, "x", where), _host(dtype), N)


def _chunk(dq, dtype, lo, hi):
    from deequ_amd.table import column_from_numpy, utf8_column

    h = _host(dtype)
    if "utf8" in dtype:
        x = utf8_column("x", h["x"].values[lo:hi], large=(dtype == "large_utf8"))
    else:
        x = column_from_numpy("x", dtype, h["x"].values[lo:hi], h["x"].valid[lo:hi])
    return dq.Table([x, column_from_numpy("w", "i32", h["w"].values[lo:hi], h["w"].valid[lo:hi])])


def _scale(c):
    """sum(|x|) over the valid finite values: the condition number of a floating-point sum (Sum / Mean: 1e-12 of it)"""
    if O.decimal_ps(c.dtype):
        return float(sum(abs(x) for x in O._as_double_list(c))) + 1.0
    if c.dtype not in ("f32", "f64"):
        return 1.0
    x = np.asarray(c.values, dtype=np.float64)[c.valid]
    return float(np.abs(x[np.isfinite(x)]).sum()) + 1.0


def _run(dq, v):
    from deequ_amd.runner import ScanPlan
    from tests.test_gpu_parity import assert_state_close

    dtype, ops, where = _case(v)
    analyzers = [getattr(dq, op)("x", where=where) for op in ops]
    tables = [_chunk(dq, dtype, 0, CHUNKS[0]), _chunk(dq, dtype, CHUNKS[0], N)]
    plan = ScanPlan(analyzers, tables[0].schema, pred_pass="interpreter")
    try:
        plan.enable_timing(True)
        for t in tables:
            plan.scan(t)
        results = plan.finish()
        launches = {u: plan.kernel_time(16 + u)[1] for u in VARIANT_NAMES}
    finally:
        plan.close()
    assert launches == {u: (len(CHUNKS) if u == v else 0) for u in VARIANT_NAMES}, (VARIANT_NAMES[v], launches)
    for a, op, r in zip(analyzers, ops, results):
        assert_state_close(a._from_result(r), _reference(dtype, op, where), scale=_scale(_host(dtype)["x"])), (v, op)


@pytest.mark.parametrize("v", sorted(VARIANT_NAMES), ids=lambda v: VARIANT_NAMES[v])
def test_variant_dispatch(dq, v, monkeypatch):
    monkeypatch.delenv("DQ_STR_PATH", raising=False)
    _run(dq, v)


@pytest.mark.parametrize("v", STR_HLL, ids=lambda v: VARIANT_NAMES[v] + "-long")
def test_variant_dispatch_long_strings(dq, v, monkeypatch):
    """The LONG instantiation of a string-HLL variant (dq_plan_create reads DQ_STR_PATH)."""
    monkeypatch.setenv("DQ_STR_PATH", "long")
    _run(dq, v)
