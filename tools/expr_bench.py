#!/usr/bin/env python3
"""Time dq_expr_eval (the derived column of an arithmetic operand of a predicate) alone.

    python tools/expr_bench.py [--rows 64000000] [--reps 7]

One JSON line per expression: the best and the median wall time of one call (launch, the program image's upload, the
NULL counter's read-back and the stream synchronisation included, as tools/strlen_bench.py times dq_utf8_length) and
the bytes moved per second as a fraction of the HBM peak.  The pass is streaming: per row it reads the inputs' widths
plus their validity bits and writes the result's width plus one bit.  The yardstick, alternating with the calls, is a
device-to-device copy of the same number of bytes.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
BLOCK = 1 << 20        # rows generated; a column is this block repeated

SCHEMA = [("a", "i32", True), ("b", "i32", True), ("c", "i64", True), ("d", "f64", True), ("f", "f32", True),
          ("g", "f32", True), ("y", "i8", True)]
CASES = [  # (name, predicate whose one operand is the expression)
    ("i32 % literal", "a % 2 = 0"),
    ("i32 + i32", "a + b > 0"),
    ("i32 * i32 + i64", "a * b + c > 0"),
    ("i32 / i32", "a / b > 0.5"),
    ("f32 * f32 + f32", "f * g + f > 0"),
    ("f64 * f64 - f64 / f64", "d * d - d / d > 0"),
    ("i64 % i32", "c % b = 0"),
    ("f64 % f64", "d % d > 0"),
    ("i8 + 1", "y + 1 > 0"),
    ("four columns, nine instructions", "(a + b) * c - d / 2 > 0"),
]


def main() -> None:
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.analyzers import PlanBuilder
    from deequ_amd.expressions import _SIZE
    from deequ_amd.table import column_from_numpy

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    n = args.rows
    reps = (n + BLOCK - 1) // BLOCK
    rng = np.random.default_rng(3)
    np_of = {"i8": np.int8, "i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
    cols = {}
    for name, dt, _ in SCHEMA:
        block = (rng.standard_normal(BLOCK) * 100).astype(np_of[dt]) if dt[0] == "f" else \
            rng.integers(-100, 100, BLOCK).astype(np_of[dt])
        valid = rng.random(BLOCK) >= 0.05
        cols[name] = column_from_numpy(name, dt, np.tile(block, reps)[:n], np.tile(valid, reps)[:n])
    words = (n + 63) // 64
    out = torch.empty(8 * n + 16, dtype=torch.uint8, device="cuda")
    validity = torch.empty((words + 1) * 8, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    device = torch.cuda.current_device()

    def timed(calls):
        """best and median seconds of each call of `calls`, run alternately args.reps times after one warm-up each"""
        times = [[] for _ in calls]
        for rep in range(args.reps + 1):
            for k, call in enumerate(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        return [(min(t), statistics.median(t)) for t in times]

    for name, text in CASES:
        b = PlanBuilder(SCHEMA, collect_exprs=True)
        b.pool.add(text)
        (e,) = b.exprs.values()
        src = [cols[c] for c in e.columns]
        views = (L.ColumnView * len(src))(*[c.view() for c in src])
        nulls = ctypes.c_int64(0)
        moved = sum(_SIZE[c.dtype] * n + n // 8 for c in src) + _SIZE[e.dtype] * n + n // 8
        half = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        other = torch.empty_like(half)

        def call():
            L.check(L.lib.dq_expr_eval(ctypes.byref(e.program), views, n, out.data_ptr(), validity.data_ptr(), device,
                                       stream, ctypes.byref(nulls)))

        (best, median), (cbest, _) = timed([call, lambda: other.copy_(half)])
        print(json.dumps({"input": name, "expression": e.text, "kernel": "dq_expr_eval", "rows": n,
                          "instructions": e.program.n_instrs, "result": e.dtype, "nulls": nulls.value,
                          "ms_best": round(best * 1e3, 3), "ms_median": round(median * 1e3, 3),
                          "bytes_per_row": round(moved / n, 3), "GBs_best": round(moved / best / 1e9, 1),
                          "fraction_of_hbm_peak": round(moved / best / 1e9 / HBM_PEAK_GBS, 3),
                          "copy_same_bytes_ms_best": round(cbest * 1e3, 3),
                          "copy_fraction_of_hbm_peak": round(moved / cbest / 1e9 / HBM_PEAK_GBS, 3)}), flush=True)
        del half, other


if __name__ == "__main__":
    main()
