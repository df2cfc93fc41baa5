#!/usr/bin/env python3
"""Time the two row-level kernels: dq_row_outcomes (predicate outcomes per row) and dq_freq_unique_rows.

    python tools/rowlevel_bench.py [--rows 50000000] [--reps 7]

One JSON line per case.  dq_row_outcomes: 1, 8 and 32 numeric outputs over four f64 columns and one regex output over
a string column; the time is the whole call (launch, the counts' read-back, the stream synchronisation) into bitmaps
allocated once.  Bytes are the algorithmic ones: the column bytes read (values, validity, offsets, string bytes, each
once) plus rows / 8 per bitmap written; hbm_frac = bytes / time / 8 TB/s.  For comparison each numeric case also runs
the same predicates as Compliance analyzers through the fused scan's interpreted predicate pass (dq_pred_scan, the
counting form) and reports its kernel time from the plan's device events.  dq_freq_unique_rows: an i64 key and a
string key, the table built beforehand; bytes are the key column plus the bitmap.  No threshold is set here.
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

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak


def main() -> None:
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.analyzers import Compliance
    from deequ_amd.grouping import _gpu_type, build_frequencies
    from deequ_amd.rowlevel import RowForm, RowProgram
    from deequ_amd.runner import ScanPlan
    from deequ_amd.table import Table, column_from_numpy
    from tools.schema_bench import string_column

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    n, rng = args.rows, np.random.default_rng(1)
    words = (n + 63) // 64
    cols = [column_from_numpy(f"x{i}", "f64", rng.normal(size=n), rng.random(n) >= 0.05) for i in range(4)]
    pieces = rng.integers(0, 10 ** 6, n).astype("S")
    pieces[rng.random(n) < 0.3] = b"abc"
    strs = string_column("s", pieces, rng.random(n) >= 0.03)
    keys = column_from_numpy("k", "i64", rng.integers(0, n // 2, n), rng.random(n) >= 0.02)
    table = Table(cols + [strs, keys])
    dev = torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        times = []
        for _ in range(args.reps + 1):  # (the first call warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times[1:]), statistics.median(times[1:])

    def line(what, best, med, nbytes, **extra):
        print(json.dumps(dict(what=what, rows=n, ms=round(best * 1e3, 3), ms_median=round(med * 1e3, 3),
                              rows_per_s=round(n / best), algorithmic_GB=round(nbytes / 1e9, 3),
                              hbm_frac=round(nbytes / best / 1e9 / HBM_PEAK_GBS, 4), **extra)), flush=True)

    def outcomes(what, forms, read_bytes, counting=None):
        prog = RowProgram(forms, table.schema)
        k = len(forms)
        bufs = [torch.zeros((words + 1) * 8, dtype=torch.uint8, device="cuda") for _ in range(k)]
        pp = (ctypes.c_void_p * k)(*[b.data_ptr() for b in bufs])
        npass = (ctypes.c_int64 * k)()
        views = (L.ColumnView * len(prog.columns))(*[table.columns[c].view() for c in prog.columns])
        best, med = timed(lambda: L.check(L.lib.dq_row_outcomes(prog.handle, views, n, pp, None, dev, stream, npass, None)))
        extra = dict(outputs=k, num_pass_0=int(npass[0]))
        if counting:  # the same predicates counted by dq_pred_scan (interpreter), kernel time from device events
            plan = ScanPlan([Compliance(f"p{i}", t) for i, t in enumerate(counting)], table.schema, pred_pass="interpreter")
            plan.enable_timing(True)
            plan.scan(table)
            plan.finish()
            plan.reset()
            plan.enable_timing(True)
            for _ in range(args.reps):
                plan.scan(table)
                plan.finish()
                plan.reset()
            ms, launches = plan.kernel_time(0)
            plan.close()
            extra["counting_pred_scan_ms"] = round(ms / max(1, launches), 3)
        line(what, best, med, read_bytes + k * n / 8, **extra)
        prog.close()

    col_bytes = 8 * n + n / 8
    for k, ncols in ((1, 1), (8, 4), (32, 4)):
        texts = [f"x{i % ncols} >= {i / 100}" for i in range(k)]
        outcomes(f"dq_row_outcomes f64 x{k}", [RowForm(f"p{i}", "predicate", ("sql", t)) for i, t in enumerate(texts)],
                 ncols * col_bytes, counting=texts)
    outcomes("dq_row_outcomes regex x1", [RowForm("r", "predicate", ("regex", "s", r"[a-c]+"))],
             4 * (n + 1) + strs.data_bytes + n / 8)

    for name, col in (("i64", keys), ("utf8", strs)):
        state = build_frequencies(table, [col.name])
        bitmap = torch.zeros((words + 1) * 8, dtype=torch.uint8, device="cuda")
        types = (ctypes.c_int32 * 1)(_gpu_type(col.dtype))
        views = (L.ColumnView * 1)(col.view())
        nu = ctypes.c_int64()
        best, med = timed(lambda: L.check(L.lib.dq_freq_unique_rows(state.frequencies.handle, types, views, n, bitmap.data_ptr(),
                                                                     None, stream, ctypes.byref(nu), None)))
        read = col_bytes if name == "i64" else 4 * (n + 1) + col.data_bytes + n / 8
        line(f"dq_freq_unique_rows {name}", best, med, read + n / 8, unique=nu.value,
             groups=int(L.lib.dq_freq_num_groups(state.frequencies.handle)))


if __name__ == "__main__":
    main()
