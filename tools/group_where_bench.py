#!/usr/bin/env python3
"""Time the filtered frequency build and the filtered quantile select against what users had before them.

    python tools/group_where_bench.py [--rows 50000000] [--reps 7] [--groups 1048576] [--selectivities 1.0,0.5,0.01]

One JSON line per (column, selectivity, route).  Columns: one i64 column (an unhashed table) and one utf8 column of
8..16 bytes (a hashed table), --groups distinct values each, 2 % NULL.  The selection is a random bitmap with each
row's bit set with the given probability (at 1.0: all ones).  Routes, per case:

    (a) build          dq_freq_build of the whole column, no selection
    (b) build_where    dq_freq_build_where with the selection
    (c) take+build     schema.take_rows of the column through the selection, then dq_freq_build of the copy

and the same three for dq_approx_quantiles (quantiles 0.25 / 0.5 / 0.75 of the i64 column).  (c) is the route a user
had before the _where entry points.  The bitmap itself is made once, outside every timed region: all three routes of
a real run share the predicate's evaluation.

The time is the whole call with its synchronisation: one warm-up call, then --reps timed ones; ms is the best,
ms_median the median and spread (max - min) / median of the timed calls.  Data is generated on the device from a seed.
No threshold is set here.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.grouping import _gpu_type
    from deequ_amd.schema import take_rows
    from deequ_amd.table import Column, Table

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--selectivities", default="1.0,0.5,0.01")
    args = ap.parse_args()
    n = args.rows
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    dev = torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")

    def padded(t, extra=16):
        raw = t.contiguous().view(torch.uint8).reshape(-1)
        return torch.cat([raw, torch.zeros((-len(raw)) % 16 + extra, dtype=torch.uint8, device="cuda")])

    def bitmap(p):
        """(bytes of whole 64-bit words + one zero word, set bits) with each row's bit set with probability p."""
        keep = torch.ones(n, dtype=torch.bool, device="cuda") if p >= 1.0 else \
            torch.rand(n, generator=gen, device="cuda") < p
        bits = torch.cat([keep, torch.zeros((-n) % 64 + 64, dtype=torch.bool, device="cuda")]).view(-1, 8)
        return (bits.to(torch.uint8) * weights).sum(dim=1, dtype=torch.uint8), int(keep.sum().item())

    def i64_column(ids):
        return Column("k", "i64", n, padded(ids * 7919), bitmap(0.98)[0], None, nullable=True)

    def utf8_column(ids):
        lens = 8 + ids % 9
        offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lens, 0, out=offs[1:])
        total = int(offs[-1].item())
        h = ids * 0x2545F4914F6CDD1D + 0x632BE59BD9B4E019
        data = torch.empty(total, dtype=torch.uint8, device="cuda")
        pos = offs[:-1]
        for j in range(16):
            sel = lens > j
            data[pos[sel] + j] = (97 + ((h[sel] >> (4 * j)) & 15) + ((ids[sel] >> (2 * j)) & 7)).to(torch.uint8)
        return Column("s", "utf8", n, padded(data), bitmap(0.98)[0], padded(offs.to(torch.int32)), nullable=True,
                      data_bytes=total)

    def timed(fn):
        times = []
        for _ in range(args.reps + 1):  # (the first call warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        t = times[1:]
        return min(t), statistics.median(t), (max(t) - min(t)) / statistics.median(t)

    def line(what, column, p, selected, timing):
        best, med, spread = timing
        print(json.dumps(dict(what=what, column=column, selectivity=p, rows=n, selected=selected,
                              ms=round(best * 1e3, 3), ms_median=round(med * 1e3, 3), spread=round(spread, 3))),
              flush=True)

    def build(col, rows, sel=None):
        types = (ctypes.c_int32 * 1)(_gpu_type(col.dtype))
        views = (L.ColumnView * 1)(col.view())
        nrows = (ctypes.c_int64 * 1)(rows)
        h = ctypes.c_void_p()
        if sel is None:
            L.check(L.lib.dq_freq_build(types, 1, views, nrows, 1, dev, stream, ctypes.byref(h)))
        else:
            ptrs = (ctypes.c_void_p * 1)(sel.data_ptr())
            L.check(L.lib.dq_freq_build_where(types, 1, views, nrows, ptrs, 1, dev, stream, ctypes.byref(h)))
        groups = L.lib.dq_freq_num_groups(h)
        L.lib.dq_freq_destroy(h)
        return groups

    qs = (ctypes.c_double * 3)(0.25, 0.5, 0.75)

    def quantiles(col, rows, sel=None):
        views = (L.ColumnView * 1)(col.view())
        nrows = (ctypes.c_int64 * 1)(rows)
        out, cnt = (ctypes.c_double * 3)(), ctypes.c_int64()
        if sel is None:
            L.check(L.lib.dq_approx_quantiles(_gpu_type(col.dtype), views, nrows, 1, qs, 3, 0.0, dev, stream, out,
                                              ctypes.byref(cnt)))
        else:
            ptrs = (ctypes.c_void_p * 1)(sel.data_ptr())
            L.check(L.lib.dq_approx_quantiles_where(_gpu_type(col.dtype), views, nrows, ptrs, 1, qs, 3, 0.0, dev, stream,
                                                    out, ctypes.byref(cnt)))
        return list(out)

    def copy_then(fn, col, sel, selected):
        taken = take_rows(Table([col]), sel, selected)
        return fn(taken.columns[col.name], selected)

    ids = torch.randint(0, args.groups, (n,), generator=gen, device="cuda")
    columns = [("i64", i64_column(ids)), ("utf8", utf8_column(ids))]
    del ids
    for p in [float(x) for x in args.selectivities.split(",") if x]:
        sel, selected = bitmap(p)
        for name, col in columns:
            line("build", name, p, n, timed(lambda: build(col, n)))
            line("build_where", name, p, selected, timed(lambda: build(col, n, sel)))
            line("take+build", name, p, selected, timed(lambda: copy_then(build, col, sel, selected)))
        col = columns[0][1]
        line("quantiles", "i64", p, n, timed(lambda: quantiles(col, n)))
        line("quantiles_where", "i64", p, selected, timed(lambda: quantiles(col, n, sel)))
        line("take+quantiles", "i64", p, selected, timed(lambda: copy_then(quantiles, col, sel, selected)))


if __name__ == "__main__":
    main()
