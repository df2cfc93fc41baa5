#!/usr/bin/env python3
"""Time dq_freq_contains_rows (referential integrity: the rows whose key is in another table's key set).

    python tools/refint_bench.py [--rows 100000000] [--reps 7] [--groups 1024,65536,1048576,16777216]

One JSON line per case.  Cases: a single i64 key column (an unhashed table) against key sets of G = 2^10, 2^16, 2^20
and 2^24 keys; a utf8 key of 8..16 bytes and an (i64, utf8) pair (hashed tables, compared by value) at G = 2^20.  The
primary has --rows rows, about 90 % of which hit (ids drawn from [0, G / 0.9)) and 2 % of which are NULL.  Beside each
unhashed line, dq_freq_unique_rows over a table of the same G and rows, built -- as that entry requires -- from its
own primary column: the existing kernel with the plain binary search, the baseline of the splitter search.

The time is the whole call (the splitter gather, the probe kernel, the counts' read-back, the stream synchronisation)
into bitmaps allocated once: one warm-up call, then --reps timed ones; ms is the best, ms_median the median and
spread (max - min) / median of the timed calls.  bytes_per_row is the model: key bytes + validity bit + 1/8 byte out,
plus the table's share (its keys, and for a hashed table its stored values, over the rows).  Data is generated on the
device from a seed.  No threshold is set here.
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

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak
STRIDE = 7919          # key = id * STRIDE: gaps between neighbouring keys


def main() -> None:
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.grouping import _gpu_type, build_frequencies
    from deequ_amd.matching import KeySet
    from deequ_amd.table import Column, Table

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--groups", default="1024,65536,1048576,16777216")
    ap.add_argument("--hashed-groups", type=int, default=1 << 20)
    args = ap.parse_args()
    n = args.rows
    words = (n + 63) // 64
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def padded(t, extra=16):
        raw = t.contiguous().view(torch.uint8).reshape(-1)
        return torch.cat([raw, torch.zeros((-len(raw)) % 16 + extra, dtype=torch.uint8, device="cuda")])

    def validity(m, null_rate):
        valid = torch.rand(m, generator=gen, device="cuda") >= null_rate
        bits = torch.cat([valid, torch.zeros((-m) % 64 + 64, dtype=torch.bool, device="cuda")]).view(-1, 8)
        weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")
        return (bits.to(torch.uint8) * weights).sum(dim=1, dtype=torch.uint8)

    def i64_column(name, ids, null_rate):
        return Column(name, "i64", len(ids), padded(ids * STRIDE), validity(len(ids), null_rate) if null_rate else None,
                      None, nullable=bool(null_rate))

    def utf8_column(name, ids, null_rate):
        """8..16 lower-case letters per id, a function of the id alone."""
        m = len(ids)
        lens = 8 + ids % 9
        offs = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lens, 0, out=offs[1:])
        total = int(offs[-1].item())
        h = ids * 0x2545F4914F6CDD1D + 0x632BE59BD9B4E019
        data = torch.empty(total, dtype=torch.uint8, device="cuda")
        pos = offs[:-1]
        for j in range(16):  # letter j of every string long enough to have one
            sel = lens > j
            data[pos[sel] + j] = (97 + ((h[sel] >> (4 * j)) & 15) + ((ids[sel] >> (2 * j)) & 7)).to(torch.uint8)
        return Column(name, "utf8", m, padded(data), validity(m, null_rate) if null_rate else None,
                      padded(offs.to(torch.int32)), nullable=bool(null_rate), data_bytes=total)

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

    def line(what, G, timing, row_bytes, table_bytes, **extra):
        best, med, spread = timing
        per_row = row_bytes / n + table_bytes / n
        print(json.dumps(dict(what=what, groups=G, rows=n, ms=round(best * 1e3, 3), ms_median=round(med * 1e3, 3),
                              spread=round(spread, 3), rows_per_s=round(n / best),
                              bytes_per_row=round(per_row, 3), GBps=round(per_row * n / best / 1e9, 1),
                              hbm_frac=round(per_row * n / best / 1e9 / HBM_PEAK_GBS, 4), **extra)), flush=True)

    def col_bytes(c):
        if c.dtype == "utf8":
            return 4 * (c.n_rows + 1) + c.data_bytes + c.n_rows / 8
        return 8 * c.n_rows + c.n_rows / 8

    def contains(what, G, key_cols, probe_cols):
        ks = KeySet.from_data(Table(key_cols), [c.name for c in key_cols])
        names = [c.name for c in probe_cols]
        bitmap = torch.zeros((words + 1) * 8, dtype=torch.uint8, device="cuda")
        types = (ctypes.c_int32 * len(names))(*[_gpu_type(c.dtype) for c in probe_cols])
        views = (L.ColumnView * len(names))(*[c.view() for c in probe_cols])
        nc = ctypes.c_int64()
        timing = timed(lambda: L.check(L.lib.dq_freq_contains_rows(ks.table.handle, types, views, n, None,
                                                                   bitmap.data_ptr(), None, stream, ctypes.byref(nc), None)))
        hashed = len(key_cols) > 1 or key_cols[0].dtype == "utf8"
        table_bytes = 8 * ks.num_keys + (sum(col_bytes(c) - c.n_rows / 8 for c in key_cols) if hashed else 0)
        line(what, ks.num_keys, timing, sum(col_bytes(c) for c in probe_cols) + n / 8, table_bytes,
             hit_rate=round(nc.value / n, 4))

    def unique_baseline(G):
        col = i64_column("k", torch.randint(0, G, (n,), generator=gen, device="cuda"), 0.02)
        state = build_frequencies(Table([col]), ["k"])
        bitmap = torch.zeros((words + 1) * 8, dtype=torch.uint8, device="cuda")
        types = (ctypes.c_int32 * 1)(L.TYPE_I64)
        views = (L.ColumnView * 1)(col.view())
        nu = ctypes.c_int64()
        timing = timed(lambda: L.check(L.lib.dq_freq_unique_rows(state.frequencies.handle, types, views, n,
                                                                 bitmap.data_ptr(), None, stream, ctypes.byref(nu), None)))
        groups = int(L.lib.dq_freq_num_groups(state.frequencies.handle))
        line("dq_freq_unique_rows i64 (plain search)", groups, timing, col_bytes(col) + n / 8, 16 * groups)

    for G in [int(g) for g in args.groups.split(",") if g]:
        ids = torch.randint(0, int(G / 0.9), (n,), generator=gen, device="cuda")
        contains("dq_freq_contains_rows i64", G, [i64_column("id", torch.arange(G, device="cuda"), 0)],
                 [i64_column("k", ids, 0.02)])
        del ids
        unique_baseline(G)
    G = args.hashed_groups
    if G:
        ref = torch.arange(G, device="cuda")
        ids = torch.randint(0, int(G / 0.9), (n,), generator=gen, device="cuda")
        strs = utf8_column("s", ids, 0.02)
        contains("dq_freq_contains_rows utf8", G, [utf8_column("name", ref, 0)], [strs])
        # the pair: a row hits when both parts belong to the same reference row (the string is a function of the id)
        contains("dq_freq_contains_rows (i64, utf8)", G, [i64_column("id", ref, 0), utf8_column("name", ref, 0)],
                 [i64_column("k", ids, 0.02), strs])


if __name__ == "__main__":
    main()
