#!/usr/bin/env python3
"""Time the dataset match: dq_freq_lookup_rows + dq_rows_match (does a row equal the reference's row with its key?).

    python tools/datamatch_bench.py [--rows 100000000] [--reps 7] [--groups 1024,1048576,16777216]

One JSON line per case and G.  Cases: an i64 key with one f64 compare column; with four mixed columns (f64, i64, i32,
f32); with one utf8 column of 8..16 bytes.  The probe has --rows rows generated on the device from a seed: about 2 %
NULL keys, about 90 % of the keys found (ids drawn from [0, G / 0.9)), about 1 % of the found rows differing from the
reference (in the first compare column).  The reference has G rows; its payload is gathered by KeyedRows.from_data.

Per line: `match` is the pair of calls a chunk costs (lookup, then match, with the per-column counts), `lookup` and
`compare` each call alone, and two yardsticks taken in the same run, alternating with them rep by rep:
`contains` -- dq_freq_contains_rows on the same keys and rows, the floor of the lookup -- and `copy` -- a device copy
of as many bytes as the model says the pair moves.  Each is the whole call into buffers allocated once: one warm-up
round, then --reps timed ones; ms is the best, ms_median the median, spread (max - min) / median.  bytes_per_row is
the model: lookup = key bytes + validity bit + 4 (group out) + the table's keys over the rows; compare = 4 (group in)
+ the compare columns' bytes + the payload's value bytes for the found rows + 1/8 out.  No threshold is set here.
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
    from deequ_amd.grouping import _gpu_type
    from deequ_amd.matching import KeyedRows
    from deequ_amd.table import Column, Table

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--groups", default="1024,1048576,16777216")
    ap.add_argument("--cases", default="f64,mixed,utf8")
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

    def fixed(name, dtype, values, null_rate=0.0):
        return Column(name, dtype, len(values), padded(values), validity(len(values), null_rate) if null_rate else None,
                      None, nullable=bool(null_rate))

    def utf8_column(name, ids):
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
        return Column(name, "utf8", m, padded(data), None, padded(offs.to(torch.int32)), nullable=False, data_bytes=total)

    # the compare columns of a case as functions of the id: (name, dtype, value bytes per row, maker)
    makers = {
        "f64": lambda: [("amount", "f64", 8, lambda ids: fixed("amount", "f64", ids.to(torch.float64) * 0.5))],
        "mixed": lambda: [("amount", "f64", 8, lambda ids: fixed("amount", "f64", ids.to(torch.float64) * 0.5)),
                          ("units", "i64", 8, lambda ids: fixed("units", "i64", ids * 3)),
                          ("day", "i32", 4, lambda ids: fixed("day", "i32", (ids % 100_000).to(torch.int32))),
                          ("rate", "f32", 4, lambda ids: fixed("rate", "f32", (ids % 4096).to(torch.float32) * 0.25))],
        # (4 offset bytes + 12 string bytes on average)
        "utf8": lambda: [("name", "utf8", 16, lambda ids: utf8_column("name", ids))],
    }

    def alternating(fns):
        """Every function once per round, in turn; the first round warms up.  {name: (best, median, spread)}."""
        times = {k: [] for k in fns}
        for _ in range(args.reps + 1):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        return {k: (min(t[1:]), statistics.median(t[1:]), (max(t[1:]) - min(t[1:])) / statistics.median(t[1:]))
                for k, t in times.items()}

    def run(case, G):
        spec = makers[case]()
        ref_ids = torch.arange(G, device="cuda")
        ref = Table([fixed("id", "i64", ref_ids * STRIDE)] + [make(ref_ids) for _, _, _, make in spec])
        kr = KeyedRows.from_data(ref, "id")
        del ref
        ids = torch.randint(0, int(G / 0.9), (n,), generator=gen, device="cuda")
        key = fixed("k", "i64", ids * STRIDE, 0.02)
        drift = torch.rand(n, generator=gen, device="cuda") < 0.01
        cols = [make(ids + drift if i == 0 else ids) for i, (_, _, _, make) in enumerate(spec)]
        del ids, drift
        k = len(cols)
        group = torch.full((n + 4,), -1, dtype=torch.int32, device="cuda")
        bitmap = torch.zeros((words + 1) * 8, dtype=torch.uint8, device="cuda")
        contained = torch.zeros((words + 1) * 8, dtype=torch.uint8, device="cuda")
        ktypes, kviews = (ctypes.c_int32 * 1)(L.TYPE_I64), (L.ColumnView * 1)(key.view())
        types = (ctypes.c_int32 * k)(*[_gpu_type(c.dtype) for c in cols])
        views = (L.ColumnView * k)(*[c.view() for c in cols])
        pcols = [kr.payload.columns[name] for name, _, _, _ in spec]
        ptypes = (ctypes.c_int32 * k)(*[_gpu_type(c.dtype) for c in pcols])
        pviews = (L.ColumnView * k)(*[c.view() for c in pcols])
        nf, nm, nfound, na, nc = (ctypes.c_int64() for _ in range(5))
        mis = (ctypes.c_int64 * k)()
        handle = kr.key_set.table.handle

        def lookup():
            L.check(L.lib.dq_freq_lookup_rows(handle, ktypes, kviews, n, None, group.data_ptr(), stream, ctypes.byref(nf)))

        def compare():
            L.check(L.lib.dq_rows_match(types, views, ptypes, pviews, k, n, kr.payload.num_rows, group.data_ptr(), None,
                                        bitmap.data_ptr(), None, None, 0, stream, ctypes.byref(nm), ctypes.byref(nfound),
                                        ctypes.byref(na), mis))

        def both():
            lookup()
            compare()

        def contains():
            L.check(L.lib.dq_freq_contains_rows(handle, ktypes, kviews, n, None, contained.data_ptr(), None, stream,
                                                ctypes.byref(nc), None))

        both()  # (the found fraction, for the model)
        found = nfound.value / n
        value_bytes = sum(b for _, _, b, _ in spec)
        lookup_bytes = 8 + 1 / 8 + 4 + 8 * G / n
        compare_bytes = 4 + value_bytes + found * value_bytes + 1 / 8
        total = int((lookup_bytes + compare_bytes) * n)
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")  # (a copy reads and writes: half each)
        dst = torch.empty_like(src)
        t = alternating({"match": both, "contains": contains, "copy": lambda: dst.copy_(src), "lookup": lookup,
                         "compare": compare})
        out = dict(what=f"dataset match i64 key + {case}", groups=G, rows=n, columns=k, found=round(found, 4),
                   matched=round(nm.value / n, 4), mismatch=list(mis),
                   bytes_per_row=round(lookup_bytes + compare_bytes, 3),
                   lookup_bytes_per_row=round(lookup_bytes, 3), compare_bytes_per_row=round(compare_bytes, 3))
        for name, (best, med, spread) in t.items():
            out[name] = dict(ms=round(best * 1e3, 3), ms_median=round(med * 1e3, 3), spread=round(spread, 3))
        best = t["match"][0]
        out["rows_per_s"] = round(n / best)
        out["GBps"] = round(total / best / 1e9, 1)
        out["hbm_frac"] = round(total / best / 1e9 / HBM_PEAK_GBS, 4)
        out["copy_GBps"] = round(total / t["copy"][0] / 1e9, 1)
        print(json.dumps(out), flush=True)

    for case in [c for c in args.cases.split(",") if c]:
        for G in [int(g) for g in args.groups.split(",") if g]:
            run(case, G)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
