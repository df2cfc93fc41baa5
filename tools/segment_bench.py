#!/usr/bin/env python3
"""Time the segmented scan: dq_freq_lookup_rows + dq_segment_order + dq_segment_scan of one chunk.

    python tools/segment_bench.py [--rows 4000000] [--groups 16,4096,1048576] [--reps 5]

One JSON line per case.  A table of --rows rows: an i64 key column of G distinct values (uniform), four f64 columns
with 5 % NULLs.  Eight slots: the statistics of the four columns without a filter and under one `where` bitmap that
keeps half of the rows.  Per G:

  lookup / order / scan   each call alone on data that is on the device, with its stream synchronisation
  total                   their sum: what a chunk of a segmented run costs once the key set exists
  filtered_analyzers      G = 16 only: the only way without segmentBy -- one ordinary AnalysisRunner run of 16 x 8
                          filtered analyzers (Mean / Maximum of each column under `k = v`, and under `k = v AND h = 1`).
                          For the larger G no equivalent exists (4096 or a million `where` texts in one run), so their
                          figures stand alone.

One warm-up call, then --reps timed ones; ms is the best, ms_median the median and spread (max - min) / median of the
timed calls.  Data is generated on the device from a seed.  No threshold is set here.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    import torch

    import deequ_amd as dq
    from deequ_amd import _lib as L
    from deequ_amd import segments
    from deequ_amd.matching import KeySet, _lookup, where_bitmaps
    from deequ_amd.table import Column, Table

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--groups", default="16,4096,1048576")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n = args.rows
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)

    def padded(t, extra=16):
        raw = t.contiguous().view(torch.uint8).reshape(-1)
        return torch.cat([raw, torch.zeros((-len(raw)) % 16 + extra, dtype=torch.uint8, device="cuda")])

    def bitmap(keep):
        words = (n + 63) // 64
        bits = torch.zeros(words * 64, dtype=torch.uint8, device="cuda")
        bits[:n] = keep.to(torch.uint8)
        weights = (2 ** torch.arange(8, device="cuda", dtype=torch.int32)).to(torch.uint8)
        packed = (bits.reshape(-1, 8) * weights).sum(1).to(torch.uint8)
        return torch.cat([packed, torch.zeros(8, dtype=torch.uint8, device="cuda")])

    def timed(fn):
        fn()
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ms)
        return {"ms": round(min(ms), 3), "ms_median": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 3)}

    values = [Column(f"x{j}", "f64", n, padded(torch.randn(n, generator=gen, device="cuda", dtype=torch.float64)),
                     bitmap(torch.rand(n, generator=gen, device="cuda") >= 0.05), None, nullable=True) for j in range(4)]
    half = Column("h", "i32", n, padded(torch.randint(0, 2, (n,), generator=gen, device="cuda", dtype=torch.int32)), None,
                  None, nullable=False)
    for G in [int(g) for g in args.groups.split(",")]:
        key = Column("k", "i64", n, padded(torch.randint(0, G, (n,), generator=gen, device="cuda", dtype=torch.int64)),
                     None, None, nullable=False)
        t = Table([key, half] + values)
        ks = KeySet.from_data(t, ["k"])
        where = where_bitmaps([t], "h = 1")[0]
        found = ks.num_keys
        seg, _ = _lookup(ks, t, ["k"])
        perm, offsets = segments.segment_order(seg, n, found)
        slots = []
        for filt in (None, where):
            for c in values:
                s = L.SegmentSlot()
                s.op, s.type = L.SEG_STATS, c.type_code
                s.col.values, s.col.validity = c.values.data_ptr(), c.validity.data_ptr()
                s.filter = None if filt is None else filt.data_ptr()
                slots.append(s)
        out = {"case": "segment", "rows": n, "groups": found, "slots": len(slots), "tile": segments.TILE,
               "lookup": timed(lambda: _lookup(ks, t, ["k"])),
               "order": timed(lambda: segments.segment_order(seg, n, found)),
               "scan": timed(lambda: segments.segment_scan(slots, perm, offsets, found + 1))}
        out["total_ms"] = round(out["lookup"]["ms"] + out["order"]["ms"] + out["scan"]["ms"], 3)
        out["gb_per_s_scan"] = round(len(slots) * n * 8 / out["scan"]["ms"] / 1e6, 1)
        if found <= 16:
            an = []
            for v in range(found):
                for c in values:
                    for w in (f"k = {v}", f"k = {v} AND h = 1"):
                        an += [dq.Mean(c.name, where=w), dq.Maximum(c.name, where=w)]
            out["filtered_analyzers"] = dict(timed(lambda: dq.AnalysisRunner.onData(t).addAnalyzers(an).run()),
                                             analyzers=len(an))
        else:
            out["filtered_analyzers"] = None  # no equivalent without segmentBy at this G
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
