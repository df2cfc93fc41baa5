#!/usr/bin/env python3
"""Time dq_bin_count (the counting pass of Histogram's `binning`) alone, and its yardstick.

    python tools/binhist_bench.py [--rows 64000000] [--reps 7]

One JSON line per case: the best and the median device time of one call (HIP events around it; after one warm-up),
rows per second and the bytes moved per second as a fraction of the HBM peak: the column's values and one validity
bit per row read, nothing written but the k + 3 counts.  Cases: f64 and i32 columns; 10, 100 and 4096 evenly spaced
bins, and 100 unevenly spaced ones (binary search instead of the first guess); values uniform over the bins, and every
value in one bin -- the LDS-contention case.  The yardstick for an LDS counting pass is dq_dict_count over the same
number of rows, with as many dictionary entries as there are bins, under the same two distributions.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E


def main() -> None:
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.table import Column, Dictionary, pack_validity, utf8_column

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    n = args.rows
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    device = torch.cuda.current_device()
    gen = torch.Generator(device="cuda").manual_seed(1)
    valid = np.random.default_rng(2).random(n) >= 0.05
    validity = torch.from_numpy(pack_validity(valid)).cuda()
    n_valid = int(np.count_nonzero(valid))
    del valid

    def timed(call):
        """best and median milliseconds of `call`, args.reps times after one warm-up"""
        times = []
        for rep in range(args.reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(t0.elapsed_time(t1))
        return min(times), statistics.median(times)

    def report(kernel, dtype, bins, spacing, values, width, best, median):
        moved = width * n + n / 8
        print(json.dumps({"kernel": kernel, "dtype": dtype, "bins": bins, "edges": spacing, "values": values, "rows": n,
                          "ms_best": round(best, 3), "ms_median": round(median, 3),
                          "rows_per_s": round(n / (best * 1e-3)), "GBps": round(moved / (best * 1e-3) / 1e9, 1),
                          "fraction_of_hbm_peak": round(moved / (best * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}), flush=True)

    def column(dtype, t):
        raw = t.view(torch.uint8)
        raw = torch.cat([raw, torch.zeros(16 + (-raw.numel()) % 16, dtype=torch.uint8, device="cuda")])
        return Column("x", dtype, n, raw, validity, None, nullable=True)

    lo, hi = 0.0, 4096.0
    for dtype, width in (("f64", 8), ("i32", 4)):
        uniform = torch.rand(n, device="cuda", dtype=torch.float64, generator=gen) * (hi - lo) + lo
        columns = {"uniform": uniform if dtype == "f64" else uniform.to(torch.int32),
                   "one bin": torch.full((n,), 1.0 if dtype == "f64" else 1, device="cuda",
                                         dtype=torch.float64 if dtype == "f64" else torch.int32)}
        del uniform
        for k, spacing in ((10, "even"), (100, "even"), (100, "uneven"), (4096, "even")):
            edges = np.linspace(lo, hi, k + 1)
            if spacing == "uneven":
                w = edges[1] - edges[0]
                edges[1:-1:2] += 0.45 * w
            arr = (ctypes.c_double * (k + 1))(*edges.tolist())
            h = ctypes.c_void_p()
            L.check(L.lib.dq_bins_create(arr, k + 1, device, ctypes.byref(h)))
            counts = torch.zeros(k + 3, dtype=torch.int64, device="cuda")
            for values, t in columns.items():
                col = column(dtype, t)
                view = col.view()
                counts.zero_()
                best, median = timed(lambda: L.check(L.lib.dq_bin_count(h, col.type_code, ctypes.byref(view), n,
                                                                        counts.data_ptr(), device, stream)))
                assert int(counts.sum().item()) == (args.reps + 1) * n_valid  # every pass counted every non-NULL row
                report("dq_bin_count", dtype, k, spacing, values, width, best, median)
                del col
            L.lib.dq_bins_destroy(h)
        del columns

    # the yardstick: dq_dict_count, an LDS counting pass over int32 indices, as many entries as bins
    for d_entries in (10, 100, 4096):
        d = Dictionary(utf8_column("x", [b"v%d" % i for i in range(d_entries)]))
        for values in ("uniform", "one bin"):
            if values == "uniform":
                idx = torch.randint(0, d_entries, (n,), device="cuda", dtype=torch.int32, generator=gen)
            else:
                idx = torch.ones(n, device="cuda", dtype=torch.int32)
            raw = torch.cat([idx.view(torch.uint8), torch.zeros(16, dtype=torch.uint8, device="cuda")])
            col = Column("x", "dict_utf8", n, raw, validity, None, nullable=True, dictionary=d)
            view = col.view()
            counts = torch.zeros(d_entries, dtype=torch.int64, device="cuda")
            best, median = timed(lambda: L.check(L.lib.dq_dict_count(ctypes.byref(view), n, counts.data_ptr(), device,
                                                                     stream)))
            report("dq_dict_count", "dict_utf8 (int32 indices)", d_entries, "-", values, 4, best, median)
            del col, raw, idx


if __name__ == "__main__":
    main()
