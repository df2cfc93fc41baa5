#!/usr/bin/env python3
"""Time dq_cast_utf8 (Cast of a string column to long / double) on a column of short numeric strings.

    python tools/cast_bench.py [--rows 100000000] [--reps 5]

Prints, per target type, the best wall time of one call (launch, the NULL / hard-row counters' read-back and the
stream synchronisation included) and the fraction of the HBM peak its algorithmic bytes amount to: offsets, string
bytes and validity read, values and validity written.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E


def numeric_strings(n: int, seed: int = 1):
    """n strings of 1..12 bytes: digits, a third with a point inside, a fifth with a sign."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 13, n, dtype=np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    data = rng.integers(ord("0"), ord("9") + 1, int(offs[-1]), dtype=np.uint8)
    signed = (rng.random(n) < 0.2) & (lens > 1)
    data[offs[:-1][signed]] = ord("-")
    pointed = (rng.random(n) < 0.33) & (lens > 3)
    data[(offs[:-1] + lens // 2)[pointed]] = ord(".")
    return data, offs


def main() -> None:
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.table import Column, pack_validity

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n = args.rows
    data, offs = numeric_strings(n)
    pad = (-len(data)) % 16 + 16
    valid = np.random.default_rng(2).random(n) >= 0.05
    col = Column("s", "utf8", n, torch.from_numpy(np.concatenate([data, np.zeros(pad, np.uint8)])).cuda(),
                 torch.from_numpy(pack_validity(valid)).cuda(),
                 torch.from_numpy(np.concatenate([offs.astype(np.int32), np.zeros(4, np.int32)]).view(np.uint8)).cuda(),
                 nullable=True, data_bytes=len(data))
    algo = 4 * (n + 1) + len(data) + n / 8 + 8 * n + n / 8
    values = torch.empty(8 * n + 16, dtype=torch.uint8, device="cuda")
    validity = torch.empty(((n + 63) // 64 + 1) * 8, dtype=torch.uint8, device="cuda")
    view = col.view()
    stream = torch.cuda.current_stream().cuda_stream
    for to, code in (("i64", L.TYPE_I64), ("f64", L.TYPE_F64)):
        best = float("inf")
        nulls = ctypes.c_int64(0)
        for _ in range(args.reps + 1):  # (the first call warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            L.check(L.lib.dq_cast_utf8(col.type_code, ctypes.byref(view), n, code, values.data_ptr(),
                                       validity.data_ptr(), torch.cuda.current_device(), stream, ctypes.byref(nulls)))
            best = min(best, time.perf_counter() - t0)
        print(json.dumps({"target": to, "rows": n, "data_bytes": len(data), "ms": round(best * 1e3, 3), "null_rows": nulls.value,
                          "algorithmic_GB": round(algo / 1e9, 3), "GBps": round(algo / best / 1e9, 1),
                          "fraction_of_hbm_peak": round(algo / best / 1e9 / HBM_PEAK_GBS, 4)}))


if __name__ == "__main__":
    main()
