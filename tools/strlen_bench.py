#!/usr/bin/env python3
"""Time dq_utf8_length (the derived length column of MinLength / MaxLength) alone, and its yardstick.

    python tools/strlen_bench.py [--rows 32000000] [--reps 7]

One JSON line per input: the best and the median wall time of one call (launch, the NULL counter's read-back and the
stream synchronisation included, as tools/cast_bench.py times dq_cast_utf8) and the bytes moved per second: offsets,
string bytes and validity read, 4 bytes per row and validity written.  Inputs: ASCII values of 8..16 bytes, of 16..48
bytes, a mix in which one value in four holds multi-byte characters, and a dictionary column (dq_dict_take_i32 over
its indices; the entries' lengths are computed once, outside the timed call).  The yardstick is dq_cast_utf8(-> i64) on
tools/cast_bench.py's digit strings, which reads the same bytes and does more work per byte; dq_utf8_length runs on
that input too, the two calls alternating.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
BLOCK = 1 << 20        # rows generated; an input is this block repeated


def ascii_block(lo: int, hi: int, seed: int, multibyte_one_in: int = 0):
    """(bytes, int64 offsets) of BLOCK values of lo..hi bytes of printable ASCII; with multibyte_one_in = k every k-th
    value is made of three-byte characters instead (its byte length rounded down to whole characters)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, BLOCK, dtype=np.int64)
    if multibyte_one_in:
        lens[::multibyte_one_in] = np.maximum(3, lens[::multibyte_one_in] // 3 * 3)
    offs = np.zeros(BLOCK + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    data = rng.integers(0x20, 0x7F, int(offs[-1]), dtype=np.uint8)
    if multibyte_one_in:
        row = np.repeat(np.arange(BLOCK), lens)
        inside = np.arange(int(offs[-1])) - offs[:-1][row]
        multi = row % multibyte_one_in == 0
        data[multi] = np.array([0xE6, 0x97, 0xA5], np.uint8)[inside[multi] % 3]  # U+65E5
    return data, offs


def repeat_block(data, offs, n: int):
    k = (n + BLOCK - 1) // BLOCK
    all_offs = (offs[:-1][None, :] + (np.arange(k, dtype=np.int64) * len(data))[:, None]).reshape(-1)
    all_offs = np.concatenate([all_offs[:n], [all_offs[n] if n < k * BLOCK else k * len(data)]])
    return np.tile(data, k)[: int(all_offs[-1])], all_offs


def main() -> None:
    import torch

    from cast_bench import numeric_strings
    from deequ_amd import _lib as L
    from deequ_amd.lengths import _entry_lengths, string_lengths
    from deequ_amd.table import Column, Dictionary, pack_validity, utf8_column

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    n = args.rows
    stream = torch.cuda.current_stream().cuda_stream
    device = torch.cuda.current_device()
    valid = np.random.default_rng(2).random(n) >= 0.05
    validity_in = torch.from_numpy(pack_validity(valid)).cuda()
    lengths = torch.empty(4 * n + 16, dtype=torch.uint8, device="cuda")
    values64 = torch.empty(8 * n + 16, dtype=torch.uint8, device="cuda")
    validity = torch.empty(((n + 63) // 64 + 1) * 8, dtype=torch.uint8, device="cuda")

    def column(data, offs):
        pad = (-len(data)) % 16 + 16
        return Column("s", "utf8", n, torch.from_numpy(np.concatenate([data, np.zeros(pad, np.uint8)])).cuda(), validity_in,
                      torch.from_numpy(np.concatenate([offs.astype(np.int32), np.zeros(4, np.int32)]).view(np.uint8)).cuda(),
                      nullable=True, data_bytes=len(data))

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

    def report(name, kernel, moved, best, median, **more):
        print(json.dumps({"input": name, "kernel": kernel, "rows": n, "ms_best": round(best * 1e3, 3),
                          "ms_median": round(median * 1e3, 3), "bytes_moved_GB": round(moved / 1e9, 3),
                          "GBps": round(moved / best / 1e9, 1),
                          "fraction_of_hbm_peak": round(moved / best / 1e9 / HBM_PEAK_GBS, 4), **more}), flush=True)

    def length_call(col):
        view = col.view()
        nulls = ctypes.c_int64(0)

        def call():
            L.check(L.lib.dq_utf8_length(col.type_code, ctypes.byref(view), n, lengths.data_ptr(), validity.data_ptr(),
                                         device, stream, ctypes.byref(nulls)))
        return call

    def length_bytes(data_bytes):
        return 4 * (n + 1) + data_bytes + n / 8 + 4 * n + n / 8

    for name, block in (("ascii 8..16 B", ascii_block(8, 16, 3)), ("ascii 16..48 B", ascii_block(16, 48, 4)),
                        ("one in four multi-byte, 8..16 B", ascii_block(8, 16, 5, multibyte_one_in=4))):
        data, offs = repeat_block(*block, n)
        col = column(data, offs)
        (best, median), = timed([length_call(col)])
        report(name, "dq_utf8_length", length_bytes(len(data)), best, median, data_bytes=len(data))
        del col

    # a dictionary column: 1000 entries of 8..16 bytes, the rows' indices gathered through the entries' lengths
    edata, eoffs = ascii_block(8, 16, 6)
    entries = [bytes(edata[eoffs[i]:eoffs[i + 1]]) for i in range(1000)]
    idx = np.random.default_rng(7).integers(0, 1000, n, dtype=np.int32)
    d = Dictionary(utf8_column("s", entries))
    dcol = Column("s", "dict_utf8", n, torch.from_numpy(np.concatenate([idx, np.zeros(4, np.int32)]).view(np.uint8)).cuda(),
                  validity_in, None, nullable=True, dictionary=d)
    _entry_lengths(d)
    (best, median), = timed([lambda: string_lengths(dcol)])
    report("dictionary, 1000 entries", "dq_dict_take_i32 (string_lengths: allocation included)",
           4 * n + n / 8 + 4 * n + n / 8, best, median)

    # the yardstick: tools/cast_bench.py's digit strings through dq_cast_utf8(-> i64) and through dq_utf8_length
    data, offs = numeric_strings(n)
    col = column(data, offs)
    view = col.view()
    nulls = ctypes.c_int64(0)

    def cast_call():
        L.check(L.lib.dq_cast_utf8(col.type_code, ctypes.byref(view), n, L.TYPE_I64, values64.data_ptr(),
                                   validity.data_ptr(), device, stream, ctypes.byref(nulls)))

    (cb, cm), (lb, lm) = timed([cast_call, length_call(col)])
    report("digit strings 1..12 B", "dq_cast_utf8 -> i64", 4 * (n + 1) + len(data) + n / 8 + 8 * n + n / 8, cb, cm,
           data_bytes=len(data))
    report("digit strings 1..12 B", "dq_utf8_length", length_bytes(len(data)), lb, lm, data_bytes=len(data))


if __name__ == "__main__":
    main()
