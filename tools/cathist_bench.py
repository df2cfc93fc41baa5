#!/usr/bin/env python3
"""Fused categorical histograms (dq_cat_hist_build) against one build_frequencies call per column, on the same
device-resident data, timed with the same device events.

  python tools/cathist_bench.py [--rows 100000000] [--k 1,4,16] [--d 2,120,480] [--reps 5] [--out FILE.json]

K string columns drawn uniformly from D values of 4..20 bytes plus one boolean column, 10 % NULLs each.  Both paths
are warmed up, then timed alternately `reps` times; the median call time (each call ends in a stream synchronise of
its own, so this is the call, not its enqueue) and the rate over the algorithmic bytes -- offsets + string bytes +
validity of the columns read, counted from the shapes -- are printed per (K, D), and the two paths' counts compared.
The per-column path reads the boolean column too (one more build_frequencies call), so both do the same work.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _validity(torch, n, null_fraction, gen):
    words = (n + 63) // 64
    bits = (torch.rand(words * 64, device="cuda", generator=gen) >= null_fraction)
    bits[n:] = False
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device="cuda")
    packed = (bits.view(-1, 8).to(torch.int32) * w).sum(dim=1).to(torch.uint8)
    return torch.cat([packed, torch.zeros(8, dtype=torch.uint8, device="cuda")])


def string_column(torch, name, n, d, seed, null_fraction=0.1, block=1 << 24):
    """A utf8 Column of n rows drawn from d values, built on the device block by block."""
    from deequ_amd.table import Column

    gen = torch.Generator(device="cuda").manual_seed(seed)
    pool = [f"{seed % 97:02d}{i:03d}".encode() + b"abcdefghijklmno"[: (i * 7 + seed) % 16] for i in range(d)]  # 5..20 bytes
    pool_len = torch.tensor([len(p) for p in pool], dtype=torch.int64, device="cuda")
    pool_off = torch.cumsum(pool_len, 0) - pool_len
    pool_bytes = torch.frombuffer(bytearray(b"".join(pool)), dtype=torch.uint8).cuda()
    idx = torch.randint(0, d, (n,), device="cuda", generator=gen)
    lens = pool_len[idx]
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=offs[1:])
    total = int(offs[-1])
    assert total < 2 ** 31, "utf8 chunk exceeds 2 GiB: fewer rows"
    data = torch.zeros((total + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda")
    for a in range(0, n, block):
        b = min(n, a + block)
        rows = torch.repeat_interleave(torch.arange(a, b, device="cuda"), lens[a:b])
        lo, hi = int(offs[a]), int(offs[b])
        pos = torch.arange(lo, hi, device="cuda") - offs[rows]
        data[lo:hi] = pool_bytes[pool_off[idx[rows]] + pos]
    o32 = torch.cat([offs.to(torch.int32), torch.zeros(8, dtype=torch.int32, device="cuda")]).view(torch.uint8)
    return Column(name, "utf8", n, data, _validity(torch, n, null_fraction, gen), o32, nullable=True, data_bytes=total)


def bool_column(torch, name, n, seed, null_fraction=0.1):
    from deequ_amd.table import Column

    gen = torch.Generator(device="cuda").manual_seed(seed)
    values = torch.cat([_validity(torch, n, 0.5, gen), torch.zeros(16, dtype=torch.uint8, device="cuda")])
    return Column(name, "bool", n, values, _validity(torch, n, null_fraction, gen), None, nullable=True)


def algorithmic_bytes(columns, n):
    """offsets + string bytes + validity (a boolean column: its value bits + validity)"""
    total = 0
    for c in columns:
        total += (n + 7) // 8
        total += (n + 7) // 8 if c.dtype == "bool" else 4 * (n + 1) + c.data_bytes
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--k", default="1,4,16")
    ap.add_argument("--d", default="2,120,480")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "cathist_bench needs a GPU: there is no CPU path to time"
    from deequ_amd.grouping import build_frequencies
    from deequ_amd.profiles import build_cat_hist
    from deequ_amd.table import Table

    ks = [int(x) for x in args.k.split(",")]
    ds = [int(x) for x in args.d.split(",")]
    n = args.rows
    results = []

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop), out

    for d in ds:
        strings = [string_column(torch, f"s{k}", n, d, seed=1000 * d + k) for k in range(max(ks))]
        flag = bool_column(torch, "b", n, seed=d)
        for k in ks:
            cols = strings[:k] + [flag]
            table = Table(cols)
            names = [c.name for c in cols]
            fused = lambda: build_cat_hist(table, names)
            per_column = lambda: [build_frequencies(table, [name]).frequencies.export()[1] for name in names]
            for _ in range(2):  # warm-up of both paths at this shape
                f_out, p_out = fused(), per_column()
            for (status, _, counts, _), pc in zip(f_out, p_out):  # same multiset of counts from both
                assert status == 0 and sorted(counts.tolist()) == sorted(pc.tolist())
            tf, tp = [], []
            for _ in range(args.reps):  # alternating, so drift hits both alike
                tf.append(timed(fused)[0])
                tp.append(timed(per_column)[0])
            nbytes = algorithmic_bytes(cols, n)
            row = {"rows": n, "K": k, "D": d, "bytes": nbytes, "fused_ms": statistics.median(tf),
                   "per_column_ms": statistics.median(tp), "fused_ms_all": tf, "per_column_ms_all": tp}
            row["fused_TBps"] = nbytes / (row["fused_ms"] * 1e-3) / 1e12
            row["per_column_TBps"] = nbytes / (row["per_column_ms"] * 1e-3) / 1e12
            results.append(row)
            print(f"K={k:2d} D={d:3d} rows={n}: fused {row['fused_ms']:8.3f} ms ({row['fused_TBps']:.3f} TB/s)   "
                  f"per-column {row['per_column_ms']:8.3f} ms ({row['per_column_TBps']:.3f} TB/s)   "
                  f"x{row['per_column_ms'] / row['fused_ms']:.2f}", flush=True)
        del strings, flag
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/cathist_bench.py", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
