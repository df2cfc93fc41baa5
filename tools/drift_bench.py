#!/usr/bin/env python3
"""Time dq_freq_distance and dq_freq_ks (distribution drift: the distance between two frequency tables).

    python tools/drift_bench.py [--groups 65536,1048576,4194304] [--reps 7]

One JSON line per case.  Two tables of G groups each, 90 % of which they share (ids [0, G) against [G / 10,
G + G / 10)), every group with a count of 1..4: a single i64 column (unhashed tables: the key is the value) and a utf8
column of 8..16 bytes (hashed tables, a found hash compared with the stored strings).  Per case:

  dq_freq_distance / dq_freq_ks   the whole call on tables that are already on the device: the launches, the result's
                                  read-back, the stream synchronisation
  export + numpy join             what a user could do before these entries: FreqTable.export() of both tables (keys
                                  and counts to the host) and the same three distances from a numpy join of the keys
                                  (np.intersect1d on the sorted keys; a hashed table's keys are its hashes, so this join
                                  does not even compare the values)

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

STRIDE = 7919  # key = id * STRIDE: gaps between neighbouring keys


def main() -> None:
    import numpy as np
    import torch

    from deequ_amd.drift import freq_distance, freq_ks
    from deequ_amd.grouping import build_frequencies
    from deequ_amd.table import Column, Table

    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="65536,1048576,4194304")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)

    def padded(t, extra=16):
        raw = t.contiguous().view(torch.uint8).reshape(-1)
        return torch.cat([raw, torch.zeros((-len(raw)) % 16 + extra, dtype=torch.uint8, device="cuda")])

    def i64_column(name, ids):
        return Column(name, "i64", len(ids), padded(ids * STRIDE), None, None, nullable=False)

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
        return Column(name, "utf8", m, padded(data), None, padded(offs.to(torch.int32)), nullable=False,
                      data_bytes=total)

    def rows_of(first, G):
        """Group ids first .. first + G - 1, each 1..4 times, in random order."""
        ids = torch.arange(first, first + G, device="cuda")
        ids = torch.repeat_interleave(ids, torch.randint(1, 5, (G,), generator=gen, device="cuda"))
        return ids[torch.randperm(len(ids), generator=gen, device="cuda")]

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

    def line(what, kind, G, timing, **extra):
        best, med, spread = timing
        print(json.dumps(dict(what=what, table=kind, groups_per_table=G, ms=round(best * 1e3, 3),
                              ms_median=round(med * 1e3, 3), spread=round(spread, 3),
                              groups_per_s=round(2 * G / best), **extra)), flush=True)

    def export_and_join(a, b):
        (ka, ca), (kb, cb) = a.export(), b.export()
        na, nb = float(ca.sum()), float(cb.sum())
        _, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
        only_a, only_b = np.ones(len(ka), bool), np.ones(len(kb), bool)
        only_a[ia], only_b[ib] = False, False
        p = np.concatenate([ca[ia] / na, ca[only_a] / na, np.zeros(int(only_b.sum()))])
        q = np.concatenate([cb[ib] / nb, np.zeros(int(only_a.sum())), cb[only_b] / nb])
        d = np.abs(p - q)
        m = (p + q) / 2
        with np.errstate(divide="ignore", invalid="ignore"):
            js = 0.5 * (np.where(p > 0, p * np.log(p / m), 0.0).sum() + np.where(q > 0, q * np.log(q / m), 0.0).sum())
        return d.max(), 0.5 * d.sum(), js

    for G in [int(g) for g in args.groups.split(",") if g]:
        for kind, column in (("i64", i64_column), ("utf8", utf8_column)):
            a = build_frequencies(Table([column("c", rows_of(0, G))]), ["c"]).materialize().frequencies
            b = build_frequencies(Table([column("c", rows_of(G // 10, G))]), ["c"]).materialize().frequencies
            r = freq_distance(a, b)
            host = export_and_join(a, b)
            assert r.linf == host[0] and abs(r.tv - host[1]) < 1e-9 and abs(r.js - host[2]) < 1e-9, (r.linf, host)
            line("dq_freq_distance", kind, G, timed(lambda: freq_distance(a, b)), linf=r.linf, tv=r.tv, js=r.js,
                 common=r.n_common)
            line("export + numpy join", kind, G, timed(lambda: export_and_join(a, b)))
            if kind == "i64":
                line("dq_freq_ks", kind, G, timed(lambda: freq_ks(a, b)), ks=freq_ks(a, b))
            del a, b


if __name__ == "__main__":
    main()
