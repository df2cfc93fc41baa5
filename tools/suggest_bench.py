#!/usr/bin/env python3
"""Time the constraint-suggestion path on a synthetic c5_table (8 fp64 + 4 int64 + 4 UTF8 columns, 10 % NULLs).

    python tools/suggest_bench.py [--rows 4000000] [--reps 3] [--ratio 0.1]

Prints one JSON line each for (a) dq_split_rows alone (launch, the counter's read-back and the stream synchronisation
included), (b) the split plus both take_rows compactions, (c) ColumnProfiler.profile alone, (d) the full runner
without and with a train / test split, and the difference (d, no split) - (c): the host-only rule work.
GB/s of (a) counts the two bitmaps written; of (b) those plus every output buffer.  No threshold is set here.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    import torch

    from deequ_amd import suggestions as S
    from deequ_amd import synth
    from deequ_amd.profiles import ColumnProfiler
    from deequ_amd.split import random_split, split_bitmaps

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.1)
    args = ap.parse_args()
    n = args.rows
    table = synth.c5_table(n, seed=7)
    rules = list(S.Rules.DEFAULT) + [S.UniqueIfApproximatelyUniqueRule()]

    def best_of(fn):
        best, out = float("inf"), None
        for _ in range(args.reps + 1):  # (the first call warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best, out

    def line(what, secs, **extra):
        print(json.dumps(dict(what=what, rows=n, ms=round(secs * 1e3, 3), rows_per_s=round(n / secs), **extra)), flush=True)

    t, b = best_of(lambda: split_bitmaps(n, 0, 0, args.ratio))
    line("dq_split_rows", t, GBps=round(2 * n / 8 / t / 1e9, 2), train=b.num_train, test=b.num_test)
    t, sp = best_of(lambda: random_split(table, args.ratio, 0))
    out_bytes = sum(c.values.numel() + (c.offsets.numel() if c.offsets is not None else 0) +
                    (c.validity.numel() if c.validity is not None else 0)
                    for side in (sp.train, sp.test) for c in side.columns.values())
    line("split+take_rows", t, GBps=round((2 * n / 8 + out_bytes) / t / 1e9, 1), train=sp.numTrain, test=sp.numTest)
    t_profile, _ = best_of(lambda: ColumnProfiler.profile(table))
    line("ColumnProfiler.profile", t_profile)
    t_run, res = best_of(lambda: S.ConstraintSuggestionRunner().onData(table).addConstraintRules(rules).run())
    n_sugg = sum(len(v) for v in res.constraintSuggestions.values())
    line("runner(no split)", t_run, suggestions=n_sugg)
    print(json.dumps(dict(what="runner(no split) - profile = host rule work", rows=n,
                          ms=round((t_run - t_profile) * 1e3, 3),
                          share_of_profile=round((t_run - t_profile) / t_profile, 4))), flush=True)
    t_split, res = best_of(lambda: S.ConstraintSuggestionRunner().onData(table).addConstraintRules(rules)
                           .useTrainTestSplitWithTestsetRatio(args.ratio, 0).run())
    line("runner(split)", t_split, suggestions=sum(len(v) for v in res.constraintSuggestions.values()),
         status=res.verificationResult.status.name, train=res.numRecords)


if __name__ == "__main__":
    main()
