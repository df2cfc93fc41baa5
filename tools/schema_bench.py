#!/usr/bin/env python3
"""Time RowLevelSchemaValidator on a CSV-shaped table of short strings: an id, an amount and a timestamp column.

    python tools/schema_bench.py [--rows 20000000] [--reps 5]

Prints one JSON line each for the verdict pass alone (dq_schema_validate: launch, the counters' read-back and the
stream synchronisation included), for the whole validate (verdict, both compactions) and, as a yardstick,
dq_cast_utf8 to i64 over the id column.  GB/s counts the algorithmic bytes of the pass: offsets, string bytes and
validity read; bitmaps, cast values and their validity written (validate: plus the bytes of both outputs).
No threshold is set here.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def string_column(name, pieces, valid):
    """A utf8 Column from fixed-width ASCII pieces (a numpy S-array) without a Python loop per row."""
    import torch

    from deequ_amd.table import Column, pack_validity

    lens = np.char.str_len(pieces).astype(np.int64)
    lens[~valid] = 0
    offs = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    width = pieces.dtype.itemsize
    flat = np.frombuffer(pieces.tobytes(), dtype=np.uint8).reshape(len(pieces), width)
    data = flat[np.arange(width)[None, :] < lens[:, None]]
    pad = (-len(data)) % 16 + 16
    return Column(name, "utf8", len(pieces), torch.from_numpy(np.concatenate([data, np.zeros(pad, np.uint8)])).cuda(),
                  torch.from_numpy(pack_validity(valid)).cuda(),
                  torch.from_numpy(np.concatenate([offs.astype(np.int32), np.zeros(4, np.int32)]).view(np.uint8)).cuda(),
                  nullable=True, data_bytes=int(offs[-1]))


def main() -> None:
    import torch

    from deequ_amd.casts import cast_column
    from deequ_amd.schema import RowLevelSchema, RowLevelSchemaValidator
    from deequ_amd.table import Table

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n, rng = args.rows, np.random.default_rng(1)
    ids = rng.integers(-1000, 10 ** 9, n).astype("S")
    ids[rng.random(n) < 0.02] = b"N/A"
    cents = rng.integers(0, 10 ** 7, n)
    amounts = np.char.add(np.char.add((cents // 100).astype("S"), b"."), np.char.zfill((cents % 100).astype("S"), 2))
    secs = rng.integers(0, 86400 * 365, n)
    stamps = np.char.add(b"2012-07-", np.char.add(np.char.zfill((1 + secs % 28).astype("S"), 2), np.char.add(
        b" ", np.char.add(np.char.zfill((secs // 3600 % 24).astype("S"), 2), np.char.add(
            b":", np.char.add(np.char.zfill((secs // 60 % 60).astype("S"), 2), np.char.add(b":", np.char.zfill((secs % 60).astype("S"), 2))))))))
    stamps[rng.random(n) < 0.01] = b"yesterday"
    table = Table([string_column(name, p, rng.random(n) >= 0.03) for name, p in (("id", ids), ("amount", amounts), ("created", stamps))])
    schema = (RowLevelSchema().withIntColumn("id", minValue=0).withDecimalColumn("amount", 10, 2)
              .withTimestampColumn("created", "yyyy-MM-dd HH:mm:ss", isNullable=False))
    read = sum(4 * (n + 1) + c.data_bytes + n / 8 for c in table.columns.values())
    verdict_bytes = read + 2 * n / 8 + (4 + 16 + 8) * n + 3 * n / 8

    def best_of(fn):
        best, out = float("inf"), None
        for _ in range(args.reps + 1):  # (the first call warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best, out

    def line(what, secs_, nbytes, **extra):
        print(json.dumps(dict(what=what, rows=n, ms=round(secs_ * 1e3, 3), rows_per_s=round(n / secs_), algorithmic_GB=round(nbytes / 1e9, 3),
                              GBps=round(nbytes / secs_ / 1e9, 1), **extra)))

    plan_positions = RowLevelSchemaValidator._positions(table, schema)
    from deequ_amd.schema import SchemaPlan

    plan = SchemaPlan(schema, plan_positions)
    t, v = best_of(lambda: RowLevelSchemaValidator.verdict(table, schema, plan))
    plan.close()
    line("verdict", t, verdict_bytes, valid=v.num_valid, invalid=v.num_invalid)
    t, res = best_of(lambda: RowLevelSchemaValidator.validate(table, schema))
    out_bytes = sum(c.values.numel() + (c.offsets.numel() if c.offsets is not None else 0)
                    for tb in (res.validRows, res.invalidRows) for c in tb.columns.values())
    line("validate", t, verdict_bytes + out_bytes + 8 * (res.numValidRows + res.numInvalidRows), valid=res.numValidRows, invalid=res.numInvalidRows)
    col = table.columns["id"]
    t, _ = best_of(lambda: cast_column(col, "i64"))
    line("dq_cast_utf8_i64(id)", t, 4 * (n + 1) + col.data_bytes + n / 8 + 8 * n + n / 8)


if __name__ == "__main__":
    main()
