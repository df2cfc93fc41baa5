"""Self-contained frequency states on the device at scale (diagnostic): dq_freq_materialize, dq_freq_merge of two
materialised tables, dq_freq_to_bytes / dq_freq_from_bytes, against the dq_freq_build that produced the table.

    python tools/freq_state_bench.py [--rows 1e8] [--reps 3] [--sweep-groups 2e6]
Two string columns of 16-byte values (device-generated): about 1e3 distinct values, and all values unique.  Per step:
ms, bytes moved (offsets + bytes read at the representative rows, plus the store written: offsets + bytes), the
achieved GB/s, and the time as a fraction of the build.  Then the lane / wave switch of the string gather: unique
strings of several lengths materialised with every string on the lane path and with every string on the wave path
(DQ_FREQ_WAVE_COPY), so that the length at which the wave path wins can be read off.  One JSON line per figure.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    assert torch.cuda.is_available()
    import deequ_amd as dq
    from deequ_amd import _lib as L
    from deequ_amd.grouping import FreqTable, build_frequencies
    from deequ_amd.table import Column

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep-groups", type=float, default=2e6)
    a = ap.parse_args()
    n = int(a.rows)

    def string_table(ids, width):
        """One utf8 column: row r holds ids[r] as 16 hex digits, repeated / cut to `width` bytes."""
        rows = ids.numel()
        shifts = torch.arange(60, -4, -4, device="cuda", dtype=torch.int64)
        nib = (ids.view(-1, 1) >> shifts) & 15
        hexd = (nib + 48 + (nib > 9) * 39).to(torch.uint8)  # 0-9a-f
        reps = (width + 15) // 16
        data = hexd.repeat(1, reps)[:, :width].contiguous().view(-1)
        data = torch.cat([data, torch.zeros(32, dtype=torch.uint8, device="cuda")])
        offs = (torch.arange(rows + 1, device="cuda", dtype=torch.int64) * width).to(torch.int32)
        offs = torch.cat([offs, torch.zeros(8, dtype=torch.int32, device="cuda")])
        return dq.Table([Column("s", "utf8", rows, data, None, offs.view(torch.uint8), nullable=False,
                                data_bytes=rows * width)])

    def timed(fn, reps=a.reps):
        fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            best.append((time.perf_counter() - t0) * 1e3)
        return sorted(best)[len(best) // 2], r

    def report(**kw):
        print(json.dumps(kw), flush=True)

    g = torch.Generator(device="cuda").manual_seed(11)
    for label, ids in (("1e3 distinct", torch.randint(0, 1000, (n,), device="cuda", dtype=torch.int64, generator=g)),
                       ("unique", torch.arange(n, device="cuda", dtype=torch.int64) * 0x9E3779B1 + 12345)):
        t = string_table(ids, 16)
        del ids
        build_ms, _ = timed(lambda: build_frequencies(t, ["s"]))
        report(case=label, step="dq_freq_build", rows=n, ms=round(build_ms, 3))

        def mat():
            s = build_frequencies(t, ["s"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.materialize()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, s

        ms = sorted(mat()[0] for _ in range(a.reps + 1))[:-1]  # (the first call also grows the scratch arena)
        mat_ms = ms[len(ms) // 2]
        st = mat()[1]
        G = L.lib.dq_freq_num_groups(st.frequencies.handle)
        moved = G * 8 + G * 8 + G * 16 + (G + 1) * 8 + G * 16  # row ids, 2 offsets, bytes read; offsets, bytes written
        report(case=label, step="dq_freq_materialize", groups=G, ms=round(mat_ms, 3), bytes=moved,
               gbps=round(moved / mat_ms / 1e6, 1), of_build=round(mat_ms / build_ms, 4))
        other = build_frequencies(t, ["s"]).materialize()
        merge_ms, merged = timed(lambda: st.frequencies.merged(other.frequencies))
        store = (G + 1) * 8 + G * 16
        report(case=label, step="dq_freq_merge (two materialised tables)", groups=2 * G, ms=round(merge_ms, 3),
               bytes=2 * G * 24 + 2 * store + store + G * 24, gbps=round((2 * G * 24 + 3 * store + G * 24) / merge_ms / 1e6, 1),
               of_build=round(merge_ms / build_ms, 4))
        del merged, other
        to_ms, image = timed(lambda: st.frequencies.to_bytes(), reps=1)
        report(case=label, step="dq_freq_to_bytes", ms=round(to_ms, 3), bytes=len(image),
               gbps=round(len(image) / to_ms / 1e6, 2), of_build=round(to_ms / build_ms, 4))
        from_ms, back = timed(lambda: FreqTable.from_bytes(image), reps=1)
        report(case=label, step="dq_freq_from_bytes", ms=round(from_ms, 3), bytes=len(image),
               gbps=round(len(image) / from_ms / 1e6, 2), of_build=round(from_ms / build_ms, 4))
        del st, back, image, t
        torch.cuda.empty_cache()

    m = int(a.sweep_groups)
    for width in (16, 32, 48, 64, 96, 128, 192, 256, 512):
        t = string_table(torch.arange(m, device="cuda", dtype=torch.int64) * 0x9E3779B1 + 7, width)
        row = {"step": "switch sweep", "groups": m, "string_bytes": width}
        for path, knob in (("lane_ms", str(1 << 40)), ("wave_ms", "1")):
            os.environ["DQ_FREQ_WAVE_COPY"] = knob
            ms = []
            for _ in range(a.reps + 1):
                s = build_frequencies(t, ["s"])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.materialize()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                del s
            row[path] = round(sorted(ms[1:])[len(ms[1:]) // 2], 3)
        os.environ.pop("DQ_FREQ_WAVE_COPY", None)
        report(**row)
        del t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
