"""Dictionary-encoded string columns: ms per pass and GB/s of, for one logical column,
  (a) the dictionary fast path (Completeness + ApproxCountDistinct + DataType over dict_utf8: dq_dict_scan),
  (b) the same analyzers over the decoded plain UTF8 column (the utf8_hll_dtype column pass),
  (c) dq_dict_entries over the dictionary, (d) dq_dict_decode of the column.
Shape: --rows rows (default 1e8), 8..24-byte strings, 10 % NULL rows, D in --entries (default 1e1 1e3 1e5 1e7);
--runs timed runs per figure (default 3) after one warm-up, each figure printed per run.

--grouping adds the grouping leg, D in --group-entries (default 1e1 1e3 4096 1e5) on a column of the same shape:
  (e) build_frequencies / Uniqueness / Histogram of the dict_utf8 column (dq_dict_count + dq_freq_build_weighted),
  (f) the same three over the decoded column, the decode included (the route before the index path: dq_dict_decode +
      dq_freq_build), and (f') dq_freq_build alone over the column already decoded,
  (g) dq_dict_count alone, as it runs ("lds" up to 4096 entries) and under DQ_DICT_COUNT_AB=global (global adds at
      every D) -- the two sides of the kernel's LDS threshold at one D.
(e) and (f) alternate run by run; each figure is a host clock around a call that ends synchronised; the two states
are compared for equality before anything is timed.

    python tools/dict_bench.py [--rows N] [--entries D ...] [--runs K] [--grouping] [--group-entries D ...]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    import deequ_amd as dq
    from deequ_amd import runner, synth, table

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--entries", type=float, nargs="*", default=[1e1, 1e3, 1e5, 1e7])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--grouping", action="store_true")
    ap.add_argument("--group-entries", type=float, nargs="*", default=[1e1, 1e3, 4096, 1e5])
    args = ap.parse_args()
    n = int(args.rows)
    torch.cuda.set_device(0)

    def timed(fn):
        out = []
        for k in range(args.runs + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if k:
                out.append(a.elapsed_time(b))
        return out

    def scan_ms(t):
        an = [dq.Completeness("c"), dq.ApproxCountDistinct("c"), dq.DataType("c")]
        plan = runner.ScanPlan(an, t.schema)
        try:
            def once():
                plan.reset()
                plan.scan(t)
            ms = timed(once)
            plan.finish()
            return ms
        finally:
            plan.close()

    def show(tag, d, ms, nbytes):
        print(f"{tag} D={d:>9} " + " ".join(f"{m:9.4f} ms {nbytes / m / 1e6:8.1f} GB/s" for m in ms), flush=True)

    def column(d):
        entries = synth.utf8_column("c", d, 1234, 0, 8, 24, 0.0)  # d distinct 8..24-byte strings, no NULL entry
        dic = table.Dictionary(entries)
        g = torch.Generator(device="cuda").manual_seed(7)
        idx = torch.randint(0, d, (n + 16,), dtype=torch.int32, device="cuda", generator=g)
        valid = torch.rand(n, device="cuda", generator=g) >= 0.10
        bits = torch.zeros(((n + 63) // 64 + 1) * 64, dtype=torch.bool, device="cuda")
        bits[:n] = valid
        packed = (bits.view(-1, 8).to(torch.uint8) << torch.arange(8, device="cuda", dtype=torch.uint8)).sum(1).to(torch.uint8)
        del bits, valid
        return entries, dic, table.Column("c", "dict_utf8", n, idx.view(torch.uint8), packed, None, nullable=True,
                                          dictionary=dic)

    print(f"rows {n}, {args.runs} runs per figure, device {torch.cuda.get_device_name(0)}", flush=True)
    for d in (int(x) for x in args.entries):
        entries, dic, col = column(d)
        ms_c = timed(lambda: (setattr(dic, "_table", None), dic.entry_table()))
        show("(c) dq_dict_entries ", d, ms_c, entries.data_bytes + 4 * d + 4 * d)
        ms_d = timed(lambda: dic.decode(col))
        plain = table.decoded(col)
        show("(d) dq_dict_decode  ", d, ms_d, 4 * n + n / 8 + 2 * (plain.data_bytes + 4 * n))
        show("(b) plain utf8 pass ", d, scan_ms(dq.Table([plain])), 4 * n + n / 8 + plain.data_bytes)
        show("(a) dictionary pass ", d, scan_ms(dq.Table([col])), 4 * n + n / 8)
        del col, plain, dic, entries
        torch.cuda.empty_cache()
    if args.grouping:
        for d in (int(x) for x in args.group_entries):
            grouping_leg(args, n, d, *column(d)[1:])
            torch.cuda.empty_cache()


def grouping_leg(args, n, d, dic, col):
    import ctypes
    import time

    import torch

    import deequ_amd as dq
    from deequ_amd import _lib as L, table
    from deequ_amd.grouping import build_frequencies, index_path_dictionaries

    t = dq.Table([col])
    assert index_path_dictionaries([t], ["c"]) is not None

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def decoded_table():  # a fresh decode, as a run that reads the bytes pays it
        col._decoded = None
        return table.plain_utf8(t)

    plain = decoded_table()
    assert build_frequencies(t, ["c"]) == build_frequencies(plain, ["c"])
    legs = [("build_frequencies", lambda x: build_frequencies(x, ["c"])),
            ("Uniqueness       ", lambda x: dq.Uniqueness("c").calculate(x).value.get()),
            ("Histogram        ", lambda x: dq.Histogram("c").calculate(x).value.get())]
    for name, fn in legs:
        e, f, f1 = [], [], []
        for k in range(args.runs + 1):  # alternating; run 0 is the warm-up
            a = wall(lambda: fn(t))
            b = wall(lambda: fn(decoded_table()))
            c = wall(lambda: fn(plain))
            if k:
                e.append(a), f.append(b), f1.append(c)
        for tag, ms in (("(e) on indices       ", e), ("(f) decode + plain   ", f), ("(f') plain, decoded  ", f1)):
            print(f"{tag} {name} D={d:>7} " + " ".join(f"{m:9.3f} ms" for m in ms), flush=True)
    before = table.Dictionary.decode_calls
    build_frequencies(t, ["c"])
    assert table.Dictionary.decode_calls == before
    # (g) the count kernel alone, device events, the two forms alternating
    counts = torch.zeros(d, dtype=torch.int64, device="cuda")
    view = col.view()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    modes = ["lds", "global"] if d <= 4096 else ["global"]
    ms = {m: [] for m in modes}
    ref = None
    for k in range(args.runs + 1):
        for m in modes:
            os.environ["DQ_DICT_COUNT_AB"] = m
            counts.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            L.check(L.lib.dq_dict_count(ctypes.byref(view), n, counts.data_ptr(), 0, stream))
            b.record()
            torch.cuda.synchronize()
            ref = counts.clone() if ref is None else ref
            assert torch.equal(ref, counts), m
            if k:
                ms[m].append(a.elapsed_time(b))
    os.environ.pop("DQ_DICT_COUNT_AB", None)
    for m in modes:
        print(f"(g) dq_dict_count {m:<8} D={d:>7} " +
              " ".join(f"{x:9.4f} ms {(4 * n + n / 8) / x / 1e6:8.1f} GB/s" for x in ms[m]), flush=True)


if __name__ == "__main__":
    main()
