"""Dictionary-encoded string columns: ms per pass and GB/s of, for one logical column,
  (a) the dictionary fast path (Completeness + ApproxCountDistinct + DataType over dict_utf8: dq_dict_scan),
  (b) the same analyzers over the decoded plain UTF8 column (the utf8_hll_dtype column pass),
  (c) dq_dict_entries over the dictionary, (d) dq_dict_decode of the column.
Shape: --rows rows (default 1e8), 8..24-byte strings, 10 % NULL rows, D in --entries (default 1e1 1e3 1e5 1e7);
--runs timed runs per figure (default 3) after one warm-up, each figure printed per run.

    python tools/dict_bench.py [--rows N] [--entries D ...] [--runs K]
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

    print(f"rows {n}, {args.runs} runs per figure, device {torch.cuda.get_device_name(0)}", flush=True)
    for d in (int(x) for x in args.entries):
        entries = synth.utf8_column("c", d, 1234, 0, 8, 24, 0.0)  # d distinct 8..24-byte strings, no NULL entry
        dic = table.Dictionary(entries)
        g = torch.Generator(device="cuda").manual_seed(7)
        idx = torch.randint(0, d, (n + 16,), dtype=torch.int32, device="cuda", generator=g)
        valid = torch.rand(n, device="cuda", generator=g) >= 0.10
        bits = torch.zeros(((n + 63) // 64 + 1) * 64, dtype=torch.bool, device="cuda")
        bits[:n] = valid
        packed = (bits.view(-1, 8).to(torch.uint8) << torch.arange(8, device="cuda", dtype=torch.uint8)).sum(1).to(torch.uint8)
        col = table.Column("c", "dict_utf8", n, idx.view(torch.uint8), packed, None, nullable=True, dictionary=dic)
        ms_c = timed(lambda: (setattr(dic, "_table", None), dic.entry_table()))
        show("(c) dq_dict_entries ", d, ms_c, entries.data_bytes + 4 * d + 4 * d)
        ms_d = timed(lambda: dic.decode(col))
        plain = table.decoded(col)
        show("(d) dq_dict_decode  ", d, ms_d, 4 * n + n / 8 + 2 * (plain.data_bytes + 4 * n))
        show("(b) plain utf8 pass ", d, scan_ms(dq.Table([plain])), 4 * n + n / 8 + plain.data_bytes)
        show("(a) dictionary pass ", d, scan_ms(dq.Table([col])), 4 * n + n / 8)
        del col, plain, idx, bits, packed, dic, entries
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
