"""The HLL floor test of the numeric column scans (dq_kernels.hip hll_floor_thr / numeric_block<FLOOR>).

After a chunk, dq_finalize leaves each HLL slot's minimum accumulator register (the floor); the next chunk's
scan folds each 512-row block's rank words with min and only redoes a block exactly when a value could exceed
the floor.  The path is only taken once a floor is high (floor - 1 >= kFloorMin = 13), so every case here is a
two-chunk scan on one plan: a primer of 2^25 distinct values (~65 k per register: every register >= 12 with
probability 1 - 6e-12; the test asserts the floor it got) and a small probe chunk of values found on the CPU
with the oracle's hash:

  * rank exactly at the floor (must change nothing), rank floor + 1 in a register that stands at the floor (must
    land: the test's `>` must not be `>=`), other values one above their own register;
  * rank >= 24 (needs the hash's low word; tests/golden/hll_redo_values.json);
  * such values in a NULL row and in a row excluded by `where` (must not land), and as the only selected row of
    a 512-row block.

Registers are compared bit-exactly with the C oracle over primer + probe, with the same scan under
DQ_HLL_FLOOR=0, and -- after plan.reset() -- the probe alone must give the probe's own registers (a floor that
survived the reset would drop its low ranks).  A 1000-distinct column and an all-NULL column ride along: their
floor stays 0.

The string column `s`: the string passes do not use the floor (a variant that did was measured and dropped, DESIGN
§7), but every HLL slot gets one, so the column pins down that a string slot stays exact with a populated floor
(and would check a later string form).  It has a primer of 2^25 unique 10-byte strings and probes of 8 bytes (the short path; XXH64 of 8 bytes is hashLong of
them, so they are searched like the integers), of 26 bytes (the deferred queue; searched with the C oracle's hash)
and of 40 bytes (the rare path), plus the golden low-word strings of each length class.  A string over 28 bytes
makes its whole 512-row block take the exact rare path, so those sit in block 0 only and the decisive short and
deferred probes sit in later blocks.

What makes a case decisive: the filler value and the value lanes past the range read (0) have ranks far below the
floor (asserted), so a block holds no above-floor value but the ones placed in it; n = 1 and, at n = 4097, a full
512-row block hold a value of rank exactly floor + 1 in a register at the floor as their only such value.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from oracle import dq_oracle as O
from oracle import dq_oracle_c as C

HERE = os.path.dirname(os.path.abspath(__file__))
N_PRIMER = 1 << 25
K_FLOOR_MIN = 13  # dq_kernels.hip kFloorMin (on floor - 1)
PROBE_ROWS = [1, 63, 64, 65, 513, 4097]
KINDS = ["i64", "f64", "i32"]
F64_BASE = 0x4010000000000000  # bit patterns of finite doubles 4.0 + k ulp: outside the primer's integers


def _np_pw(h: np.ndarray):
    """(register index, pw) of hashes, vectorised: pw from the 23 rank bits of the high word (pw <= 23), else 64
    as a marker for `needs the low word` (not searched for here)."""
    idx = (h >> np.uint64(55)).astype(np.int64)
    r = ((h >> np.uint64(32)) & np.uint64(0x7FFFFF)).astype(np.int64)
    bl = np.zeros(len(h), dtype=np.int64)
    nz = r > 0
    bl[nz] = np.floor(np.log2(r[nz])).astype(np.int64) + 1  # bit length (exact: r < 2^23)
    return idx, np.where(nz, 23 - bl + 1, 64)


def _candidates(kind: str, start: int, n: int):
    """n candidate values outside the primer, as (column values, their hashes)."""
    k = np.arange(start, start + n, dtype=np.int64)
    if kind == "i64":
        v = k + (1 << 40)
        return v, O.np_xxh64_long(v)
    if kind == "f64":
        bits = k + F64_BASE
        return bits.view(np.float64), O.np_xxh64_long(bits)
    if kind == "s":  # 8 bytes 'A'..'P' from k's nibbles; XXH64 of 8 bytes = hashLong of them as a little-endian long
        b = np.empty((n, 8), dtype=np.uint8)
        for j in range(8):
            b[:, j] = 65 + ((k >> (4 * j)) & 15)
        return b.view(np.int64).reshape(n), O.np_xxh64_long(b.view(np.int64).reshape(n))
    v = (k + (1 << 26)).astype(np.int32)
    return v, O.np_xxh64_int(v)


def _s8(v) -> bytes:
    """The 8-byte string of a candidate of kind "s"."""
    return np.array([v], dtype=np.int64).tobytes()


def _str_pw(b: bytes):
    return O.hll_index_and_pw(C.lib().dqo_xxh64_bytes(b, len(b), 42))


def _str_lands(regs: np.ndarray, fmt: str, count: int, used: set):
    """`count` strings fmt % k whose rank exceeds their register of `regs` (distinct registers, none in `used`)."""
    out = []
    for k in range(1 << 22):
        b = (fmt % k).encode("ascii")
        idx, pw = _str_pw(b)
        if pw > int(regs[idx]) and idx not in used:
            out.append(b)
            used.add(idx)
            if len(out) == count:
                return out
    raise AssertionError("no string probe found")


def _str_primer():
    """2^25 unique 10-byte strings "pr" + 8 letters: (bytes padded for the oracle, int64 offsets)."""
    k = np.arange(N_PRIMER, dtype=np.int64)
    b = np.empty((N_PRIMER, 10), dtype=np.uint8)
    b[:, 0], b[:, 1] = ord("p"), ord("r")
    for j in range(8):
        b[:, 2 + j] = 97 + ((k >> (4 * j)) & 15)
    data = np.concatenate([b.reshape(-1), np.zeros(16, np.uint8)])
    return data, np.arange(N_PRIMER + 1, dtype=np.int64) * 10


def _str_oracle_regs(strs, inc):
    n = len(strs)
    lens = np.array([0 if x is None else len(x) for x in strs], dtype=np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"".join(x for x in strs if x is not None) + b"\0" * 16, dtype=np.uint8)
    bm = np.packbits(np.array([x is not None for x in strs], bool), bitorder="little")
    mk = None if inc is None else np.packbits(inc, bitorder="little")
    return C.hll_registers("large_utf8", data, offs, bm, mk, n)


def _search(kind: str, regs: np.ndarray):
    """Probe values against the primer's registers `regs`: (at_floor, lands) -- a value whose pw equals the
    floor, and 8 values with pw = regs[idx] + 1 in distinct registers, the first and the last with pw = floor + 1
    (in registers that stand at the floor)."""
    floor = int(regs.min())
    at_floor, first, rest, used = None, [], [], set()
    step = 1 << 21
    for start in range(0, 1 << 27, step):
        v, h = _candidates(kind, start, step)
        idx, pw = _np_pw(h)
        if at_floor is None:
            hit = np.nonzero(pw == floor)[0]
            if len(hit):
                at_floor = v[hit[0]]
        up = np.nonzero(pw == regs[idx].astype(np.int64) + 1)[0]
        for i in up.tolist():
            if int(idx[i]) in used:
                continue
            if len(first) < 2 and pw[i] == floor + 1:
                first.append(v[i])
                used.add(int(idx[i]))
            elif len(rest) < 8:
                rest.append(v[i])
                used.add(int(idx[i]))
        if at_floor is not None and len(first) == 2 and len(rest) >= 6:
            return at_floor, [first[0]] + rest[:6] + [first[1]]
    raise AssertionError("no probe values found")


def _primer_values(kind: str) -> np.ndarray:
    a = np.arange(N_PRIMER, dtype=np.int64)
    return a.astype(np.float64) if kind == "f64" else a.astype(np.int32) if kind == "i32" else a


def _oracle_regs(kind, values, valid, mask):
    n = len(values)
    bm = np.packbits(valid, bitorder="little")
    mk = None if mask is None else np.packbits(mask, bitorder="little")
    return C.hll_registers(kind, np.ascontiguousarray(values), None, bm, mk, n)


@pytest.fixture(scope="module")
def setup():
    """Primer table on the device, its oracle registers, and the probe values per kind (computed once)."""
    import deequ_amd as dq
    from deequ_amd.table import column_from_numpy

    with open(os.path.join(HERE, "golden", "hll_redo_values.json")) as f:
        g = json.load(f)
    low_word = {"i64": np.array([v for v in g["i64"] if v >= N_PRIMER], dtype=np.int64),
                "f64": np.array([int(b, 16) for b in g["f64_bits"]], dtype=np.uint64).view(np.float64),
                "i32": np.array([v for v in g["i32"] if v >= N_PRIMER], dtype=np.int32)}
    low_word["f64"] = low_word["f64"][np.isfinite(low_word["f64"])]
    ones = np.ones(N_PRIMER, bool)
    cols, info = [], {}
    for kind in KINDS:
        pv = _primer_values(kind)
        regs = _oracle_regs(kind, pv, ones, None)
        at_floor, lands = _search(kind, regs)
        info[kind] = {"regs": regs, "at_floor": at_floor, "lands": lands, "low_word": low_word[kind]}
        cols.append(column_from_numpy(kind, kind, pv, ones))
    # the string column: built from buffers (2^25 Python strings would take a minute)
    import torch
    from deequ_amd.table import Column, _pad_u8, pack_validity

    sdata, soffs = _str_primer()
    sregs = C.hll_registers("large_utf8", sdata, soffs, np.packbits(ones, bitorder="little"), None, N_PRIMER)
    at_floor, lands = _search("s", sregs)
    used = {_str_pw(_s8(v))[0] for v in lands}
    gs = [x.encode("ascii") for x in g["utf8"]]
    filler = next(x for x in (bytes(sdata[10 * i:10 * i + 10]) for i in range(1000)) if _str_pw(x)[1] <= 5)
    info["s"] = {"regs": sregs, "at_floor": _s8(at_floor), "lands": [_s8(v) for v in lands], "filler": filler,
                 "deferred": _str_lands(sregs, "deferred-probe-%011d", 2, used),  # 26 bytes
                 "rare": _str_lands(sregs, "rare-path-probe-string-%017d", 1, used),  # 40 bytes
                 "lw_short": [x for x in gs if 8 <= len(x) <= 23][:2],
                 "lw_deferred": [x for x in gs if 24 <= len(x) <= 28][:2], "lw_rare": [x for x in gs if len(x) > 28][:2]}
    cols.append(Column("s", "utf8", N_PRIMER, torch.from_numpy(_pad_u8(sdata[:-16], 16, 16)).cuda(),
                       torch.from_numpy(pack_validity(ones)).cuda(),  # (nullable, as the probe chunk's column is)
                       torch.from_numpy(_pad_u8(soffs.astype(np.int32).view(np.uint8), 16, 16)).cuda(), nullable=True,
                       data_bytes=int(soffs[-1])))
    lc = (np.arange(N_PRIMER, dtype=np.int64) % 1000)
    info["lc"] = {"regs": _oracle_regs("i64", lc, ones, None)}
    cols.append(column_from_numpy("lc", "i64", lc, ones))
    cols.append(column_from_numpy("nn", "i64", np.zeros(N_PRIMER, np.int64), np.zeros(N_PRIMER, bool)))
    cols.append(column_from_numpy("w", "i64", np.ones(N_PRIMER, np.int64), ones))
    return dq.Table(cols), info


def _probe(kind: str, inf: dict, n: int):
    """Probe chunk of n rows: (values, valid, where-included).  Filler rows hold 0 (a primer value)."""
    lands, lw = inf["lands"], inf["low_word"]
    dt = np.float64 if kind == "f64" else np.int32 if kind == "i32" else np.int64
    v = np.zeros(n, dtype=dt)
    valid = np.ones(n, bool)
    inc = np.ones(n, bool)
    v[0] = lands[0]  # rank floor + 1 in a register at the floor (n = 1: the block's only row)
    if n >= 63:
        v[1] = inf["at_floor"]
        v[2] = lw[0]                    # rank >= 24: the hash's low word
        v[3], valid[3] = lands[1], False  # would land, NULL
        v[4], inc[4] = lands[2], False    # would land, excluded by `where`
        v[5], valid[5] = lw[1], False
        v[6], inc[6] = lw[2], False
        v[n - 1] = lands[3]             # the range's last row
    if n >= 513:
        valid[512:] = False             # the second block: one selected row
        i = min(512 + 70, n - 1)
        v[i], valid[i] = lands[4], True
        if n > 1024:
            inc[1024:1536] = False      # a block with no where-included row but a would-land value
            v[1100], valid[1100] = lands[5], True
            v[n - 1], valid[n - 1] = lw[3], True  # a one-row tail block holding a low-word value
            valid[1536:2048] = True         # a full block whose only above-floor value has rank floor + 1
            v[1636] = lands[7]
    return v, valid, inc


def _probe_str(inf: dict, n: int, inc: np.ndarray):
    """The string column's probe rows (None = NULL), under the numeric probes' `where` rows `inc`."""
    lands = inf["lands"]
    v = [inf["filler"]] * n
    v[0] = lands[0]
    if n >= 63:
        v[1] = inf["at_floor"]
        v[2] = inf["lw_short"][0]
        v[3] = None
        v[4] = lands[2]                 # would land, excluded by `where` (inc[4])
        v[5] = inf["rare"][0]           # > 28 bytes: block 0 takes the exact rare path
        v[6] = inf["lw_deferred"][0]    # excluded by `where` (inc[6])
        v[7] = inf["lw_rare"][0]
        v[n - 1] = lands[3]
    if n >= 513:
        for i in range(512, n):
            v[i] = None                 # the second block: few selected rows, short and deferred ones
        v[min(512 + 70, n - 1)] = lands[4]
        if n > 1024:
            v[600] = inf["deferred"][0]
            v[700] = inf["lw_deferred"][1]
            v[1100] = inf["deferred"][1]  # in the block with no where-included row (inc[1024:1536])
            for i in range(1536, 2048):
                v[i] = inf["filler"]
            v[1636] = lands[7]          # the full block's only above-floor value: rank floor + 1
            v[n - 1] = inf["lw_short"][1]
    assert not inc[4:5].any() or n < 63
    return v


def _analyzers(dq, stats: bool):
    out = []
    for c in KINDS + ["lc", "nn", "s"]:
        out += [dq.ApproxCountDistinct(c), dq.ApproxCountDistinct(c, "w > 0")]
        if stats and c != "s":  # the stats + HLL instantiations (one task per column and `where`)
            out += [dq.StandardDeviation(c), dq.StandardDeviation(c, "w > 0")]
    return out


def _words(analyzers, states):
    return {a: a._from_result(s).words for a, s in zip(analyzers, states) if type(a).__name__ == "ApproxCountDistinct"}


@pytest.fixture(scope="module")
def plans(setup):
    """(analyzers, plan with the floor test, plan created under DQ_HLL_FLOOR=0) for the HLL-only and the
    stats + HLL variants."""
    import deequ_amd as dq
    from deequ_amd.runner import ScanPlan

    primer, _ = setup
    out = []
    for stats in (False, True):
        an = _analyzers(dq, stats)
        on = ScanPlan(an, primer.schema, pred_pass="interpreter")
        old = os.environ.get("DQ_HLL_FLOOR")
        os.environ["DQ_HLL_FLOOR"] = "0"
        try:
            off = ScanPlan(an, primer.schema, pred_pass="interpreter")
        finally:
            if old is None:
                del os.environ["DQ_HLL_FLOOR"]
            else:
                os.environ["DQ_HLL_FLOOR"] = old
        out.append((an, on, off))
    yield out
    for _, on, off in out:
        on.close()
        off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PROBE_ROWS)
def test_two_chunk_scan_matches_oracle(n, setup, plans):
    import deequ_amd as dq
    from deequ_amd.table import column_from_numpy, utf8_column

    primer, info = setup
    # no block holds an above-floor value but the probes: the fillers and the 0 that lanes past the range read
    for kind, h0 in (("i64", O.xxh64_long(0)), ("f64", O.xxh64_long(0)), ("i32", O.xxh64_int(0))):
        assert O.hll_index_and_pw(h0)[1] <= int(info[kind]["regs"].min())
    assert _str_pw(info["s"]["filler"])[1] <= int(info["s"]["regs"].min())
    cols, want, want_probe = [], {}, {}
    wcol = None
    for kind in KINDS:
        v, valid, inc = _probe(kind, info[kind], n)
        wcol = inc  # (the same rows for every kind)
        cols.append(column_from_numpy(kind, kind, v, valid))
        for where in (False, True):
            pr = _oracle_regs(kind, v, valid, inc if where else None)
            want_probe[(kind, where)] = pr
            want[(kind, where)] = np.maximum(info[kind]["regs"], pr)
    strs = _probe_str(info["s"], n, wcol)
    cols.append(utf8_column("s", strs))
    for where in (False, True):
        want_probe[("s", where)] = _str_oracle_regs(strs, wcol if where else None)
        want[("s", where)] = np.maximum(info["s"]["regs"], want_probe[("s", where)])
    for where in (False, True):
        want[("lc", where)] = info["lc"]["regs"]
        want_probe[("lc", where)] = _oracle_regs("i64", np.arange(n, dtype=np.int64) % 1000, np.ones(n, bool),
                                                 wcol if where else None)
        want[("nn", where)] = want_probe[("nn", where)] = np.zeros(512, np.uint8)
    cols.append(column_from_numpy("lc", "i64", np.arange(n, dtype=np.int64) % 1000, np.ones(n, bool)))
    cols.append(column_from_numpy("nn", "i64", np.zeros(n, np.int64), np.zeros(n, bool)))
    cols.append(column_from_numpy("w", "i64", wcol.astype(np.int64), np.ones(n, bool)))
    probe = dq.Table(cols)
    # the probe must be able to tell a skipped update from an applied one
    for kind in KINDS + ["s"]:
        assert (want[(kind, False)] != info[kind]["regs"]).sum() >= (1 if n < 63 else 3)
        if n >= 63:
            assert int(want[(kind, False)].max()) >= 24 and (want[(kind, True)] != want[(kind, False)]).any()

    for an, on, off in plans:
        got = {}
        for name, plan in (("on", on), ("off", off)):
            plan.reset()
            plan.scan(primer)
            first = _words(an, plan.finish())
            for a, w in first.items():
                regs = O.words_to_registers(w)
                if a.column in KINDS + ["s"]:  # the floor the probe chunk's scan reads: high enough for the floor test
                    assert regs == info[a.column]["regs"].tolist()
                    assert min(regs) - 1 >= K_FLOOR_MIN, (a, min(regs))
                else:
                    assert min(regs) == 0, a
            plan.scan(probe)
            got[name] = _words(an, plan.finish())
        for a, w in got["on"].items():
            key = (a.column, bool(a.where))
            assert w == tuple(O.registers_to_words(want[key].tolist())), (a, n)
            assert w == got["off"][a], (a, n)
        # after a reset the floors are gone: the probe alone gives the probe's own (low) registers
        on.reset()
        on.scan(probe)
        for a, w in _words(an, on.finish()).items():
            assert w == tuple(O.registers_to_words(want_probe[(a.column, bool(a.where))].tolist())), (a, n)
