"""Self-contained frequency states on the device: dq_freq_materialize (the gather of every group's representative
tuple into a store the table owns), dq_freq_merge carrying and comparing the values, the byte image
(dq_freq_to_bytes / dq_freq_from_bytes), HdfsStateProvider for the grouping analyzers, MutualInformation and
Histogram from states, and runOnAggregatedStates over all seven grouping analyzers.

Expectations come from a collections.Counter over the non-null tuples, from the reference's own numbers
(tests/golden/freq_state_kats.json: IncrementalAnalyzerTest.scala) and, for MutualInformation, from the formula of
MutualInformation.scala:32-80 evaluated with math.fsum (1e-12 relative: SURVEY.md section 0's fp64 tolerance).
Tables hold at most a few thousand rows; states are built once per column type and shared."""
from __future__ import annotations

import collections
import decimal
import json
import math
import os
import struct

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WAVE_COPY_LEN = 40  # dq_freq_store.hip kWaveCopyLen: strings at least this long are copied by the whole wave
LENGTHS = [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, WAVE_COPY_LEN - 1, WAVE_COPY_LEN, WAVE_COPY_LEN + 1,
           1003]
KINDS = {"utf8": ["utf8"], "large_utf8": ["large_utf8"], "decimal": ["decimal(20,4)"], "utf8_i32": ["utf8", "i32"],
         "f64_i64": ["f64", "i64"], "i64": ["i64"]}


@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import deequ_amd

    return deequ_amd


def _text(seed: int, length: int) -> str:
    """A deterministic ASCII string of this length, different for every seed."""
    out, x = [], seed * 2654435761 % (1 << 32) or 1
    while len(out) < length:
        x = (x * 1103515245 + 12345) % (1 << 31)
        out.append(chr(97 + x % 26))
    return "".join(out)


def _strings():
    """Every length of LENGTHS after a string of every length 0..8 (so it starts at every source alignment), and
    multi-byte UTF-8; values repeat, and every sixth row is NULL."""
    vals = []
    for pre in range(9):
        for k, n in enumerate(LENGTHS):
            vals.append(_text(1000 + pre, pre))
            vals.append(_text(pre * 100 + k, n))
    vals += ["é", "中文", "naïve \U0001F600 text", "é" * 70, "中" * 50]
    vals = vals + vals[::3] + vals[::7]
    return [None if i % 6 == 5 else v for i, v in enumerate(vals)]


def _rows(kind: str):
    """The rows (tuples, None = NULL) of a column type's table."""
    s = _strings()
    n = len(s)
    if kind in ("utf8", "large_utf8"):
        return [(v,) for v in s]
    if kind == "decimal":
        base = [decimal.Decimal(((i * 7919) % 301 - 150) * 10 ** (i % 5 * 3)) / 10000 for i in range(n)]
        base[3], base[4] = decimal.Decimal("9999999999999999.9999"), decimal.Decimal("-9999999999999999.9999")
        return [(None if i % 9 == 8 else v,) for i, v in enumerate(base)]
    if kind == "utf8_i32":
        return [(v, None if i % 11 == 10 else (i % 3) - 1) for i, v in enumerate(s)]
    if kind == "f64_i64":
        f = [float("nan") if i % 13 == 0 else (-0.0 if i % 13 == 1 else (i % 37) / 8.0) for i in range(n)]
        return [(None if i % 10 == 9 else f[i], None if i % 14 == 13 else (i % 5) * (1 << 40) - 7) for i in range(n)]
    return [(None if i % 8 == 7 else ((i * 7919) % 401 - 200) * (1 << 33),) for i in range(n)]


def _table(dq, kind, rows, chunks=1):
    types = KINDS[kind]

    def one(part):
        return dq.Table.from_pydict({f"c{c}": (t, [r[c] for r in part]) for c, t in enumerate(types)})

    if chunks == 1:
        return one(rows)
    step = (len(rows) + chunks - 1) // chunks
    return [one(rows[i:i + step]) for i in range(0, len(rows), step)]


def _cols(kind):
    return [f"c{c}" for c in range(len(KINDS[kind]))]


def _enc(dtype: str, v) -> bytes:
    """A value as the store holds it."""
    if dtype in ("utf8", "large_utf8"):
        return v.encode("utf-8")
    if dtype == "i32":
        return struct.pack("<i", v)
    if dtype == "i64":
        return struct.pack("<q", v)
    if dtype == "f64":
        return struct.pack("<d", v)
    return int(v.scaleb(4)).to_bytes(16, "little", signed=True)  # decimal(20,4)


def _dec(dtype: str, b: bytes):
    if dtype in ("utf8", "large_utf8"):
        return b.decode("utf-8")
    if dtype == "i32":
        return struct.unpack("<i", b)[0]
    if dtype == "i64":
        return struct.unpack("<q", b)[0]
    if dtype == "f64":
        return struct.unpack("<d", b)[0]
    return decimal.Decimal(int.from_bytes(b, "little", signed=True)).scaleb(-4)


def _counter(kind, rows):
    """Counter over the non-null tuples, keyed by the store's bytes (any NaN is Spark's canonical NaN)."""
    types = KINDS[kind]
    canon = [tuple(float("nan") if isinstance(v, float) and math.isnan(v) else v for v in r) for r in rows]
    return collections.Counter(tuple(_enc(t, v) for t, v in zip(types, r)) for r in canon if None not in r)


def _stored(kind, state):
    """{tuple of stored values: count} of a state's table (an unhashed table's keys are its values)."""
    keys, counts = state.frequencies.export()
    if kind == "i64":
        return {(struct.pack("<Q", int(k)),): int(c) for k, c in zip(keys, counts)}
    cols = [state.frequencies.take_values(keys, c) for c in range(len(KINDS[kind]))]
    got = {}
    for g in range(len(keys)):
        got[tuple(col[g] for col in cols)] = int(counts[g])
    assert len(got) == len(keys), "two groups hold the same tuple"
    return got


def _metrics(dq, state):
    """The five summary metrics as (success, the double's bits)."""
    out = []
    for a in (dq.Uniqueness("c0"), dq.Distinctness("c0"), dq.CountDistinct("c0"), dq.UniqueValueRatio("c0"),
              dq.Entropy("c0")):
        m = a.computeMetricFrom(state).value
        out.append((True, struct.pack("<d", m.get())) if m.isSuccess else (False, type(m.failed).__name__))
    return out


def _reload(state):
    from deequ_amd.grouping import FreqTable, FrequenciesAndNumRows

    return FrequenciesAndNumRows(FreqTable.from_bytes(state.materialize().frequencies.to_bytes()), state.numRows)


_CACHE = {}


def _state(dq, kind, part="all"):
    """The state of a part of a kind's rows, built once: "all" (three chunks), or the overlapping parts A (the first
    60 %), B (the last 60 %), and the thirds T0 T1 T2."""
    from deequ_amd.grouping import build_frequencies

    key = (kind, part)
    if key not in _CACHE:
        rows = _rows(kind)
        n = len(rows)
        sel = {"all": rows, "A": rows[:n * 6 // 10], "B": rows[n * 4 // 10:], "AB": rows[:n * 6 // 10] + rows[n * 4 // 10:],
               "T0": rows[:n // 3], "T1": rows[n // 3:2 * n // 3], "T2": rows[2 * n // 3:]}[part]
        tbl = _table(dq, kind, sel, chunks=3 if part == "all" else 1)
        _CACHE[key] = (build_frequencies(tbl, _cols(kind)), sel, tbl)
    return _CACHE[key]


@pytest.mark.parametrize("kind", list(KINDS))
def test_materialize_and_round_trip(dq, kind):
    """build (three chunks) -> materialize -> to_bytes -> from_bytes: the stored tuples and their counts are the
    Counter's; keys, counts, stored values and the five summary metrics survive the image unchanged."""
    state, rows, _ = _state(dq, kind)
    want = _counter(kind, rows)
    before = _metrics(dq, state)
    state.materialize()
    state.materialize()  # a second call is harmless
    assert state.frequencies.self_contained()
    assert _stored(kind, state) == dict(want)
    back = _reload(state)
    assert back == state
    assert back.frequencies.self_contained()
    assert _stored(kind, back) == dict(want)
    assert _metrics(dq, back) == before == _metrics(dq, state)
    assert back.frequencies.to_bytes() == state.frequencies.to_bytes()


@pytest.mark.parametrize("n_groups", [0, 1, 255, 256, 257])
def test_group_counts(dq, n_groups):
    """0, 1 and 255 / 256 / 257 groups (either side of a workgroup's 256 groups), each value twice plus NULLs."""
    from deequ_amd.grouping import build_frequencies

    vals = [f"g{i:04d}" + "x" * (i % 11) for i in range(n_groups)]
    rows = [(v,) for v in vals + [None, None] + vals[::-1]]
    state = build_frequencies(_table(dq, "utf8", rows), ["c0"])
    state.materialize()
    want = _counter("utf8", rows)
    assert len(want) == n_groups
    assert _stored("utf8", state) == dict(want)
    back = _reload(state)
    assert back == state and _stored("utf8", back) == dict(want)
    assert _metrics(dq, back) == _metrics(dq, state)
    merged = state.sum(back)
    assert _stored("utf8", merged) == {k: 2 * c for k, c in want.items()}


@pytest.mark.parametrize("kind", list(KINDS))
def test_merge_equals_union(dq, kind):
    """state(A).sum(state(B)) = state(A + B) for overlapping, unequal value sets -- directly, with both sides taken
    through a save and a load, and over three parts (IncrementalAnalyzerTest.scala:202-241); the merged table's
    stored tuples are the Counter's, and each hashes to its key."""
    from deequ_amd.grouping import build_frequencies

    (sa, ra, _), (sb, rb, _), (su, ru, _) = _state(dq, kind, "A"), _state(dq, kind, "B"), _state(dq, kind, "AB")
    assert set(_counter(kind, ra)) != set(_counter(kind, rb)) and set(_counter(kind, ra)) & set(_counter(kind, rb))
    want = _counter(kind, ru)
    for merged in (sa.sum(sb), _reload(sa).sum(_reload(sb)), _reload(sa.sum(sb))):
        assert merged == su
        assert _metrics(dq, merged) == _metrics(dq, su)
        assert merged.frequencies.self_contained()
        assert _stored(kind, merged) == dict(want)
    parts = [_state(dq, kind, p) for p in ("T0", "T1", "T2")]
    whole, rows, _ = _state(dq, kind)
    three = parts[0][0].sum(parts[1][0]).sum(parts[2][0])
    assert three == whole and _metrics(dq, three) == _metrics(dq, whole)
    assert _stored(kind, three) == dict(_counter(kind, rows))
    if kind != "i64":  # every stored tuple hashes to its key: a table of the stored tuples has the same keys
        keys, _ = three.frequencies.export()
        cols = [three.frequencies.take_values(keys, c) for c in range(len(KINDS[kind]))]
        tuples = [tuple(_dec(t, col[g]) for t, col in zip(KINDS[kind], cols)) for g in range(len(keys))]
        again = build_frequencies(_table(dq, kind, tuples), _cols(kind))
        k2, c2 = again.frequencies.export()
        assert k2.tolist() == keys.tolist() and set(c2.tolist()) == {1}


def test_merge_compares_values_exactly(dq, monkeypatch):
    """With the first hash cut to 4 bits, two materialised tables over different strings under one key must refuse
    to merge (DQ_E_UNSUPPORTED, decided by the values); two tables over the same string add their counts."""
    from deequ_amd import _lib as L
    from deequ_amd.grouping import build_frequencies

    monkeypatch.setenv("DQ_TEST_GROUP_HASH_MASK", "f")

    def single(text, times):
        s = build_frequencies(_table(dq, "utf8", [(text,)] * times), ["c0"])
        return s, int(s.frequencies.export()[0][0])

    a, key = single("value-0", 2)
    other = next(t for t in (f"value-{i}" for i in range(1, 400)) if single(t, 1)[1] == key)
    b, _ = single(other, 3)
    a.materialize()
    b.materialize()
    with pytest.raises(L.DQError) as e:
        a.sum(b)
    assert e.value.status == L.DQ_E_UNSUPPORTED and "collision" in str(e.value)
    same, _ = single("value-0", 5)
    merged = a.sum(same)
    assert _stored("utf8", merged) == {(b"value-0",): 7}


def test_reference_kats_through_state_provider(dq, tmp_path):
    """IncrementalAnalyzerTest.scala:103-147: Uniqueness("att1") and Uniqueness(["att1", "count"]) of initialData,
    deltaData and their merged states, the states going through HdfsStateProvider files; :202-241: Entropy over
    three snapshots, incrementally and at once."""
    from deequ_amd.state_provider import HdfsStateProvider

    kats = json.load(open(os.path.join(HERE, "golden", "freq_state_kats.json")))
    names = list(kats["columns"])

    def table(*tables):
        rows = [r for t in tables for r in kats["tables"][t]]
        return dq.Table.from_pydict({n: (kats["columns"][n], [r[i] for r in rows]) for i, n in enumerate(names)})

    initial, delta, more = table("initialData"), table("deltaData"), table("moreDeltaData")
    for i, case in enumerate(kats["uniqueness"]):
        an = dq.Uniqueness(case["columns"])
        p1, p2 = HdfsStateProvider(str(tmp_path / f"u{i}a")), HdfsStateProvider(str(tmp_path / f"u{i}b"))
        assert an.calculate(initial, saveStatesWith=p1).value.get() == case["initial"]
        assert an.calculate(delta, saveStatesWith=p2).value.get() == case["delta"]
        assert an.calculate(delta, aggregateWith=p1).value.get() == case["merged"]
        ctx = dq.AnalysisRunner.runOnAggregatedStates(initial.schema, [an], [p1, p2])
        assert ctx.metric(an).value.get() == case["merged"]
        assert sorted(os.listdir(tmp_path))[-1].endswith("-num_rows.bin")
    ent = dq.Entropy("att1")
    p = HdfsStateProvider(str(tmp_path / "ent"), allowOverwrite=True)
    assert ent.calculate(initial, saveStatesWith=p) == ent.calculate(initial)
    assert ent.calculate(delta, aggregateWith=p, saveStatesWith=p) == ent.calculate(table("initialData", "deltaData"))
    assert ent.calculate(more, aggregateWith=p, saveStatesWith=p) == ent.calculate(
        table("initialData", "deltaData", "moreDeltaData"))
    with open(str(tmp_path / "ent") + f"-{dq.state_provider.identifier(ent)}-num_rows.bin", "rb") as f:
        assert f.read() == (7).to_bytes(8, "big")


@pytest.mark.parametrize("dtype", ["utf8", "decimal(20,4)"])
def test_histogram_incremental(dq, tmp_path, dtype):
    """Batch 1 with saveStatesWith, batch 2 with aggregateWith: the Histogram of the concatenation (bins, counts,
    ratios, numberOfBins), with NULLs and -- for strings -- a literal "NullValue" joining them."""
    from deequ_amd.state_provider import HdfsStateProvider

    if dtype == "utf8":
        b1 = ["a", "b", None, "NullValue", "a", "été", "long " * 40]
        b2 = ["b", "c", None, None, "NullValue", "a", "long " * 40, ""]
    else:
        d = decimal.Decimal
        b1 = [d("1.5"), d("-2.25"), None, d("1.5"), d("0.0001"), d("1234567890123456.7891")]
        b2 = [d("-2.25"), None, d("3"), d("0"), d("1234567890123456.7891"), None]
    t1, t2, both = (dq.Table.from_pydict({"v": (dtype, b)}) for b in (b1, b2, b1 + b2))
    h = dq.Histogram("v")
    p = HdfsStateProvider(str(tmp_path / "h"))
    first = h.calculate(t1, saveStatesWith=p)
    assert first == h.calculate(t1)
    got = h.calculate(t2, aggregateWith=p)
    want = h.calculate(both)
    assert want.value.isSuccess and got == want
    dist = got.value.get()
    assert dist.numberOfBins == len(set(b1 + b2) - {None} | {"NullValue"})
    assert dist.values["NullValue"].absolute == (b1 + b2).count(None) + (b1 + b2).count("NullValue")
    assert h.computeMetricFrom(p.load(h).sum(dq.grouping.build_frequencies(t2, ["v"]))) == want
    top2 = dq.Histogram("v", None, 2)  # (another analyzer: its state has files of its own)
    top2.calculate(t1, saveStatesWith=p)
    assert top2.calculate(t2, aggregateWith=p) == top2.calculate(both)


def _mi_formula(rows):
    """MutualInformation.scala:32-80 over the joint counter, N = all rows."""
    joint = collections.Counter(r for r in rows if None not in r)
    if not joint:
        return None
    n = float(len(rows))
    px, py = collections.Counter(), collections.Counter()
    for (x, y), c in joint.items():
        px[x] += c
        py[y] += c
    return math.fsum((c / n) * math.log((c / n) / ((px[x] / n) * (py[y] / n))) for (x, y), c in joint.items())


def test_mutual_information_from_states(dq, tmp_path):
    from deequ_amd.state_provider import HdfsStateProvider, InMemoryStateProvider

    def table(rows):
        return dq.Table.from_pydict({"x": ("utf8", [r[0] for r in rows]), "y": ("i32", [r[1] for r in rows])})

    rows = [(None if i % 17 == 16 else f"x{(i * i) % 7}" + "y" * (i % 3), None if i % 19 == 18 else (i * 5) % 4)
            for i in range(900)]
    r1, r2 = rows[:400], rows[400:]
    mi = dq.MutualInformation("x", "y")
    want = _mi_formula(rows)
    p = HdfsStateProvider(str(tmp_path / "mi"))
    first = mi.calculate(table(r1), saveStatesWith=p).value.get()
    assert abs(first - _mi_formula(r1)) <= 1e-12 * abs(_mi_formula(r1))
    merged = mi.calculate(table(r2), aggregateWith=p).value.get()
    assert abs(merged - want) <= 1e-12 * abs(want), (merged, want)
    mem = InMemoryStateProvider()
    unsplit = mi.calculate(table(rows), saveStatesWith=mem).value.get()  # the state path on the whole table
    assert struct.pack("<d", merged) == struct.pack("<d", unsplit)
    assert abs(mi.calculate(table(rows)).value.get() - want) <= 1e-12 * abs(want)  # the one-pass path, as before
    const = [("k", i % 3) for i in range(300)]  # a constant column: no information
    assert _mi_formula(const) == 0.0
    c = mi.calculate(table(const[100:]), aggregateWith=_saved(mi, table(const[:100]))).value.get()
    assert c == 0.0
    nulls = [(None, i % 3) for i in range(50)]  # an all-NULL column: the empty-state failure
    m = mi.calculate(table(nulls), saveStatesWith=InMemoryStateProvider())
    assert m.value.isFailure and "Empty state" in str(m.value.failed)
    m = mi.calculate(table(nulls), aggregateWith=_saved(mi, table(nulls)))
    assert m.value.isFailure and "Empty state" in str(m.value.failed)


def _saved(analyzer, data):
    from deequ_amd.state_provider import InMemoryStateProvider

    p = InMemoryStateProvider()
    analyzer.calculate(data, saveStatesWith=p)
    return p


def test_run_on_aggregated_states(dq, tmp_path):
    """Two HdfsStateProviders written from two partitions: runOnAggregatedStates equals doAnalysisRun on the union
    for all seven grouping analyzers."""
    from deequ_amd.state_provider import HdfsStateProvider

    def table(rows):
        return dq.Table.from_pydict({"s": ("utf8", [r[0] for r in rows]), "k": ("i64", [r[1] for r in rows])})

    rows = [(None if i % 13 == 12 else f"s{(i * 31) % 57}" + "z" * (i % 20), None if i % 10 == 9 else (i * 7) % 5)
            for i in range(1500)]
    analyzers = [dq.Uniqueness(["s", "k"]), dq.Distinctness("s"), dq.CountDistinct("s"), dq.UniqueValueRatio(["s"]),
                 dq.Entropy("s"), dq.MutualInformation("s", "k"), dq.Histogram("s"), dq.Uniqueness("k")]
    providers = []
    for i, part in enumerate((rows[:700], rows[700:])):
        providers.append(HdfsStateProvider(str(tmp_path / f"part{i}")))
        ctx = dq.AnalysisRunner.doAnalysisRun(table(part), analyzers, saveStatesWith=providers[-1])
        assert all(m.value.isSuccess for m in ctx.allMetrics), ctx.allMetrics
    agg = dq.AnalysisRunner.runOnAggregatedStates(table(rows[:1]).schema, analyzers, providers)
    whole = dq.AnalysisRunner.doAnalysisRun(table(rows), analyzers)
    for a in analyzers:
        assert whole.metric(a).value.isSuccess, whole.metric(a)
        assert agg.metric(a) == whole.metric(a), (a, agg.metric(a), whole.metric(a))


def test_error_paths(dq, tmp_path):
    from deequ_amd import _lib as L
    from deequ_amd.grouping import FreqTable, _views, build_frequencies
    from deequ_amd.state_provider import HdfsStateProvider

    rows = [(f"v{i}",) for i in range(300)]  # all distinct: the representative rows lie in every chunk
    chunks = _table(dq, "utf8", rows, chunks=3)
    state = build_frequencies(chunks, ["c0"])
    with pytest.raises(L.DQError) as e:  # a hashed table that does not own its values has no image
        state.frequencies.to_bytes()
    assert e.value.status == L.DQ_E_STATE
    views, nrows = _views(chunks[:1], ["c0"])  # views that cannot cover the stored row ids
    assert L.lib.dq_freq_materialize(state.frequencies.handle, views, nrows, 1) == L.DQ_E_INVALID
    assert not state.frequencies.self_contained()
    an = dq.Uniqueness("c0")
    p = HdfsStateProvider(str(tmp_path / "s"))
    assert p.load(an) is None
    p.persist(an, state)
    assert state.frequencies.self_contained()
    with pytest.raises(FileExistsError):
        p.persist(an, state)
    HdfsStateProvider(str(tmp_path / "s"), allowOverwrite=True).persist(an, state)
    assert p.load(an) == state
    state.materialize()  # harmless
    image = state.frequencies.to_bytes()
    with pytest.raises(L.DQError) as e:
        FreqTable.from_bytes(image[:-8])
    assert e.value.status == L.DQ_E_STATE
    # either input without a store: the second hash decides and the output carries no values, as before
    plain = build_frequencies(chunks, ["c0"]).frequencies
    merged = plain.merged(state.frequencies)
    assert not merged.self_contained()
    assert L.lib.dq_freq_materialize(merged.handle, views, nrows, 1) == L.DQ_E_STATE
