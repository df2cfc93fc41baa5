"""String lengths on the device: string_lengths (dq_utf8_length, dq_dict_take_i32) against Python's len() of the
decoded values -- independent of the library, and equal to the kernel's rule on well-formed UTF-8 -- and the
MinLength / MaxLength analyzers, checks, states and repository on top of it.  Every comparison is exact.
Tables of at most 4097 rows, plus one value of 100 000 characters.
"""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048  # rows of one workgroup of dq_utf8_length: kStrlenRowsPerBlock (deequ_amd/csrc/dq_strlen.hip)
ROW_COUNTS = [0, 1, 63, 64, 65, TILE + 1, 2 * TILE + 1]
ALPHABET = "aZ9 é߿日本€😀𝄞"  # 1-, 2-, 3- and 4-byte code points


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd

    return deequ_amd


def mixed_values(n, seed, null_ratio=0.1, max_len=40, alphabet=ALPHABET):
    rng = random.Random(seed)
    return [None if rng.random() < null_ratio else "".join(rng.choice(alphabet) for _ in range(rng.randint(0, max_len)))
            for _ in range(n)]


def expected(values):
    """(len() of every value, 0 for None; the non-None rows)"""
    return (np.array([0 if v is None else len(v) for v in values], np.int32),
            np.array([v is not None for v in values], bool))


def read(col):
    """(int32 lengths, bool validity) of an i32 device Column."""
    n = col.n_rows
    assert col.dtype == "i32" and col.nullable
    values = col.values.cpu().numpy()[: 4 * n].view(np.int32)
    valid = np.unpackbits(col.validity.cpu().numpy(), bitorder="little")[:n].astype(bool)
    return values, valid


def check(dq, col, values):
    got, valid = read(dq.string_lengths(col))
    want, want_valid = expected(values)
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(got, want)


def raw_column(dq, name, slots, valid, large=False, lead=b"", nullable=True):
    """A utf8 / large_utf8 Column from the bytes of every slot, NULL rows' included, behind `lead` unused bytes (so the
    first offset is len(lead) and the first value starts off the data pointer's alignment)."""
    import torch

    from deequ_amd import table as T

    lens = np.array([len(b) for b in slots], np.int64)
    offs = np.full(len(slots) + 1, len(lead), np.int64)
    offs[1:] += np.cumsum(lens)
    data = np.frombuffer(lead + b"".join(slots), np.uint8)
    offs_np = offs if large else offs.astype(np.int32)
    return dq.Column(name, "large_utf8" if large else "utf8", len(slots),
                     torch.from_numpy(T._pad_u8(data, 16, 16)).cuda(),
                     torch.from_numpy(T.pack_validity(np.asarray(valid, bool))).cuda() if nullable else None,
                     torch.from_numpy(T._pad_u8(offs_np.view(np.uint8), 16, 16)).cuda(), nullable=nullable,
                     data_bytes=int(offs[-1]))


# ----------------------------------------------------------------------------------------------- string_lengths
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_nullable_mixed_code_points(dq, n):
    values = mixed_values(n, seed=n)  # lengths 0..40 of 1- to 4-byte code points, about 10 % NULL
    check(dq, dq.Table.from_pydict({"s": ("utf8", values)}).columns["s"], values)


@pytest.mark.parametrize("n", [65, TILE + 1])
def test_non_nullable_and_ascii(dq, n):
    values = mixed_values(n, seed=3, null_ratio=0.0)
    col = dq.Table.from_pydict({"s": ("utf8", values)}, nullable={"s": False}).columns["s"]
    assert col.validity is None
    check(dq, col, values)
    ascii_values = mixed_values(n, seed=4, null_ratio=0.0, alphabet="abc xyz019")
    check(dq, dq.Table.from_pydict({"s": ("utf8", ascii_values)}, nullable={"s": False}).columns["s"], ascii_values)


def test_null_slots_that_hold_bytes(dq):
    values = mixed_values(TILE + 1, seed=5, null_ratio=0.3)
    slots = ["日本語 filler".encode() if v is None else v.encode() for v in values]
    col = raw_column(dq, "s", slots, [v is not None for v in values])
    check(dq, col, values)


@pytest.mark.parametrize("n", [1, 65, TILE + 1])
def test_all_empty_strings(dq, n):
    values = [""] * n
    check(dq, dq.Table.from_pydict({"s": ("utf8", values)}).columns["s"], values)


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("before", [0, 1, 70])
def test_one_long_value_between_short_ones(dq, large, before):
    # 100 000 three-byte characters (300 000 bytes: hundreds of the wave's 1 KiB spans), behind `before` short rows, so
    # the value starts at the head, inside, and in the second 64-row group of a wave, and further short rows follow
    values = mixed_values(before, seed=6) + ["日" * 100_000] + mixed_values(70, seed=7)
    check(dq, dq.Table.from_pydict({"s": ("large_utf8" if large else "utf8", values)}).columns["s"], values)


@pytest.mark.parametrize("n", [65, TILE + 1])
def test_large_utf8(dq, n):
    values = mixed_values(n, seed=8)
    col = dq.Table.from_pydict({"s": ("large_utf8", values)}).columns["s"]
    assert col.dtype == "large_utf8"
    check(dq, col, values)


@pytest.mark.parametrize("lead", [1, 5, 16, 21])
def test_first_offset_not_zero(dq, lead):
    values = mixed_values(200, seed=9)
    slots = [b"" if v is None else v.encode() for v in values]
    col = raw_column(dq, "s", slots, [v is not None for v in values], lead=bytes([0xE6] * lead))
    assert col.values.data_ptr() % 16 == 0
    check(dq, col, values)


def test_ill_formed_bytes_match_the_host_rule(dq):
    from deequ_amd import _lib as L

    rng = np.random.default_rng(10)
    slots = [bytes(rng.integers(0, 256, rng.integers(0, 30), dtype=np.uint8)) for _ in range(TILE + 1)]
    slots[:4] = [b"\x80\x80\xbf", b"\xe6\x97", b"\xff\xffa", b"a\xe6"]
    valid = rng.random(len(slots)) > 0.1
    got, got_valid = read(dq.string_lengths(raw_column(dq, "s", slots, valid)))
    data = np.frombuffer(b"".join(slots), np.uint8)
    offs = np.zeros(len(slots) + 1, np.int64)
    offs[1:] = np.cumsum([len(b) for b in slots])
    bits = np.packbits(valid, bitorder="little")
    want = np.full(len(slots), -1, np.int32)
    assert L.lib.dq_utf8_length_host(data.ctypes.data, offs.ctypes.data, len(slots), bits.ctypes.data,
                                     want.ctypes.data) == 0
    assert np.array_equal(got_valid, valid) and np.array_equal(got, want)
    # the rule itself, in numpy: bytes that are not continuation bytes
    lead = ((data & 0xC0) != 0x80).astype(np.int64)
    rule = np.concatenate([[0], np.cumsum(lead)])
    assert np.array_equal(want, np.where(valid, rule[offs[1:]] - rule[offs[:-1]], 0))


def test_rejects_other_columns_and_types(dq):
    from deequ_amd import _lib as L

    t = dq.Table.from_pydict({"x": ("i64", [1, 2, 3])})
    with pytest.raises(TypeError):
        dq.string_lengths(t.columns["x"])
    view = t.columns["x"].view()
    assert L.lib.dq_utf8_length(L.TYPE_I64, ctypes.byref(view), 3, None, None, 0, None, None) == L.DQ_E_UNSUPPORTED
    assert b"dq_utf8_length" in L.lib.dq_last_error()
    assert L.lib.dq_utf8_length(L.TYPE_UTF8, ctypes.byref(view), -1, None, None, 0, None, None) == L.DQ_E_INVALID
    assert L.lib.dq_abi_version() == 6 and len(L.VARIANT_NAMES) == 32


# --------------------------------------------------------------------------------------------------- analyzers
N = TILE + 77


@pytest.fixture(scope="module")
def data(dq):
    s = mixed_values(N, seed=11, max_len=25)
    s[5], s[6] = "", None
    x = [(i * 7) % 11 for i in range(N)]
    f = [float(i % 13) - 3.5 for i in range(N)]
    table = dq.Table.from_pydict({"s": ("utf8", s), "x": ("i64", x), "f": ("f64", f),
                                  "nothing": ("utf8", [None] * N)})
    return table, s, x


def value(ctx, analyzer):
    return ctx.metric(analyzer).value.get()


def lens(values, keep=None):
    return [len(v) for i, v in enumerate(values) if v is not None and (keep is None or keep[i])]


def is_empty_state_failure(metric):
    from deequ_amd.metrics import EmptyStateException

    return metric.value.isFailure and isinstance(metric.value.failed, EmptyStateException)


def test_min_max_length(dq, data):
    table, s, x = data
    an = [dq.MinLength("s"), dq.MaxLength("s"), dq.MinLength("s", "x > 3"), dq.MaxLength("s", "x > 3"),
          dq.MinLength("nothing"), dq.MaxLength("s", "x > 100"), dq.Minimum("nothing")]
    ctx = dq.AnalysisRunner.onData(table).addAnalyzers(an).run()
    assert value(ctx, an[0]) == 0.0 == float(min(lens(s)))  # an empty string is present
    assert value(ctx, an[1]) == float(max(lens(s)))
    keep = np.array(x) > 3
    assert value(ctx, an[2]) == float(min(lens(s, keep))) and value(ctx, an[3]) == float(max(lens(s, keep)))
    m = ctx.metric(an[0])
    assert (m.name, m.instance, m.entity) == ("MinLength", "s", dq.Entity.Column) and isinstance(m.value.get(), float)
    assert is_empty_state_failure(ctx.metric(an[4])) and is_empty_state_failure(ctx.metric(an[5]))
    assert "MinLength(nothing,None)" in str(ctx.metric(an[4]).value.failed)
    assert list(table.columns) == ["s", "x", "f", "nothing"] and table.length_columns == {}  # nothing outlives the run
    # alone, through Analyzer.calculate
    assert dq.MaxLength("s", "x > 3").calculate(table).value.get() == float(max(lens(s, keep)))


def test_fused_with_other_analyzers(dq, data):
    from deequ_amd import runner

    table, s, _ = data
    others = [dq.Completeness("s"), dq.ApproxCountDistinct("s"), dq.Mean("f"), dq.Maximum("x")]
    length = [dq.MinLength("s"), dq.MaxLength("s")]
    both = dq.AnalysisRunner.onData(table).addAnalyzers(length + others).run()
    alone = dq.AnalysisRunner.onData(table).addAnalyzers(others).run()
    assert value(both, length[0]) == float(min(lens(s))) and value(both, length[1]) == float(max(lens(s)))
    for a in others:
        assert np.float64(value(both, a)).tobytes() == np.float64(value(alone, a)).tobytes()
    # one plan for all six, one derived column for the two length analyzers
    from deequ_amd.lengths import attach_length_columns

    attached = attach_length_columns(table, length + others)
    assert list(attached.length_columns) == ["s"] and len(attached.columns) == len(table.columns) + 1
    plan = runner.ScanPlan(length + others, attached.schema, length_columns=attached.length_columns)
    try:
        assert plan.columns.count(attached.length_columns["s"]) == 1
    finally:
        plan.close()


def test_dictionary_column_stays_encoded(dq):
    from deequ_amd.table import Dictionary

    entries = ["the longest entry, which only NULL rows point at", "ab", "日本語", "", "an unused entry, longer than the used"]
    rng = random.Random(12)
    n = TILE + 5
    indices = [None if rng.random() < 0.2 else rng.choice([1, 2, 3]) for _ in range(n)]  # (a NULL row's index is 0)
    x = [i % 9 for i in range(n)]
    table = dq.Table.from_pydict({"s": ("dict_utf8", (indices, entries)), "x": ("i64", x)})
    assert table.columns["s"].dtype == "dict_utf8"
    assert int(table.columns["s"].values.cpu().numpy()[: 4 * n].view(np.int32)[indices.index(None)]) == 0
    values = [None if i is None else entries[i] for i in indices]
    check(dq, table.columns["s"], values)
    plain = dq.Table.from_pydict({"s": ("utf8", values), "x": ("i64", x)})
    an = [dq.MinLength("s"), dq.MaxLength("s"), dq.MaxLength("s", "x < 4"), dq.Completeness("s"),
          dq.ApproxCountDistinct("s")]
    before = Dictionary.decode_calls
    got = dq.AnalysisRunner.onData(table).addAnalyzers(an).run()
    assert Dictionary.decode_calls == before
    want = dq.AnalysisRunner.onData(plain).addAnalyzers(an).run()
    for a in an:
        assert value(got, a) == value(want, a)
    assert value(got, an[0]) == 0.0 and value(got, an[1]) == 3.0


def test_dictionary_with_null_entry(dq):
    entries = ["abc", None, "日本"]
    indices = [0, 1, 2, None, 1, 2]
    col = dq.Table.from_pydict({"s": ("dict_utf8", (indices, entries))}).columns["s"]
    check(dq, col, ["abc", None, "日本", None, None, "日本"])


# ------------------------------------------------------------------------------------------ chunks and states
def _slice(dq, s, x, a, b):
    return dq.Table.from_pydict({"s": ("utf8", s[a:b]), "x": ("i64", x[a:b])})


def test_chunk_tables_equal_the_single_table(dq, data):
    _, s, x = data
    an = [dq.MinLength("s", "x > 3"), dq.MaxLength("s"), dq.Size()]
    whole = dq.AnalysisRunner.onData(_slice(dq, s, x, 0, N)).addAnalyzers(an).run()
    chunks = [_slice(dq, s, x, 0, 100), _slice(dq, s, x, 100, 101), _slice(dq, s, x, 101, N)]
    parts = dq.AnalysisRunner.onData(chunks).addAnalyzers(an).run()
    for a in an:
        assert value(parts, a) == value(whole, a)


@pytest.mark.parametrize("kind", ["memory", "files"])
def test_incremental_states(dq, data, tmp_path, kind):
    _, s, x = data
    cut = 700

    def provider(name):
        return dq.InMemoryStateProvider() if kind == "memory" else dq.HdfsStateProvider(str(tmp_path / name))

    an = [dq.MinLength("s", "x > 3"), dq.MaxLength("s"), dq.MaxLength("s", "x > 100")]
    whole = dq.AnalysisRunner.onData(_slice(dq, s, x, 0, N)).addAnalyzers(an).run()
    states_a, states_b = provider("a"), provider("b")
    dq.AnalysisRunner.onData(_slice(dq, s, x, 0, cut)).addAnalyzers(an).saveStatesWith(states_a).run()
    merged = (dq.AnalysisRunner.onData(_slice(dq, s, x, cut, N)).addAnalyzers(an).aggregateWith(states_a).run())
    dq.AnalysisRunner.onData(_slice(dq, s, x, cut, N)).addAnalyzers(an).saveStatesWith(states_b).run()
    schema = _slice(dq, s, x, 0, 1).schema
    from_states = dq.AnalysisRunner.runOnAggregatedStates(schema, an, [states_a, states_b])
    for a in an[:2]:
        assert value(merged, a) == value(whole, a) == value(from_states, a)
    for ctx in (whole, merged, from_states):
        assert is_empty_state_failure(ctx.metric(an[2]))


# ------------------------------------------------------------------------------------------------------ checks
def test_checks_and_repository(dq, data):
    table, s, x = data
    longest, keep = max(lens(s)), np.array(x) > 3
    shortest_kept = min(lens(s, keep))
    check_ = (dq.Check(dq.CheckLevel.Error, "lengths")
              .hasMaxLength("s", lambda v: v <= longest)
              .hasMaxLength("s", lambda v: v <= longest - 1)
              .hasMinLength("s", lambda v: v == shortest_kept).where("x > 3")
              .hasMinLength("s", lambda v: v == 0))
    repository, key = dq.InMemoryMetricsRepository(), dq.ResultKey(7, {"set": "lengths"})
    result = dq.VerificationSuite().onData(table).addCheck(check_).useRepository(repository).saveOrAppendResult(key).run()
    statuses = [r.status for r in result.checkResults[check_].constraintResults]
    ok, bad = dq.ConstraintStatus.Success, dq.ConstraintStatus.Failure
    assert statuses == [ok, bad, ok, ok]
    names = [str(r.constraint) for r in result.checkResults[check_].constraintResults]
    assert names[0] == "MaxLengthConstraint(MaxLength(s,None))"
    assert names[2] == "MinLengthConstraint(MinLength(s,Some(x > 3)))"
    stored = repository.loadByKey(key)
    for a in (dq.MaxLength("s"), dq.MinLength("s"), dq.MinLength("s", "x > 3")):
        assert stored.metric(a) == result.metrics[a] and stored.metric(a).value.isSuccess
    # stored results are recognised: nothing is computed again
    again = (dq.AnalysisRunner.onData(table).addAnalyzers([dq.MaxLength("s"), dq.MinLength("s")])
             .useRepository(repository).reuseExistingResultsForKey(key, failIfResultsMissing=True).run())
    assert value(again, dq.MaxLength("s")) == float(longest)
