"""RowLevelSchemaValidator on the device (deequ_amd/schema.py over dq_schema_validate / dq_take_index / dq_take_rows)
against the plain-Python restatement (tests/schema_ref.py): the reference's seven cases, a mixed schema over the
adversarial pools at sizes around a validity word and a block, the minValue quirk, the stable row compaction for every
column layout, pass-through columns, chunked input and the refusals."""
import numpy as np
import pytest

from tests import schema_ref as R
from tests.test_schema_host import check_kat, kat_rows, load_kats, render

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dq():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import deequ_amd
    from deequ_amd import schema  # noqa: F401

    return deequ_amd


def to_schema(defs):
    from deequ_amd.schema import RowLevelSchema

    s = RowLevelSchema()
    for d in defs:
        if d["kind"] == "int":
            s = s.withIntColumn(d["name"], d.get("nullable", True), d.get("min"), d.get("max"))
        elif d["kind"] == "decimal":
            s = s.withDecimalColumn(d["name"], d["precision"], d["scale"], d.get("nullable", True))
        elif d["kind"] == "timestamp":
            s = s.withTimestampColumn(d["name"], d["mask"], d.get("nullable", True))
        else:
            s = s.withStringColumn(d["name"], d.get("nullable", True), d.get("min"), d.get("max"), d.get("matches"))
    return s


def to_table(columns, rows, large=(), not_nullable=()):
    from deequ_amd.table import Table, utf8_column

    return Table([utf8_column(c, [r[c] for r in rows], large=c in large, nullable=c not in not_nullable) for c in columns])


def bits_of(t, n):
    return np.unpackbits(t.cpu().numpy(), bitorder="little")[:n].astype(bool)


def column_values(col):
    """A device column as Python values (None = NULL): bytes for strings, ints for i32 / decimal / timestamp."""
    n = col.n_rows
    valid = np.ones(n, bool) if col.validity is None else bits_of(col.validity, n)
    raw = col.values.cpu().numpy()
    if col.dtype in ("utf8", "large_utf8"):
        o = col.offsets.cpu().numpy().view(np.int64 if col.dtype == "large_utf8" else np.int32)[:n + 1]
        vals = [raw[o[i]:o[i + 1]].tobytes() for i in range(n)]
    else:
        w = {"i32": 4, "timestamp": 8}.get(col.dtype, 16)
        vals = [int.from_bytes(raw[i * w:(i + 1) * w].tobytes(), "little", signed=True) for i in range(n)]
    return [v if ok else None for v, ok in zip(vals, valid)]


def table_rows(t):
    cols = {name: column_values(c) for name, c in t.columns.items()}
    return [{name: cols[name][i] for name in cols} for i in range(t.num_rows)]


def check_padding(col):
    """What table.py promises of every buffer."""
    n, words = col.n_rows, (col.n_rows + 63) // 64
    raw = col.values.cpu().numpy()
    assert col.values.data_ptr() % 16 == 0 and len(raw) % 16 == 0
    if col.validity is not None:
        v = col.validity.cpu().numpy()
        assert len(v) == (words + 1) * 8 and not v[words * 8:].any()
        assert not np.unpackbits(v, bitorder="little")[n:].any()
    if col.dtype in ("utf8", "large_utf8"):
        w = 8 if col.dtype == "large_utf8" else 4
        o = col.offsets.cpu().numpy()
        total = int(o.view(np.int64 if w == 8 else np.int32)[n])
        assert len(o) >= (n + 1) * w and not o[(n + 1) * w:].any()
        assert len(raw) >= (total + 3) // 4 * 4 and not raw[total:].any() and col.data_bytes == total
    elif col.dtype == "bool":
        assert len(raw) >= (words + 1) * 8 and not np.unpackbits(raw, bitorder="little")[n:].any()
    else:
        w = {"f64": 8, "i64": 8, "timestamp": 8, "i32": 4, "f32": 4, "date32": 4, "i16": 2, "i8": 1}.get(col.dtype, 16)
        assert len(raw) >= n * w + 16 - (n * w) % 16 and not raw[n * w:].any()


@pytest.mark.parametrize("case", load_kats(), ids=lambda c: c["lines"])
def test_reference_case(dq, case):
    from deequ_amd.schema import RowLevelSchemaValidator

    last = {d["name"]: d for d in case["schema"]}
    res = RowLevelSchemaValidator.validate(to_table(case["columns"], kat_rows(case)), to_schema(case["schema"]))
    valid = [{c: render(last.get(c), v) for c, v in r.items()} for r in table_rows(res.validRows)]
    invalid = [{c: render(None, v) for c, v in r.items()} for r in table_rows(res.invalidRows)]
    check_kat(case, valid, invalid, res.numValidRows, res.numInvalidRows)
    assert list(res.validRows.columns) == list(res.invalidRows.columns) == case["columns"]
    for name, dtype in case.get("validDtypes", {}).items():
        assert res.validRows.columns[name].dtype == dtype
    for name, dtype in case.get("invalidDtypes", {}).items():
        assert res.invalidRows.columns[name].dtype == dtype
    # every row, not only the members the reference test names
    want_valid, want_invalid = R.validate(case["schema"], case["columns"], kat_rows(case))
    assert table_rows(res.validRows) == want_valid and table_rows(res.invalidRows) == want_invalid


_MIXED = {}


def mixed(n):
    """(rows, verdicts, valid rows, invalid rows) of the restatement, computed once per size."""
    if n not in _MIXED:
        rows = R.mixed_rows(n)
        _MIXED[n] = (rows, [R.cnf(R.mixed_schema(), r) for r in rows]) + R.validate(R.mixed_schema(), R.MIXED_COLUMNS, rows)
    return _MIXED[n]


def packed(flags, n):
    out = np.zeros(((n + 63) // 64 + 1) * 8, np.uint8)
    b = np.packbits(np.array(flags, bool), bitorder="little")
    out[:len(b)] = b
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_mixed_schema(dq, n):
    """One definition per kind (`name` as large_utf8, `extra` passing through) over the adversarial pool: both
    bitmaps bit for bit with their zero tails, both counts, and the cast values of validRows as raw bytes."""
    from deequ_amd.schema import RowLevelSchemaValidator

    rows, verdicts, want_valid, want_invalid = mixed(n)
    table, schema = to_table(R.MIXED_COLUMNS, rows, large=("name",)), to_schema(R.mixed_schema())
    v = RowLevelSchemaValidator.verdict(table, schema)
    assert np.array_equal(v.valid.cpu().numpy(), packed([m is True for m in verdicts], n))
    assert np.array_equal(v.invalid.cpu().numpy(), packed([m is False for m in verdicts], n))
    assert (v.num_valid, v.num_invalid) == (verdicts.count(True), verdicts.count(False))
    res = RowLevelSchemaValidator.validate(table, schema)
    assert (res.numValidRows, res.numInvalidRows) == (len(want_valid), len(want_invalid))
    assert table_rows(res.invalidRows) == want_invalid
    assert [c.dtype for c in res.validRows.columns.values()] == ["i32", "utf8", "decimal(10,2)", "timestamp", "large_utf8"]
    got = {name: c for name, c in res.validRows.columns.items()}
    for name, w in (("id", 4), ("amount", 16), ("created", 8)):
        raw = got[name].values.cpu().numpy()
        valid = bits_of(got[name].validity, len(want_valid))
        for i, r in enumerate(want_valid):
            assert valid[i] == (r[name] is not None), (name, i)
            if name == "created":  # the value is promised inside the pinned domain only
                src = [x for x, m in zip(rows, verdicts) if m is True][i]["created"]
                if not R.timestamp_pinned(src, R.MAIN_MASK):
                    continue
            want = (0 if r[name] is None else r[name]).to_bytes(w, "little", signed=True)
            assert raw[i * w:(i + 1) * w].tobytes() == want, (name, i, r[name])
    for name in ("extra", "name"):
        assert column_values(got[name]) == [r[name] for r in want_valid]
    for t in (res.validRows, res.invalidRows):
        for c in t.columns.values():
            check_padding(c)


def test_min_value_quirk(dq):
    """:246 is `FALSE OR v >= min`: a NULL id under a minValue is UNKNOWN, in neither output."""
    from deequ_amd.schema import RowLevelSchema, RowLevelSchemaValidator

    rows = [{"id": b"5"}, {"id": None}, {"id": b"-3"}, {"id": b"7"}]
    res = RowLevelSchemaValidator.validate(to_table(["id"], rows), RowLevelSchema().withIntColumn("id", minValue=0))
    assert (res.numValidRows, res.numInvalidRows) == (2, 1) and res.numValidRows + res.numInvalidRows == len(rows) - 1
    assert column_values(res.validRows.columns["id"]) == [5, 7]
    assert column_values(res.invalidRows.columns["id"]) == [b"-3"]
    # without the bound (or with maxValue alone) the same row is valid
    res = RowLevelSchemaValidator.validate(to_table(["id"], rows), RowLevelSchema().withIntColumn("id", maxValue=6))
    assert column_values(res.validRows.columns["id"]) == [5, None, -3] and res.numInvalidRows == 1


TAKE_N = 1000  # several 256-thread blocks, a partial last word
SELECTIONS = {"none": lambda i: False, "all": lambda i: True, "alternating_words": lambda i: (i // 64) % 2 == 0}


def take_source(dq, dtype):
    from deequ_amd.table import Table, column_from_numpy, utf8_column

    rng = np.random.default_rng(3)
    valid = rng.random(TAKE_N) > 0.2
    if dtype in ("utf8", "large_utf8"):
        vals = [None if not ok else bytes(rng.integers(97, 123, int(rng.integers(0, 23))).astype(np.uint8)) for ok in valid]
        return utf8_column("c", vals, large=dtype == "large_utf8"), vals
    if dtype == "bool":
        arr = rng.random(TAKE_N) > 0.5
        return column_from_numpy("c", "bool", arr, valid), [bool(x) if ok else None for x, ok in zip(arr, valid)]
    if dtype.startswith("decimal"):
        u = [int(x) * 10 ** 20 + 7 for x in rng.integers(-10 ** 9, 10 ** 9, TAKE_N)]
        return column_from_numpy("c", dtype, u, valid), [x if ok else None for x, ok in zip(u, valid)]
    np_t = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64}[dtype]
    arr = rng.integers(np.iinfo(np_t).min, np.iinfo(np_t).max, TAKE_N).astype(np_t)
    return column_from_numpy("c", dtype, arr, valid), [int(x) if ok else None for x, ok in zip(arr, valid)]


def fixed_values(col):
    n = col.n_rows
    valid = bits_of(col.validity, n)
    raw = col.values.cpu().numpy()
    if col.dtype == "bool":
        vals = [bool(x) for x in np.unpackbits(raw, bitorder="little")[:n]]
    else:
        w = {"i8": 1, "i16": 2, "i32": 4, "i64": 8}.get(col.dtype, 16)
        vals = [int.from_bytes(raw[i * w:(i + 1) * w].tobytes(), "little", signed=True) for i in range(n)]
    return [v if ok else None for v, ok in zip(vals, valid)]


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
@pytest.mark.parametrize("dtype", ["i8", "i16", "i32", "i64", "decimal(38,4)", "bool", "utf8", "large_utf8"])
def test_take(dq, dtype, selection):
    """Widths 1, 2, 4, 8, 16, bit-packed bool and both string layouts: the selected rows in order, validity carried,
    the buffers padded as table.py pads them."""
    import torch

    from deequ_amd.schema import take_rows
    from deequ_amd.table import Table

    col, vals = take_source(dq, dtype)
    keep = np.array([SELECTIONS[selection](i) for i in range(TAKE_N)], bool)
    sel = torch.from_numpy(packed(keep, TAKE_N)).cuda()
    out = take_rows(Table([col]), sel, int(keep.sum())).columns["c"]
    assert out.n_rows == int(keep.sum()) and out.dtype == dtype
    want = [v for v, k in zip(vals, keep) if k]  # numpy's boolean indexing, in order
    assert (column_values(out) if dtype in ("utf8", "large_utf8") else fixed_values(out)) == want
    check_padding(out)


def test_take_refuses_a_wrong_count(dq):
    import torch

    from deequ_amd import _lib as L
    from deequ_amd.schema import take_index

    sel = torch.from_numpy(packed([True] * 10, 100)).cuda()
    with pytest.raises(L.DQError):
        take_index(sel, 100, 11)


def test_pass_through_and_non_nullable_columns(dq):
    """A column the schema does not name appears in both outputs; a nullable = False column has no validity buffer."""
    from deequ_amd.schema import RowLevelSchema, RowLevelSchemaValidator

    rows = [{"id": b"1", "tag": b"a"}, {"id": b"x", "tag": None}, {"id": b"3", "tag": b"c"}, {"id": b"", "tag": b"d"}]
    table = to_table(["tag", "id"], rows, not_nullable=("id",))
    assert table.columns["id"].validity is None
    res = RowLevelSchemaValidator.validate(table, RowLevelSchema().withIntColumn("id", isNullable=False))
    assert list(res.validRows.columns) == list(res.invalidRows.columns) == ["tag", "id"]
    assert table_rows(res.validRows) == [{"tag": b"a", "id": 1}, {"tag": b"c", "id": 3}]
    assert table_rows(res.invalidRows) == [{"tag": None, "id": b"x"}, {"tag": b"d", "id": b""}]
    assert res.validRows.columns["tag"].dtype == "utf8" and res.invalidRows.columns["id"].validity is None


def test_two_chunks_equal_the_concatenated_table(dq):
    from deequ_amd.schema import RowLevelSchemaValidator

    rows, _, want_valid, want_invalid = mixed(4097)
    schema = to_schema(R.mixed_schema())
    chunks = [to_table(R.MIXED_COLUMNS, rows[:1500]), to_table(R.MIXED_COLUMNS, rows[1500:])]
    res = RowLevelSchemaValidator.validate(chunks, schema)
    assert isinstance(res.validRows, list) and len(res.validRows) == len(res.invalidRows) == 2
    assert (res.numValidRows, res.numInvalidRows) == (len(want_valid), len(want_invalid))
    pinned = lambda rs: [dict(r, created=None) for r in rs]  # (timestamp values: test_mixed_schema)
    assert pinned(table_rows(res.validRows[0]) + table_rows(res.validRows[1])) == pinned(want_valid)
    assert table_rows(res.invalidRows[0]) + table_rows(res.invalidRows[1]) == want_invalid


def test_refusals_raise_before_any_launch(dq, monkeypatch):
    from deequ_amd import schema as S
    from deequ_amd.metrics import NoSuchColumnException, UnsupportedOnGpuPathException
    from deequ_amd.table import Table

    def launched(*a, **k):
        raise AssertionError("a launch was attempted")

    monkeypatch.setattr(S.RowLevelSchemaValidator, "verdict", staticmethod(launched))
    monkeypatch.setattr(S, "take_rows", launched)
    table = Table.from_pydict({"s": ("utf8", ["a", None]), "k": ("i64", [1, 2])})
    V, sch = S.RowLevelSchemaValidator, S.RowLevelSchema()
    with pytest.raises(UnsupportedOnGpuPathException):
        V.validate(table, sch.withIntColumn("k"))
    with pytest.raises(UnsupportedOnGpuPathException):
        V.validate(table, sch.withStringColumn("s", matches=r"(a)\1"))
    with pytest.raises(UnsupportedOnGpuPathException):
        V.validate(table, sch.withTimestampColumn("s", mask="yyyy-MM-dd HH:mm:ss.SSS"))
    with pytest.raises(NoSuchColumnException):
        V.validate(table, sch.withStringColumn("zz"))
