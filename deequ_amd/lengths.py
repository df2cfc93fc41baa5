"""String lengths on the device: length(col) of a string column as a derived i32 column, and the derived columns a
run of MinLength / MaxLength analyzers reads.

Spark computes min(length(col)) / max(length(col)) as a derived expression under an ordinary aggregate; here
dq_utf8_length (include/dqscan.h) materialises the derived column -- as casts.cast_column does for the profiler's
numeric-string cast -- and the analyzers lower to DQ_OP_MIN / DQ_OP_MAX over it, inside the run's one fused plan.
A dictionary-encoded column is not decoded: the lengths of its dictionary's entries are computed once and
dq_dict_take_i32 gathers them through the indices.  There is no host fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterable, Sequence, Union

from . import _lib as L
from .analyzers import Preconditions, _ColumnAnalyzer
from .metrics import UnsupportedOnGpuPathException
from .table import Column, Dictionary, Table

STRING_DTYPES = ("utf8", "large_utf8", "dict_utf8")


class _LengthAnalyzer(_ColumnAnalyzer):
    """min / max of length(column) (Deequ 1.0.3 MinLength.scala / MaxLength.scala): DQ_OP_MIN / DQ_OP_MAX over the
    derived i32 length column the runner attaches for the run, with the analyzer's own `where`; the states are
    MinState / MaxState."""
    numeric = False

    def additionalPreconditions(self):
        return [Preconditions.hasColumn(self.column), Preconditions.isString(self.column)]

    def _lower(self, b):
        where = b.pred(self.where)  # (first: a `where` outside the GPU grammar is a routing decision)
        return (self.OP, b.length_col(self.column), -1, -1, where)


class MinLength(_LengthAnalyzer):
    name = "MinLength"
    OP = L.OP_MIN


class MaxLength(_LengthAnalyzer):
    name = "MaxLength"
    OP = L.OP_MAX


def _check(status: int) -> None:
    try:
        L.check(status)
    except L.DQError as e:
        if e.status == L.DQ_E_UNSUPPORTED:
            raise UnsupportedOnGpuPathException(e.message) from e
        raise


def _buffers(n: int, dev):
    """An i32 column's buffers, padded as table.column_from_numpy pads them (values: 4 n bytes rounded up to 16, + 16;
    validity: whole 64-bit words + 1).  The kernels write every value and every validity word of the n rows: only the
    padding is cleared."""
    import torch

    words = (n + 63) // 64
    values = torch.empty(max(16, (4 * n + 15) // 16 * 16 + 16), dtype=torch.uint8, device=dev)
    validity = torch.empty((words + 1) * 8, dtype=torch.uint8, device=dev)
    values[4 * n:].zero_()
    validity[8 * words:].zero_()
    return values, validity


def _where(dev):
    import torch

    index = dev.index if dev.index is not None else torch.cuda.current_device()
    return index, torch.cuda.current_stream(dev).cuda_stream


def _plain_lengths(col: Column, name: str):
    """(i32 Column of col's lengths, its NULL rows) for a utf8 / large_utf8 column."""
    n = col.n_rows
    dev = col.values.device
    values, validity = _buffers(n, dev)
    view = col.view()
    if not col.nullable:
        view.validity = None
    nulls = ctypes.c_int64(0)
    index, stream = _where(dev)
    _check(L.lib.dq_utf8_length(col.type_code, ctypes.byref(view), n, values.data_ptr(), validity.data_ptr(), index,
                                stream, ctypes.byref(nulls)))
    return Column(name, "i32", n, values, validity, None, nullable=True), nulls.value


def _entry_lengths(d: Dictionary):
    """int32[n_entries] on the device: the length of every entry of a dictionary, -1 for a NULL entry (what
    dq_dict_take_i32 reads as a NULL row).  Computed once per dictionary and kept with it, as its entry table is."""
    import torch

    if getattr(d, "_entry_lengths", None) is None:
        col, nulls = _plain_lengths(d.entries, d.entries.name)
        lengths = col.values[: 4 * d.n_entries].view(torch.int32)
        if nulls:
            bits = (col.validity[: (d.n_entries + 7) // 8, None] >> torch.arange(8, device=lengths.device)) & 1
            lengths = torch.where(bits.reshape(-1)[: d.n_entries].bool(), lengths, torch.full_like(lengths, -1))
        if d.n_entries == 0:
            lengths = torch.zeros(4, dtype=torch.int32, device=col.values.device)
        d._entry_lengths = lengths.contiguous()
    return d._entry_lengths


def string_lengths(col: Column) -> Column:
    """length(col) of a utf8 / large_utf8 / dict_utf8 column: a new nullable i32 Column of the same name and length,
    NULL where the source row is NULL.  The length of a value is its number of code points (include/dqscan.h
    dq_utf8_length states the rule for ill-formed bytes).  A dict_utf8 column is not decoded."""
    if col.dtype not in STRING_DTYPES:
        raise TypeError(f"string_lengths: column {col.name!r} is {col.dtype}, not a string column")
    if col.dtype != "dict_utf8":
        return _plain_lengths(col, col.name)[0]
    n = col.n_rows
    dev = col.values.device
    entries = _entry_lengths(col.dictionary)
    values, validity = _buffers(n, dev)
    view = L.ColumnView()
    view.values = col.values.data_ptr()
    view.validity = col.validity.data_ptr() if col.validity is not None and col.nullable else None
    index, stream = _where(dev)
    _check(L.lib.dq_dict_take_i32(ctypes.byref(view), n, entries.data_ptr(), col.dictionary.n_entries,
                                  values.data_ptr(), validity.data_ptr(), index, stream))
    return Column(col.name, "i32", n, values, validity, None, nullable=True)


# ------------------------------------------------------------------------------------------ the runner's side
def length_column_name(column: str, taken: Iterable[str]) -> str:
    """The name of the derived length column of `column`: "length(column)", with underscores in front until no
    column of the data carries it (a `where` can only name columns of the data, so it cannot name this one)."""
    taken = set(taken)
    name = f"length({column})"
    while name in taken:
        name = "_" + name
    return name


def length_columns_needed(analyzers: Sequence) -> list:
    """The source columns the MinLength / MaxLength analyzers among `analyzers` name, in first-use order."""
    return list(dict.fromkeys(a.column for a in analyzers if isinstance(a, _LengthAnalyzer)))


def attach_length_columns(data: Union[Table, Sequence[Table]], analyzers: Sequence):
    """`data` (a Table or a list of chunk Tables) with one derived length column attached to every chunk for each
    string column a MinLength / MaxLength of `analyzers` names -- one per source column, however many analyzers and
    `where`s read it -- as new Tables that share the chunks' columns; Table.length_columns maps source to derived
    name.  Columns that are missing or not strings are left to the analyzers' preconditions.  Data whose tables
    already carry the columns, or a run without such an analyzer, comes back as it is."""
    wanted = length_columns_needed(analyzers)
    if not wanted:
        return data
    chunks = [data] if isinstance(data, Table) else list(data)
    if not chunks:
        return data
    first = chunks[0]
    todo = [c for c in wanted if c not in first.length_columns and c in first.columns
            and first.columns[c].dtype in STRING_DTYPES]
    if not todo:
        return data
    names: Dict[str, str] = dict(first.length_columns)
    taken = set(first.columns)
    for c in todo:
        names[c] = length_column_name(c, taken)
        taken.add(names[c])

    def one(t: Table) -> Table:
        derived = []
        for c in todo:
            col = string_lengths(t.columns[c])
            col.name = names[c]
            derived.append(col)
        out = Table(list(t.columns.values()) + derived)
        out.length_columns = dict(names)
        out.expr_columns = dict(t.expr_columns)
        return out

    return one(data) if isinstance(data, Table) else [one(t) for t in chunks]


def length_columns_of(data) -> Dict[str, str]:
    """source column -> derived length column of attached data ({} for data as the user built it)."""
    chunks = [data] if isinstance(data, Table) else list(data)
    return dict(chunks[0].length_columns) if chunks else {}
