"""RowLevelSchemaValidator (schema/RowLevelSchemaValidator.scala:25-282) on the device.

A table of string columns and a declared schema -- int, decimal(p, s), timestamp(mask), or string with length bounds
and a regex -- give, per row, the three-valued SQL boolean m = toCNF(schema) (:225-281).  validRows holds the rows
whose m is TRUE, each schema column cast to its declared type (:208-223); invalidRows the rows whose NOT m is TRUE,
i.e. m is FALSE, untouched (:197-199).  A row whose m is NULL is in neither: the reference wrote the minValue clause
as `colIsNull.isNull.or(v >= min)` (:246), which is FALSE OR NULL for a NULL source, and that behaviour is kept.

dq_schema_validate (include/dqscan.h) computes both verdict bitmaps, both counts and every cast column of a chunk in
one launch; dq_take_index / dq_take_rows then compact every column of the chunk through the two bitmaps.  There is no
host fallback: a regex outside the DFA subset or a timestamp mask outside the supported subset raises
UnsupportedOnGpuPathException before anything is launched.  The session time zone is UTC.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

from . import _lib as L
from .metrics import NoSuchColumnException, UnsupportedOnGpuPathException
from .table import Column, Table, decimal_ps

_STRING = ("utf8", "large_utf8")


@dataclass(frozen=True)
class StringColumnDefinition:
    name: str
    isNullable: bool = True
    minLength: Optional[int] = None
    maxLength: Optional[int] = None
    matches: Optional[str] = None


@dataclass(frozen=True)
class IntColumnDefinition:
    name: str
    isNullable: bool = True
    minValue: Optional[int] = None
    maxValue: Optional[int] = None


@dataclass(frozen=True)
class DecimalColumnDefinition:
    name: str
    precision: int
    scale: int
    isNullable: bool = True


@dataclass(frozen=True)
class TimestampColumnDefinition:
    name: str
    mask: str
    isNullable: bool = True


ColumnDefinition = Union[StringColumnDefinition, IntColumnDefinition, DecimalColumnDefinition, TimestampColumnDefinition]


@dataclass(frozen=True)
class RowLevelSchema:
    """RowLevelSchema (:73-151): every with*Column returns a new schema with the definition appended."""
    columnDefinitions: Tuple[ColumnDefinition, ...] = field(default_factory=tuple)

    def withStringColumn(self, name: str, isNullable: bool = True, minLength: Optional[int] = None,
                         maxLength: Optional[int] = None, matches: Optional[str] = None) -> "RowLevelSchema":
        return RowLevelSchema(tuple(self.columnDefinitions) +
                              (StringColumnDefinition(name, isNullable, minLength, maxLength, matches),))

    def withIntColumn(self, name: str, isNullable: bool = True, minValue: Optional[int] = None,
                      maxValue: Optional[int] = None) -> "RowLevelSchema":
        return RowLevelSchema(tuple(self.columnDefinitions) + (IntColumnDefinition(name, isNullable, minValue, maxValue),))

    def withDecimalColumn(self, name: str, precision: int, scale: int, isNullable: bool = True) -> "RowLevelSchema":
        return RowLevelSchema(tuple(self.columnDefinitions) + (DecimalColumnDefinition(name, precision, scale, isNullable),))

    def withTimestampColumn(self, name: str, mask: str, isNullable: bool = True) -> "RowLevelSchema":
        return RowLevelSchema(tuple(self.columnDefinitions) + (TimestampColumnDefinition(name, mask, isNullable),))


@dataclass
class RowLevelSchemaValidationResult:
    """(:161-166); validRows / invalidRows are a Table, or one Table per chunk when chunks were given."""
    validRows: Union[Table, List[Table]]
    numValidRows: int
    invalidRows: Union[Table, List[Table]]
    numInvalidRows: int


def _int32(v: int, what: str) -> int:
    if not -(1 << 31) <= int(v) < (1 << 31):
        raise ValueError(f"{what} {v} is not an Int")
    return int(v)


def cast_dtype(d: ColumnDefinition) -> Optional[str]:
    """The dtype castExpression (:29, :47, :57, :66-68) gives the column in validRows; None: unchanged."""
    if isinstance(d, IntColumnDefinition):
        return "i32"
    if isinstance(d, DecimalColumnDefinition):
        return f"decimal({d.precision},{d.scale})"
    if isinstance(d, TimestampColumnDefinition):
        return "timestamp"
    return None


class SchemaPlan:
    """dq_schema_plan of a schema whose definition i reads column `positions[i]` of a chunk (host only)."""

    def __init__(self, schema: RowLevelSchema, positions: Sequence[int]):
        defs = schema.columnDefinitions
        arr = (L.SchemaColumn * max(1, len(defs)))()
        for c, d, pos in zip(arr, defs, positions):
            c.column, c.nullable = pos, 1 if d.isNullable else 0
            lo = hi = None
            if isinstance(d, StringColumnDefinition):
                c.kind, lo, hi = L.SCHEMA_STRING, d.minLength, d.maxLength
                c.text = None if d.matches is None else d.matches.encode("utf-8")
            elif isinstance(d, IntColumnDefinition):
                c.kind, lo, hi = L.SCHEMA_INT, d.minValue, d.maxValue
            elif isinstance(d, DecimalColumnDefinition):
                c.kind, c.precision, c.scale = L.SCHEMA_DECIMAL, d.precision, d.scale
            else:
                c.kind, c.text = L.SCHEMA_TIMESTAMP, d.mask.encode("utf-8")
            if lo is not None:
                c.has_min, c.min_value = 1, _int32(lo, "bound")
            if hi is not None:
                c.has_max, c.max_value = 1, _int32(hi, "bound")
        self.n_defs = len(defs)
        self.handle = ctypes.c_void_p()
        try:
            L.check(L.lib.dq_schema_plan_create(arr, len(defs), ctypes.byref(self.handle)))
        except L.DQError as e:
            if e.status == L.DQ_E_UNSUPPORTED:
                raise UnsupportedOnGpuPathException(e.message) from e
            raise

    def close(self) -> None:
        if self.handle:
            L.lib.dq_schema_plan_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        self.close()


def _round16(n: int) -> int:
    return (n + 15) // 16 * 16


def _device_args(dev):
    import torch

    index = dev.index if dev.index is not None else torch.cuda.current_device()
    return index, torch.cuda.current_stream(dev).cuda_stream


def _view(col: Column) -> L.ColumnView:
    v = col.view()
    if not col.nullable:
        v.validity = None
    return v


def take_index(selection, n_rows: int, n_selected: int):
    """The rows a selection bitmap (device uint8 tensor of whole 64-bit words) holds, in order: a device int64 tensor."""
    import torch

    index = torch.empty(max(1, n_selected), dtype=torch.int64, device=selection.device)
    dev, stream = _device_args(selection.device)
    L.check(L.lib.dq_take_index(selection.data_ptr(), n_rows, n_selected, index.data_ptr(), dev, stream))
    return index


def take_column(col: Column, index, n_selected: int) -> Column:
    """The rows `index` lists of a column, as a new Column with the padding table.py gives every buffer: values
    16-byte aligned with a cleared tail, bitmaps in whole 64-bit words plus one, string data readable to the next
    4-byte boundary."""
    import torch

    dev = col.values.device
    d, stream = _device_args(dev)
    n, words = n_selected, (n_selected + 63) // 64
    view = _view(col)
    keep_validity = col.nullable and col.validity is not None
    validity = torch.zeros((words + 1) * 8, dtype=torch.uint8, device=dev) if keep_validity else None
    vptr = validity.data_ptr() if keep_validity else None
    nbytes = ctypes.c_int64(0)
    if col.dtype in _STRING:
        width = 8 if col.dtype == "large_utf8" else 4
        offsets = torch.zeros(_round16((n + 1) * width) + 16, dtype=torch.uint8, device=dev)
        # the sizing call (offsets and the byte count), then the copy into a buffer of that size
        L.check(L.lib.dq_take_rows(col.type_code, ctypes.byref(view), col.n_rows, index.data_ptr(), n, None, 0, vptr,
                                   offsets.data_ptr(), ctypes.byref(nbytes), d, stream))
        total = nbytes.value
        values = torch.zeros(max(16, _round16(total) + 16), dtype=torch.uint8, device=dev)
        if total:
            L.check(L.lib.dq_take_rows(col.type_code, ctypes.byref(view), col.n_rows, index.data_ptr(), n,
                                       values.data_ptr(), total, None, offsets.data_ptr(), ctypes.byref(nbytes), d, stream))
        return Column(col.name, col.dtype, n, values, validity, offsets, nullable=keep_validity, data_bytes=total)
    if col.dtype == "bool":
        need = words * 8
        values = torch.zeros(_round16((words + 1) * 8) + 16, dtype=torch.uint8, device=dev)
    else:
        width = 16 if decimal_ps(col.dtype) else {"f64": 8, "i64": 8, "timestamp": 8, "i32": 4, "f32": 4, "date32": 4,
                                                  "i16": 2, "i8": 1}[col.dtype]
        need = width * n
        values = torch.zeros(max(16, _round16(need) + 16), dtype=torch.uint8, device=dev)
    L.check(L.lib.dq_take_rows(col.type_code, ctypes.byref(view), col.n_rows, index.data_ptr(), n, values.data_ptr(), need,
                               vptr, None, ctypes.byref(nbytes), d, stream))
    return Column(col.name, col.dtype, n, values, validity, None, nullable=keep_validity)


def take_rows(table: Table, selection, n_selected: int) -> Table:
    """Every column of a table compacted through one selection bitmap (the index is built once)."""
    index = take_index(selection, table.num_rows, n_selected)
    return Table([take_column(c, index, n_selected) for c in table.columns.values()])


@dataclass
class ChunkVerdict:
    """What the verdict pass leaves of one chunk: the TRUE / FALSE bitmaps (device uint8 tensors of whole 64-bit
    words plus one), their popcounts, and the cast columns (full length) by column name."""
    valid: object
    invalid: object
    num_valid: int
    num_invalid: int
    casts: dict


class RowLevelSchemaValidator:
    """RowLevelSchemaValidator (:169-282)."""

    @staticmethod
    def _positions(table: Table, schema: RowLevelSchema) -> List[int]:
        names = list(table.columns)
        out = []
        for d in schema.columnDefinitions:
            if d.name not in table.columns:
                raise NoSuchColumnException(f"Input data does not include column {d.name}!")
            if table.columns[d.name].dtype not in _STRING:
                raise UnsupportedOnGpuPathException(
                    f"schema column {d.name} is {table.columns[d.name].dtype}: the validator reads string columns")
            out.append(names.index(d.name))
        return out

    @staticmethod
    def verdict(table: Table, schema: RowLevelSchema, plan: Optional[SchemaPlan] = None) -> ChunkVerdict:
        """The verdict pass over one chunk (dq_schema_validate): bitmaps, counts and cast columns."""
        import torch

        own = plan is None
        if own:
            plan = SchemaPlan(schema, RowLevelSchemaValidator._positions(table, schema))
        try:
            n, words = table.num_rows, (table.num_rows + 63) // 64
            cols = list(table.columns.values())
            dev = cols[0].values.device if cols else torch.device("cuda", torch.cuda.current_device())
            d, stream = _device_args(dev)
            valid = torch.empty((words + 1) * 8, dtype=torch.uint8, device=dev)
            invalid = torch.empty((words + 1) * 8, dtype=torch.uint8, device=dev)
            valid[words * 8:].zero_()
            invalid[words * 8:].zero_()
            types = (ctypes.c_int32 * max(1, len(cols)))(*[c.type_code for c in cols])
            views = (L.ColumnView * max(1, len(cols)))(*[_view(c) for c in cols])
            nd = plan.n_defs
            cvals = (ctypes.c_void_p * max(1, nd))()
            cbits = (ctypes.c_void_p * max(1, nd))()
            casts = {}
            for i, df in enumerate(schema.columnDefinitions):
                to = cast_dtype(df)
                if to is None:
                    continue
                width = {"i32": 4, "timestamp": 8}.get(to, 16)
                # (the pass writes every value and validity word of the n rows: only the padding is cleared)
                v = torch.empty(max(16, _round16(width * n) + 16), dtype=torch.uint8, device=dev)
                b = torch.empty((words + 1) * 8, dtype=torch.uint8, device=dev)
                v[width * n:].zero_()
                b[words * 8:].zero_()
                cvals[i], cbits[i] = v.data_ptr(), b.data_ptr()
                casts[df.name] = Column(df.name, to, n, v, b, None, nullable=True)  # (a later definition wins: toMap)
            nv, ni = ctypes.c_int64(0), ctypes.c_int64(0)
            L.check(L.lib.dq_schema_validate(plan.handle, types, views, len(cols), n, valid.data_ptr(), invalid.data_ptr(),
                                             cvals, cbits, d, stream, ctypes.byref(nv), ctypes.byref(ni)))
            return ChunkVerdict(valid, invalid, nv.value, ni.value, casts)
        finally:
            if own:
                plan.close()

    @staticmethod
    def validate(data: Union[Table, Sequence[Table]], schema: RowLevelSchema) -> RowLevelSchemaValidationResult:
        """validate (:183-206).  `data`: a Table, or a sequence of chunk Tables of one layout, validated chunk by
        chunk (the result tables are then lists, one Table per chunk)."""
        from .table import plain_utf8

        from .runner import arrow_data

        data = plain_utf8(arrow_data(data))  # (dictionary-encoded string columns: read as the plain columns they stand for)
        single = isinstance(data, Table)
        chunks = [data] if single else list(data)
        if not chunks:
            raise ValueError("RowLevelSchemaValidator.validate: no chunks")
        # every refusal comes before the first launch
        positions = [RowLevelSchemaValidator._positions(t, schema) for t in chunks]
        if any(p != positions[0] or list(t.columns) != list(chunks[0].columns) for p, t in zip(positions, chunks)):
            raise ValueError("RowLevelSchemaValidator.validate: the chunks differ in their columns")
        plan = SchemaPlan(schema, positions[0])
        try:
            valid_tables, invalid_tables, nv, ni = [], [], 0, 0
            for t in chunks:
                v = RowLevelSchemaValidator.verdict(t, schema, plan)
                # extractAndCastValidRows (:208-223): the data's column order, schema columns through their cast
                projected = Table([v.casts.get(c.name, c) for c in t.columns.values()])
                valid_tables.append(take_rows(projected, v.valid, v.num_valid))
                invalid_tables.append(take_rows(t, v.invalid, v.num_invalid))
                nv += v.num_valid
                ni += v.num_invalid
        finally:
            plan.close()
        if single:
            return RowLevelSchemaValidationResult(valid_tables[0], nv, invalid_tables[0], ni)
        return RowLevelSchemaValidationResult(valid_tables, nv, invalid_tables, ni)
