"""HBM-resident columnar tables (Arrow physical layout) handed to the scan.

A Column owns device buffers (torch CUDA/HIP tensors are used purely as device allocations):
values (f64 / f32 / i64 / i32 / i16 / i8 / date32 / timestamp, decimal(p,s) as 16-byte two's-complement unscaled
integers, bit-packed bool, or UTF-8 bytes), an optional LSB-first validity bitmap, and int32
(utf8) / int64 (large_utf8) offsets.  Buffers are allocated with the padding dqscan.h requires:
values 16-byte aligned, bitmaps readable in whole 32-bit words, UTF-8 data readable up to the
next 4-byte boundary past the last string.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

DTYPES = {"f64": L.TYPE_F64, "i64": L.TYPE_I64, "i32": L.TYPE_I32, "utf8": L.TYPE_UTF8,
          "large_utf8": L.TYPE_LARGE_UTF8, "f32": L.TYPE_F32, "i16": L.TYPE_I16, "i8": L.TYPE_I8,
          "bool": L.TYPE_BOOL, "date32": L.TYPE_DATE32, "timestamp": L.TYPE_TIMESTAMP,
          "dict_utf8": L.TYPE_DICT_UTF8}
# Preconditions.isNumeric (Analyzer.scala:322-334): ByteType .. DoubleType, and DecimalType ("decimal(p,s)")
NUMERIC = ("f64", "i64", "i32", "f32", "i16", "i8")


def decimal_ps(dtype: str) -> Optional[Tuple[int, int]]:
    """(precision, scale) of a "decimal(p,s)" dtype (DecimalType(p, s)), else None."""
    if not dtype.startswith("decimal(") or not dtype.endswith(")"):
        return None
    p, s = dtype[8:-1].split(",")
    return int(p), int(s)


def is_numeric(dtype: str) -> bool:
    return dtype in NUMERIC or decimal_ps(dtype) is not None


def type_code(dtype: str) -> int:
    ps = decimal_ps(dtype)
    return L.decimal_type(*ps) if ps else DTYPES[dtype]


def decimal_unscaled(v, scale: int) -> int:
    """A value as the unscaled integer of DecimalType(_, scale): an int is taken as the value itself, a
    decimal.Decimal / str / float through its exact decimal value, rounded HALF_UP to the scale (Spark's
    Decimal.changePrecision)."""
    import decimal

    d = v if isinstance(v, decimal.Decimal) else decimal.Decimal(str(v) if isinstance(v, float) else v)
    return int((d.scaleb(scale)).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_UP))
# fixed-width physical layouts (bool: bit-packed values; date32: int32 days since 1970-01-01; timestamp: int64 us)
_NP = {"f64": np.float64, "i64": np.int64, "i32": np.int32, "f32": np.float32, "i16": np.int16, "i8": np.int8,
       "date32": np.int32, "timestamp": np.int64}
FIXED = tuple(_NP) + ("bool",)


def _torch():
    import torch

    return torch


def _pad_u8(a: np.ndarray, mult: int, extra: int = 0) -> np.ndarray:
    n = len(a)
    total = ((n + mult - 1) // mult) * mult + extra
    out = np.zeros(max(total, mult), dtype=np.uint8)
    out[:n] = a
    return out


def pack_validity(valid: np.ndarray) -> np.ndarray:
    """bool[n] -> Arrow LSB-first bitmap padded to whole 64-bit words (+1 word)."""
    bits = np.packbits(np.asarray(valid, dtype=bool), bitorder="little")
    return _pad_u8(bits, 8, 8)


@dataclass
class Column:
    name: str
    dtype: str
    n_rows: int
    values: object                 # torch tensor on the device
    validity: Optional[object]     # torch uint8 tensor or None (no nulls)
    offsets: Optional[object] = None
    nullable: bool = True
    data_bytes: int = 0            # UTF-8 payload bytes (for traffic accounting)
    dictionary: Optional["Dictionary"] = None  # dict_utf8: values = int32 indices into it
    null_count: Optional[int] = None  # NULL rows, where the constructor knew them (from_pydict, from_arrow)

    def view(self) -> L.ColumnView:
        v = L.ColumnView()
        if self.dtype == "dict_utf8":  # dqscan.h: indices, their bitmap, the entry words, the number of entries
            v.values = self.values.data_ptr()
            v.validity = self.validity.data_ptr() if self.validity is not None else None
            v.offsets = self.dictionary.entry_table().data_ptr()
            v.reserved = self.dictionary.n_entries
            return v
        v.values = self.values.data_ptr() if self.values is not None else None
        v.validity = self.validity.data_ptr() if self.validity is not None else None
        v.offsets = self.offsets.data_ptr() if self.offsets is not None else None
        v.reserved = 0
        return v

    @property
    def type_code(self) -> int:
        return type_code(self.dtype)


class Dictionary:
    """The strings a dict_utf8 column's indices refer to: a device utf8 / large_utf8 Column of n_entries entries (an
    entry may be NULL), shared by every column and chunk that uses it.  The entry table (dq_dict_entries) and the
    decoded plain column of a given index column are built on first use and kept."""

    entries_calls = 0  # dq_dict_entries launches of the process (tests count them)
    decode_calls = 0   # columns decoded by the process (dq_dict_decode): a run on the indices alone adds none

    def __init__(self, entries: Column):
        if entries.dtype not in ("utf8", "large_utf8"):
            raise ValueError("a dictionary holds utf8 / large_utf8 entries")
        self.entries = entries
        self.n_entries = entries.n_rows
        self._table = None

    def entry_table(self):
        """uint32[n_entries] entry words on the device (include/dqscan.h dq_dict_entries)."""
        if self._table is None:
            import ctypes

            torch = _torch()
            dev = self.entries.values.device
            t = torch.zeros(max(4, self.n_entries), dtype=torch.int32, device=dev)
            view = self.entries.view()
            with torch.cuda.device(dev):
                L.check(L.lib.dq_dict_entries(self.entries.type_code, ctypes.byref(view), self.n_entries, t.data_ptr(),
                                              dev.index or 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            Dictionary.entries_calls += 1
            self._table = t
        return self._table

    def decode(self, col: Column) -> Column:
        """The plain utf8 / large_utf8 Column a dict_utf8 column of this dictionary stands for (dq_dict_decode)."""
        return self.decode_buffers(col.name, col.n_rows, col.values.data_ptr(),
                                   col.validity.data_ptr() if col.validity is not None else None)

    def decode_buffers(self, name: str, n: int, indices_ptr: int, validity_ptr: Optional[int]) -> Column:
        """decode() of int32 indices / validity given as device addresses (an uploaded Arrow batch's slot)."""
        import ctypes

        Dictionary.decode_calls += 1
        torch = _torch()
        dev = self.entries.values.device
        large = self.entries.dtype == "large_utf8"
        ow = 8 if large else 4
        offsets = torch.zeros(((n + 1) * ow + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
        validity = torch.zeros(((n + 63) // 64) * 8 + 8, dtype=torch.uint8, device=dev)
        dview = self.entries.view()
        iview = L.ColumnView()
        iview.values = indices_ptr
        iview.validity = validity_ptr
        need = ctypes.c_int64(0)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            args = (self.entries.type_code, ctypes.byref(dview), self.n_entries, ctypes.byref(iview), n)
            L.check(L.lib.dq_dict_decode(*args, None, 0, validity.data_ptr(), offsets.data_ptr(), ctypes.byref(need),
                                         dev.index or 0, stream))
            values = torch.zeros((need.value + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
            if n:
                L.check(L.lib.dq_dict_decode(*args, values.data_ptr(), need.value, validity.data_ptr(),
                                             offsets.data_ptr(), ctypes.byref(need), dev.index or 0, stream))
        return Column(name, self.entries.dtype, n, values, validity, offsets, nullable=True, data_bytes=need.value)


def decoded(col: Column) -> Column:
    """A dict_utf8 column as the plain string column it stands for (built once per column, then kept); any other
    column unchanged."""
    if col.dtype != "dict_utf8":
        return col
    if getattr(col, "_decoded", None) is None:
        col._decoded = col.dictionary.decode(col)
    return col._decoded


def plain_utf8(data, columns: Optional[Iterable[str]] = None):
    """`data` (a Table or a list of chunk Tables) with its dict_utf8 columns -- all, or those named -- replaced by
    their decoded plain string columns: what the consumers that read string bytes (predicates, patterns, groupings
    that are not computed on the indices, schema validation, casts, row takes) ask for.  Data without such a column
    comes back as it is."""
    names = None if columns is None else set(columns)

    def one(t: "Table") -> "Table":
        hit = [c.name for c in t.columns.values() if c.dtype == "dict_utf8" and (names is None or c.name in names)]
        if not hit:
            return t
        out = Table([decoded(c) if c.name in hit else c for c in t.columns.values()])
        out.length_columns = dict(t.length_columns)
        out.expr_columns = dict(t.expr_columns)
        return out

    return one(data) if isinstance(data, Table) else [one(t) for t in data]


class Table:
    """An ordered set of equally long device columns (the scan input of one chunk / shard)."""

    def __init__(self, columns: Sequence[Column]):
        self.columns: Dict[str, Column] = {}
        n = None
        for c in columns:
            if n is None:
                n = c.n_rows
            elif c.n_rows != n:
                raise ValueError("columns differ in length")
            self.columns[c.name] = c
        self.num_rows = n or 0
        # source string column -> its derived length column, for tables lengths.attach_length_columns built
        self.length_columns: Dict[str, str] = {}
        # canonical arithmetic expression -> its derived column, for tables expressions.attach_expression_columns built
        self.expr_columns: Dict[str, str] = {}

    @property
    def schema(self) -> List[Tuple[str, str, bool]]:
        return [(c.name, c.dtype, c.nullable) for c in self.columns.values()]

    def count(self) -> int:
        return self.num_rows

    # -------------------------------------------------------------------- construction helpers
    @staticmethod
    def from_pydict(data: Dict[str, Tuple[str, Iterable]], device: str = "cuda", nullable: Optional[Dict[str, bool]] = None) -> "Table":
        """{"att1": ("i32", [1, None, 3]), "name": ("utf8", ["a", None])} -> device Table."""
        cols = []
        for name, (dtype, vals) in data.items():
            nl = True if nullable is None else nullable.get(name, True)
            if dtype == "dict_utf8":
                # (indices, entries) as given -- entries may be unused, repeated or None, an index None for a NULL
                # row -- or a list of values, encoded in first-occurrence order
                indices, entries = vals if isinstance(vals, tuple) else encode_dictionary(vals)
                cols.append(dict_utf8_column(name, list(indices), list(entries), device=device, nullable=nl))
                continue
            vals = list(vals)
            valid = np.array([v is not None for v in vals], dtype=bool)
            if dtype == "bool":
                arr = np.array([False if v is None else bool(v) for v in vals], dtype=bool)
                cols.append(column_from_numpy(name, dtype, arr, valid, device=device, nullable=nl))
            elif dtype in FIXED:
                arr = np.array([0 if v is None else v for v in vals], dtype=_NP[dtype])
                cols.append(column_from_numpy(name, dtype, arr, valid, device=device, nullable=nl))
            elif decimal_ps(dtype):
                sc = decimal_ps(dtype)[1]
                u = [0 if v is None else decimal_unscaled(v, sc) for v in vals]
                cols.append(column_from_numpy(name, dtype, u, valid, device=device, nullable=nl))
            else:
                b = [None if v is None else (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for v in vals]
                cols.append(utf8_column(name, b, device=device, large=(dtype == "large_utf8"), nullable=nl))
        return Table(cols)

    @staticmethod
    def from_arrow(obj, device: str = "cuda") -> "Table":
        """A pyarrow RecordBatch, Table, RecordBatchReader or sequence of RecordBatches -> ONE device Table (several
        batches are concatenated), its Columns identical -- values, validity, offsets, padding -- to from_pydict's for
        the same values.  Arrow types: float64 / float32, int64 / 32 / 16 / 8, bool, date32, timestamp[us], utf8,
        large_utf8, decimal128(p <= 38, s), dictionary<int8 / 16 / 32 or uint8 / 16, utf8 or large_utf8> (dict_utf8);
        any other raises TypeError naming the column.  ingest.tables_from_arrow keeps the batches as a chunk list."""
        from .ingest import table_from_arrow

        return table_from_arrow(obj, device)


def column_from_numpy(name: str, dtype: str, values: np.ndarray, valid: Optional[np.ndarray] = None,
                      device: str = "cuda", nullable: bool = True) -> Column:
    torch = _torch()
    if dtype == "bool":  # Arrow boolean: LSB-first bit-packed values, read as whole 32-bit words
        n = len(values)
        raw = pack_validity(np.asarray(values, dtype=bool))
        raw = _pad_u8(raw, 16, 16)
    elif decimal_ps(dtype):  # Arrow decimal128: the unscaled values (Python ints) as 16-byte little-endian
        p, _ = decimal_ps(dtype)
        L.decimal_type(p, 0)  # (validates the precision)
        n = len(values)
        mask = (1 << 64) - 1
        w = np.zeros((n, 2), dtype=np.uint64)
        if n:
            u = [int(v) for v in values]
            if any(abs(v) >= 10 ** p for v in u):
                raise ValueError(f"a value exceeds the precision of {dtype}")
            w[:, 0] = [v & mask for v in u]
            w[:, 1] = [(v >> 64) & mask for v in u]
        raw = _pad_u8(w.view(np.uint8).reshape(-1), 16, 16)
    else:
        values = np.ascontiguousarray(values, dtype=_NP[dtype])
        n = len(values)
        raw = _pad_u8(values.view(np.uint8), 16, 16)
    vt = torch.from_numpy(raw).to(device)
    bt = None
    if valid is not None and nullable:
        bt = torch.from_numpy(pack_validity(valid)).to(device)
    return Column(name, dtype, n, vt, bt, None, nullable=nullable and valid is not None,
                  null_count=int(n - np.count_nonzero(valid)) if bt is not None else 0)


def utf8_column(name: str, values: Sequence[Optional[bytes]], device: str = "cuda", large: bool = False,
                nullable: bool = True) -> Column:
    torch = _torch()
    n = len(values)
    valid = np.array([v is not None for v in values], dtype=bool)
    lens = np.array([0 if v is None else len(v) for v in values], dtype=np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    if not large and offs[-1] >= 2 ** 31:
        raise ValueError("utf8 chunk exceeds 2 GiB; use large_utf8")
    data = b"".join(v for v in values if v is not None)
    raw = _pad_u8(np.frombuffer(data, dtype=np.uint8) if data else np.zeros(0, np.uint8), 16, 16)
    offs_np = offs if large else offs.astype(np.int32)
    ot = torch.from_numpy(_pad_u8(offs_np.view(np.uint8), 16, 16)).to(device)
    return Column(name, "large_utf8" if large else "utf8", n, torch.from_numpy(raw).to(device),
                  torch.from_numpy(pack_validity(valid)).to(device) if nullable else None, ot,
                  nullable=nullable, data_bytes=int(offs[-1]), null_count=int(n - valid.sum()) if nullable else 0)


def encode_dictionary(values: Iterable) -> Tuple[List[Optional[int]], List]:
    """(indices, entries) of a list of values: the distinct non-None values in first-occurrence order, None rows
    as None indices (no NULL entry)."""
    entries, seen, indices = [], {}, []
    for v in values:
        if v is not None and v not in seen:
            seen[v] = len(entries)
            entries.append(v)
        indices.append(None if v is None else seen[v])
    return indices, entries


def _as_bytes(v):
    return None if v is None else (v.encode("utf-8") if isinstance(v, str) else bytes(v))


def dict_utf8_column(name: str, indices: Sequence[Optional[int]], dictionary_values, valid: Optional[np.ndarray] = None,
                     device: str = "cuda", nullable: bool = True, large: bool = False) -> Column:
    """A dictionary-encoded string column: int32 `indices` (None: a NULL row) into `dictionary_values` -- a sequence
    of str / bytes / None entries, or a Dictionary shared with other columns and chunks.  Indices of non-NULL rows
    must lie in [0, number of entries) (ValueError otherwise: the device never sees an unchecked index)."""
    d = dictionary_values if isinstance(dictionary_values, Dictionary) else Dictionary(
        utf8_column(name, [_as_bytes(v) for v in dictionary_values], device=device, large=large))
    ok = np.array([i is not None for i in indices], dtype=bool)
    if valid is not None:
        ok &= np.asarray(valid, dtype=bool)
    idx = np.array([0 if i is None else int(i) for i in indices], dtype=np.int64)
    bad = ok & ((idx < 0) | (idx >= d.n_entries))
    if bad.any():
        r = int(np.flatnonzero(bad)[0])
        raise ValueError(f"dictionary index {int(idx[r])} at row {r} is outside the dictionary's {d.n_entries} entries")
    idx[~ok] = 0
    c = column_from_numpy(name, "i32", idx.astype(np.int32), ok, device=device, nullable=nullable)
    return Column(name, "dict_utf8", c.n_rows, c.values, c.validity, None, nullable=c.nullable, dictionary=d,
                  null_count=c.null_count)
