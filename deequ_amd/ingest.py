"""Host-resident Arrow batches -> the fused GPU scan (libdqscan dq_arrow_import / dq_upload*).

The data path of a JVM-free drop-in: record batches arrive through the Arrow C Data Interface (Spark's
Arrow export, pyarrow, arrow-rs), are mapped without copying to host column buffers
(dq_arrow_import), copied by CPU threads into a pinned staging slot and DMA'd into a device slot on the
uploader's own stream (dq_upload), while the previous chunk scans (dq_upload_fence / dq_upload_release
order the plan's stream against the slot).  Reference seam: AnalysisRunner.runScanningAnalyzers'
data.agg over the DataFrame (analyzers/runners/AnalysisRunner.scala:279-326).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

from . import _lib as L

_FORMAT_DTYPE = {"g": "f64", "l": "i64", "i": "i32", "u": "utf8", "U": "large_utf8", "f": "f32", "s": "i16",
                 "c": "i8", "b": "bool", "tdD": "date32"}  # + "tsu:<tz>" -> timestamp, "d:p,s" -> decimal(p,s)


class ArrowSchemaC(ctypes.Structure):
    pass


class ArrowArrayC(ctypes.Structure):
    pass


ArrowSchemaC._fields_ = [("format", ctypes.c_char_p), ("name", ctypes.c_char_p), ("metadata", ctypes.c_char_p),
                         ("flags", ctypes.c_int64), ("n_children", ctypes.c_int64),
                         ("children", ctypes.POINTER(ctypes.POINTER(ArrowSchemaC))),
                         ("dictionary", ctypes.POINTER(ArrowSchemaC)),
                         ("release", ctypes.CFUNCTYPE(None, ctypes.POINTER(ArrowSchemaC))),
                         ("private_data", ctypes.c_void_p)]
ArrowArrayC._fields_ = [("length", ctypes.c_int64), ("null_count", ctypes.c_int64), ("offset", ctypes.c_int64),
                        ("n_buffers", ctypes.c_int64), ("n_children", ctypes.c_int64),
                        ("buffers", ctypes.POINTER(ctypes.c_void_p)),
                        ("children", ctypes.POINTER(ctypes.POINTER(ArrowArrayC))),
                        ("dictionary", ctypes.POINTER(ArrowArrayC)),
                        ("release", ctypes.CFUNCTYPE(None, ctypes.POINTER(ArrowArrayC))),
                        ("private_data", ctypes.c_void_p)]


class HostColumn(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("nullable", ctypes.c_int32), ("n_rows", ctypes.c_int64),
                ("values", ctypes.c_void_p), ("validity", ctypes.c_void_p), ("offsets", ctypes.c_void_p),
                ("value_bytes", ctypes.c_int64), ("validity_bytes", ctypes.c_int64), ("offset_bytes", ctypes.c_int64),
                ("offset_base", ctypes.c_int64), ("validity_bit", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class UploadDest(ctypes.Structure):
    """dq_upload_dest: the buffers of one destination column of dq_upload_to and their whole sizes."""
    _fields_ = [("values", ctypes.c_void_p), ("validity", ctypes.c_void_p), ("offsets", ctypes.c_void_p),
                ("value_bytes", ctypes.c_int64), ("validity_bytes", ctypes.c_int64), ("offset_bytes", ctypes.c_int64)]


def _bind():
    lib = L.lib
    if getattr(lib, "_dq_ingest_bound", False):
        return lib
    P = ctypes.POINTER
    lib.dq_arrow_import.restype = ctypes.c_int32
    lib.dq_arrow_import.argtypes = [P(ArrowSchemaC), P(ArrowArrayC), P(HostColumn)]
    lib.dq_arrow_import_dictionary.restype = ctypes.c_int32
    lib.dq_arrow_import_dictionary.argtypes = [P(ArrowSchemaC), P(ArrowArrayC), P(HostColumn), P(HostColumn)]
    lib.dq_uploader_create.restype = ctypes.c_int32
    lib.dq_uploader_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                       P(ctypes.c_void_p)]
    lib.dq_upload.restype = ctypes.c_int32
    lib.dq_upload.argtypes = [ctypes.c_void_p, P(HostColumn), ctypes.c_int32, P(L.ColumnView)]
    for f in ("dq_upload_fence", "dq_upload_release"):
        getattr(lib, f).restype = ctypes.c_int32
        getattr(lib, f).argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.dq_upload_sync.restype = ctypes.c_int32
    lib.dq_upload_sync.argtypes = [ctypes.c_void_p]
    lib.dq_uploader_destroy.restype = None
    lib.dq_uploader_destroy.argtypes = [ctypes.c_void_p]
    lib.dq_upload_payload.restype = ctypes.c_int32
    lib.dq_upload_payload.argtypes = [P(HostColumn), ctypes.c_int32, P(ctypes.c_int64)]
    lib.dq_upload_stage.restype = ctypes.c_int32
    lib.dq_upload_stage.argtypes = [P(HostColumn), ctypes.c_int32, P(UploadDest), ctypes.c_void_p, ctypes.c_int64,
                                    ctypes.c_int32, P(ctypes.c_int64), P(ctypes.c_int64)]
    lib.dq_upload_to.restype = ctypes.c_int32
    lib.dq_upload_to.argtypes = [ctypes.c_void_p, P(HostColumn), ctypes.c_int32, P(UploadDest)]
    lib._dq_ingest_bound = True
    return lib


class ImportedArray:
    """One pyarrow array exported through the C Data Interface and mapped by dq_arrow_import; the
    exported structures are released by close() (the pyarrow array must outlive the upload)."""

    def __init__(self, arr):
        lib = _bind()
        self._arr = arr
        self.c_array, self.c_schema = ArrowArrayC(), ArrowSchemaC()
        arr._export_to_c(ctypes.addressof(self.c_array), ctypes.addressof(self.c_schema))
        self.host = HostColumn()
        st = lib.dq_arrow_import(ctypes.byref(self.c_schema), ctypes.byref(self.c_array), ctypes.byref(self.host))
        if st != L.DQ_OK:
            self.close()
            L.check(st)

    def close(self):
        for s in (self.c_array, self.c_schema):
            if s.release:
                s.release(ctypes.byref(s))


class ImportedDictionaryArray:
    """One dictionary-encoded pyarrow array mapped by dq_arrow_import_dictionary: `host` is the index column as
    dq_upload takes it (narrow indices are widened to int32 and range-checked in its copy loop), `dictionary` the
    entries' string column, `key` what tells one dictionary from another without reading it: its buffer addresses,
    offset, length and null count."""

    def __init__(self, arr):
        lib = _bind()
        self._arr = arr
        self.c_array, self.c_schema = ArrowArrayC(), ArrowSchemaC()
        arr._export_to_c(ctypes.addressof(self.c_array), ctypes.addressof(self.c_schema))
        self.host, self.dictionary = HostColumn(), HostColumn()
        st = lib.dq_arrow_import_dictionary(ctypes.byref(self.c_schema), ctypes.byref(self.c_array),
                                            ctypes.byref(self.host), ctypes.byref(self.dictionary))
        if st != L.DQ_OK:
            self.close()
            L.check(st)
        d = self.c_array.dictionary.contents
        self.key = (tuple(d.buffers[k] for k in range(d.n_buffers)), d.offset, d.length, d.null_count)

    close = ImportedArray.close


def _device_dictionary(host: HostColumn, device):
    """A table.Dictionary on `device` from the host column of a dictionary's entries (its slice rebased)."""
    import numpy as np
    import torch

    from . import table as T

    n, large = host.n_rows, host.type == L.TYPE_LARGE_UTF8
    ot = np.int64 if large else np.int32
    offs = np.zeros(n + 1, dtype=ot)
    if n:
        offs = np.frombuffer(ctypes.string_at(host.offsets, host.offset_bytes), dtype=ot) - ot(host.offset_base)
    data = np.frombuffer(ctypes.string_at(host.values, host.value_bytes), dtype=np.uint8) if host.value_bytes else \
        np.zeros(0, np.uint8)
    valid = None
    if host.validity:
        nb = (host.validity_bit + n + 7) // 8
        bits = np.unpackbits(np.frombuffer(ctypes.string_at(host.validity, nb), dtype=np.uint8), bitorder="little")
        valid = bits[host.validity_bit:host.validity_bit + n].astype(bool)
    dev = torch.device("cuda", device)
    col = T.Column("dictionary", "large_utf8" if large else "utf8", n,
                   torch.from_numpy(T._pad_u8(data, 16, 16)).to(dev),
                   None if valid is None else torch.from_numpy(T.pack_validity(valid)).to(dev),
                   torch.from_numpy(T._pad_u8(np.ascontiguousarray(offs).view(np.uint8), 16, 16)).to(dev),
                   nullable=valid is not None, data_bytes=int(host.value_bytes))
    return T.Dictionary(col)


def arrow_schema(batch) -> List[tuple]:
    """(name, dtype, nullable) of a pyarrow RecordBatch / Table for ScanPlan."""
    import pyarrow as pa

    out = []
    for f in batch.schema:
        dt = {pa.float64(): "f64", pa.int64(): "i64", pa.int32(): "i32", pa.string(): "utf8",
              pa.large_string(): "large_utf8", pa.float32(): "f32", pa.int16(): "i16", pa.int8(): "i8",
              pa.bool_(): "bool", pa.date32(): "date32"}.get(f.type)
        if dt is None and pa.types.is_timestamp(f.type) and f.type.unit == "us":
            dt = "timestamp"
        if dt is None and pa.types.is_dictionary(f.type) and f.type.value_type in (pa.string(), pa.large_string()) \
                and f.type.index_type in (pa.int8(), pa.int16(), pa.int32(), pa.uint8(), pa.uint16()):
            dt = "dict_utf8"
        if dt is None and pa.types.is_decimal128(f.type) and 1 <= f.type.precision <= 38 and 0 <= f.type.scale:
            dt = f"decimal({f.type.precision},{f.type.scale})"
        if dt is None:
            raise TypeError(f"column {f.name}: Arrow type {f.type} is not a GPU column type")
        out.append((f.name, dt, f.nullable))
    return out


def is_arrow(obj) -> bool:
    """A pyarrow RecordBatch / Table / RecordBatchReader, or a non-empty list / tuple of record batches (decided by
    the objects' module, so pyarrow is not imported for data that is not Arrow)."""
    def one(o):
        return type(o).__module__.split(".")[0] == "pyarrow"

    return one(obj) or (isinstance(obj, (list, tuple)) and len(obj) > 0 and all(one(o) for o in obj))


def _record_batches(obj):
    """The record batches of any Arrow shape, in order (an iterator: a reader is read as it is consumed)."""
    import pyarrow as pa

    def empty(schema):
        return pa.RecordBatch.from_arrays([pa.array([], type=f.type) for f in schema], schema=schema)

    if isinstance(obj, pa.RecordBatch):
        return iter([obj])
    if isinstance(obj, pa.Table):
        return iter(obj.to_batches() or [empty(obj.schema)])
    if isinstance(obj, pa.RecordBatchReader):
        return iter(obj)
    if isinstance(obj, (list, tuple)) and obj and all(isinstance(b, pa.RecordBatch) for b in obj):
        return iter(obj)
    raise TypeError("Arrow data is a pyarrow RecordBatch, Table, RecordBatchReader or a non-empty sequence of "
                    f"RecordBatches, not {type(obj).__name__}")


def _padded(nbytes: int) -> int:
    """table._pad_u8(_, 16, 16): rounded up to 16, plus 16."""
    return (nbytes + 15) // 16 * 16 + 16


def _bitmap_bytes(n: int) -> int:
    """table.pack_validity: the rows' bytes in whole 64-bit words, plus one word."""
    return ((n + 7) // 8 + 7) // 8 * 8 + 8


class ArrowTableBuilder:
    """Arrow record batches -> device Tables that own their buffers (dq_upload_to): each batch's columns are staged
    by CPU threads into a pinned slot and DMA'd on the uploader's stream straight into the torch tensors the Columns
    hold, batch k + 1 staged while batch k is in flight.  The Columns equal, byte for byte and in their padding, those
    Table.from_pydict builds for the same values.  Consecutive batches that share an Arrow dictionary (by
    ImportedDictionaryArray.key) share one table.Dictionary; `dictionary_uploads` counts the dictionaries uploaded."""

    def __init__(self, device="cuda", n_slots: int = 2, host_threads: int = 0):
        import torch

        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"Arrow data is uploaded to a GPU, not to {dev}")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.lib = _bind()
        self.n_slots, self.host_threads = n_slots, host_threads
        self.h = None
        self.slot_bytes = 0
        self._dicts: Dict[str, tuple] = {}  # column -> (ImportedDictionaryArray.key, table.Dictionary)
        self.dictionary_uploads = 0
        self._pending = False               # an upload no stream has been ordered behind yet

    def _uploader(self, need: int):
        if self.h is not None and need <= self.slot_bytes:
            return
        if self.h is not None:  # a larger batch than any before: drain, then a larger pair of slots
            L.check(self.lib.dq_upload_sync(self.h))
            self._pending = False
            self.lib.dq_uploader_destroy(self.h)
            self.h = None
        self.slot_bytes = max(need + need // 4, 1 << 20)
        h = ctypes.c_void_p()
        L.check(self.lib.dq_uploader_create(self.device.index, self.n_slots, self.slot_bytes, self.host_threads,
                                            ctypes.byref(h)))
        self.h = h

    def add(self, batch):
        """One record batch as a Table.  The upload is in flight when this returns: finish() orders the current
        stream behind it."""
        import pyarrow as pa
        import torch

        from . import table as T

        schema = arrow_schema(batch)  # (TypeError for a type outside the GPU columns, before anything is uploaded)
        n = batch.num_rows
        imported, names, specs = [], [], []  # specs: (kind, column name, dtype, nullable, host column, null count)
        try:
            for k, (name, dtype, nullable) in enumerate(schema):
                arr = batch.column(k)
                im = ImportedDictionaryArray(arr) if dtype == "dict_utf8" else ImportedArray(arr)
                imported.append(im)
                specs.append(("column", name, dtype, nullable, im.host, arr.null_count, im))
                names.append(name)
            for kind, name, dtype, nullable, host, nulls, im in list(specs):
                have = self._dicts.get(name)
                if dtype == "dict_utf8" and (have is None or have[0] != im.key):  # a new dictionary: its entries too
                    large = im.dictionary.type == L.TYPE_LARGE_UTF8
                    specs.append(("dictionary", name, "large_utf8" if large else "utf8", True, im.dictionary,
                                  im._arr.dictionary.null_count, im))
                    names.append(name + ".dictionary")
            hosts = (HostColumn * max(1, len(specs)))(*[s[4] for s in specs])
            payload = (ctypes.c_int64 * max(1, len(specs)))()
            self._check(self.lib.dq_upload_payload(hosts, len(specs), payload), names)
            dests = (UploadDest * max(1, len(specs)))()
            columns, need = [], 0
            with torch.cuda.device(self.device):
                for k, (kind, name, dtype, nullable, host, nulls, im) in enumerate(specs):
                    rows = host.n_rows
                    string = dtype in ("utf8", "large_utf8")
                    if dtype == "bool":
                        vbytes = _padded(_bitmap_bytes(rows))
                    elif dtype == "dict_utf8":
                        vbytes = _padded(4 * rows)
                    else:
                        vbytes = _padded(payload[k])
                    buf = [torch.empty(vbytes, dtype=torch.uint8, device=self.device),
                           torch.empty(_bitmap_bytes(rows), dtype=torch.uint8, device=self.device) if nullable else None,
                           torch.empty(_padded((rows + 1) * (8 if dtype == "large_utf8" else 4)), dtype=torch.uint8,
                                       device=self.device) if string else None]
                    d = dests[k]
                    d.values, d.value_bytes = buf[0].data_ptr(), buf[0].numel()
                    if buf[1] is not None:
                        d.validity, d.validity_bytes = buf[1].data_ptr(), buf[1].numel()
                    if buf[2] is not None:
                        d.offsets, d.offset_bytes = buf[2].data_ptr(), buf[2].numel()
                    need += sum((b.numel() + 255) // 256 * 256 for b in buf if b is not None)
                    columns.append(T.Column(name, dtype, rows, buf[0], buf[1], buf[2], nullable=nullable,
                                            data_bytes=int(payload[k]) if string else 0,
                                            null_count=int(nulls) if nullable else 0))
                self._uploader(need)
                # the tensors may reuse memory that work already queued on the current stream still reads: let it
                # finish before the copy stream writes them (a no-op for an idle stream; the uploads themselves are
                # never waited for here)
                torch.cuda.current_stream().synchronize()
                self._check(self.lib.dq_upload_to(self.h, hosts, len(specs), dests), names)
            self._pending = True
        finally:
            for im in imported:
                im.close()
        out = []
        for (kind, name, dtype, nullable, host, nulls, im), col in zip(specs, columns):
            if kind == "dictionary":
                self._dicts[name] = (im.key, T.Dictionary(col))
                self.dictionary_uploads += 1
            else:
                out.append(col)
        for col in out:
            if col.dtype == "dict_utf8":
                col.dictionary = self._dicts[col.name][1]
        return T.Table(out) if out else _empty_table(n)

    @staticmethod
    def _check(status: int, names) -> None:
        """DQ_E_INVALID of the upload -> ValueError naming the column (the message names the row)."""
        import re

        if status == L.DQ_OK:
            return
        message = L.lib.dq_last_error().decode("utf-8", "replace")
        if status != L.DQ_E_INVALID:
            raise L.DQError(status, message)
        m = re.search(r"column (\d+): ", message)
        if m:
            message = f"column {names[int(m.group(1))]!r}: {message[m.end():]}"
        raise ValueError(message)

    def finish(self) -> None:
        """Order the current torch stream behind every upload so far (dq_upload_fence: the copy stream runs in order,
        so the last upload's event covers them all)."""
        import torch

        if self._pending:
            with torch.cuda.device(self.device):
                L.check(self.lib.dq_upload_fence(self.h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            self._pending = False

    def close(self) -> None:
        if self.h is not None:
            self.lib.dq_uploader_destroy(self.h)  # (waits for the copy stream)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _empty_table(n: int):
    from . import table as T

    t = T.Table([])
    t.num_rows = n
    return t


def tables_from_arrow(obj, device="cuda", builder: Optional[ArrowTableBuilder] = None) -> List:
    """One device Table per record batch of `obj` -- a pyarrow RecordBatch, a Table (one per batch of to_batches()), a
    sequence of RecordBatches or a RecordBatchReader -- in order: a chunk list for every runner.  Types outside
    arrow_schema's raise TypeError naming the column before anything is uploaded; a dictionary index outside its
    dictionary or a decimal outside its precision raises ValueError naming column and row."""
    batches = _record_batches(obj)
    first = next(batches, None)
    if first is None:
        raise ValueError("Arrow data without a record batch")
    arrow_schema(first)  # (a refused type: before a device is touched)
    own = builder is None
    b = ArrowTableBuilder(device) if own else builder
    try:
        out = [b.add(first)]
        for batch in batches:
            if batch.schema != first.schema:
                raise ValueError("the record batches differ in schema")
            out.append(b.add(batch))
        b.finish()
        return out
    finally:
        if own:
            b.close()


def table_from_arrow(obj, device="cuda", builder: Optional[ArrowTableBuilder] = None):
    """Table.from_arrow: the batches of `obj` as ONE Table (several batches are concatenated on the host, by Arrow,
    dictionaries unified, and uploaded as one)."""
    import pyarrow as pa

    batches = list(_record_batches(obj))
    if not batches:
        raise ValueError("Arrow data without a record batch")
    arrow_schema(batches[0])
    if len(batches) > 1:
        batches = list(_record_batches(pa.Table.from_batches(batches).combine_chunks()))
    return tables_from_arrow(batches[0], device, builder)[0]


class _SlotBuffer:
    """A device address inside an upload slot, with the two members of a tensor that Column.view(), lengths and
    expressions read; it owns nothing."""

    def __init__(self, address: int, device):
        self._address, self.device = address, device

    def data_ptr(self) -> int:
        return self._address


class ArrowScanner:
    """Scan pyarrow record batches with a ScanPlan: upload chunk k + 1 while chunk k scans."""

    def __init__(self, plan, slot_bytes: int, n_slots: int = 2, host_threads: int = 0,
                 length_columns: Optional[dict] = None, expressions: Optional[dict] = None):
        """length_columns: source string column -> the derived length column the plan reads (MinLength / MaxLength);
        expressions: derived column -> the expressions.Expression it holds (arithmetic operands).  Both are built per
        batch on the scan's stream from the slot's columns, which are uploaded for them."""
        import torch

        self.plan = plan
        self.length_columns = dict(length_columns or {})
        self.expressions = dict(expressions or {})
        derived = set(self.length_columns.values()) | set(self.expressions)
        # what a batch uploads: the plan's own columns, then the sources the derived columns are computed from
        self.upload_columns = [n for n in plan.columns if n not in derived]
        for n in list(self.length_columns) + [c for e in self.expressions.values() for c in e.columns]:
            if n not in self.upload_columns:
                self.upload_columns.append(n)
        self.source_schema = {n: (dt, nl) for n, dt, nl in getattr(plan, "schema", [])}
        self.lib = _bind()
        h = ctypes.c_void_p()
        L.check(self.lib.dq_uploader_create(plan.device, n_slots, slot_bytes, host_threads, ctypes.byref(h)))
        self.h = h
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(plan.device).cuda_stream)
        # per dictionary column: (ImportedDictionaryArray.key, table.Dictionary) of the previous batch -- consecutive
        # batches sharing a dictionary reuse its device buffers and its entry table
        self._dicts: Dict[str, tuple] = {}
        self.dictionary_uploads = 0  # dictionaries uploaded (one dq_dict_entries pass each, on the fast path)
        self._keep: List = []        # decoded columns of the batch in flight

    def _dictionary(self, name: str, im: "ImportedDictionaryArray"):
        have = self._dicts.get(name)
        if have is None or have[0] != im.key:
            have = (im.key, _device_dictionary(im.dictionary, self.plan.device))
            self._dicts[name] = have
            self.dictionary_uploads += 1
        return have[1]

    def scan(self, batch) -> None:
        """Upload one batch (its columns in the plan's order) and enqueue its scan.  A dictionary-encoded column
        uploads its indices only; the plan reads it as dict_utf8 (entry table) or, where the plan's schema says
        utf8 / large_utf8 (the run reads its bytes), as the column decoded on the device."""
        import pyarrow as pa

        names = self.upload_columns
        cols = [batch.column(batch.schema.get_field_index(n)) for n in names]
        cols = [c.combine_chunks() if hasattr(c, "combine_chunks") else c for c in cols]
        imported = [ImportedDictionaryArray(c) if pa.types.is_dictionary(c.type) else ImportedArray(c) for c in cols]
        plan_dtype = {n: dt for n, dt, _ in getattr(self.plan, "schema", [])}
        try:
            hosts = (HostColumn * max(1, len(imported)))(*[i.host for i in imported])
            views = (L.ColumnView * max(1, len(imported)))()
            L.check(self.lib.dq_upload(self.h, hosts, len(imported), views))
            dicts = {n: self._dictionary(n, i) for n, i in zip(names, imported)
                     if isinstance(i, ImportedDictionaryArray)}
        finally:
            for i in imported:
                i.close()
        L.check(self.lib.dq_upload_fence(self.h, self.stream))
        self._keep = []
        decoded = {}
        for k, n in enumerate(names):
            if n not in dicts:
                continue
            if plan_dtype.get(n) == "dict_utf8":
                views[k].offsets = dicts[n].entry_table().data_ptr()
                views[k].reserved = dicts[n].n_entries
            elif n in plan_dtype:  # (on the scan's stream, after the fence: the slot's indices are there)
                col = dicts[n].decode_buffers(n, batch.num_rows, views[k].values, views[k].validity)
                self._keep.append(col)
                decoded[n] = col
                views[k] = col.view()
        by_name = {n: views[k] for k, n in enumerate(names)}
        if self.length_columns or self.expressions:
            by_name.update(self._derive(batch.num_rows, names, views, dicts, decoded))
        scan_views = (L.ColumnView * max(1, len(self.plan.columns)))(*[by_name[n] for n in self.plan.columns])
        L.check(L.lib.dq_scan(self.plan.handle, scan_views, batch.num_rows, self.plan.chunk))
        self.plan.chunk += 1
        L.check(self.lib.dq_upload_release(self.h, self.stream))

    def _derive(self, n_rows: int, names, views, dicts, decoded) -> Dict[str, L.ColumnView]:
        """The views of the batch's derived columns: a Table over the slot's column views (it owns none of them),
        lengths.string_lengths / expressions.evaluate on the scan's stream, the results kept until the next batch."""
        import torch

        from . import table as T
        from .expressions import evaluate
        from .lengths import string_lengths

        dev = torch.device("cuda", self.plan.device)
        cols = []
        for k, n in enumerate(names):
            if n in decoded:
                cols.append(decoded[n])
                continue
            dtype, nullable = self.source_schema[n]
            v = views[k]
            ptr = [None if a is None else _SlotBuffer(a, dev) for a in (v.values, v.validity, v.offsets)]
            cols.append(T.Column(n, dtype, n_rows, ptr[0], ptr[1], None if dtype == "dict_utf8" else ptr[2],
                                 nullable=nullable, dictionary=dicts.get(n)))
        slot = T.Table(cols)
        out = {}
        with torch.cuda.device(dev):
            for src, name in self.length_columns.items():
                col = string_lengths(slot.columns[src])
                col.name = name
                self._keep.append(col)
                out[name] = col.view()
            for name, e in self.expressions.items():
                col = evaluate(e, slot, name)
                self._keep.append(col)
                out[name] = col.view()
        return out

    def close(self) -> None:
        if self.h:
            self.lib.dq_uploader_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scan_arrow(batches: Sequence, analyzers, slot_bytes: int = 0, n_slots: int = 2) -> List[L.State]:
    """Fused scan of host-resident Arrow record batches -> raw aggregation-result slot sets."""
    from .runner import ScanPlan

    from .runner import dictionary_columns_to_decode

    from .expressions import _merge, analyzer_expressions, derived_schema
    from .lengths import STRING_DTYPES, length_column_name, length_columns_needed

    batches = list(batches)
    schema = arrow_schema(batches[0])
    # the dictionary columns this run reads as bytes are decoded on the device, per batch (ArrowScanner.scan)
    decode = dictionary_columns_to_decode(schema, analyzers)
    schema = [(n, {"dict_utf8": _decoded_dtype(batches[0], n)}.get(dt, dt) if n in decode else dt, nl)
              for n, dt, nl in schema]
    # the derived columns of the run, named as attach_length_columns / attach_expression_columns name them for Tables:
    # one i32 length column per string column under MinLength / MaxLength, one column per distinct arithmetic operand;
    # ArrowScanner builds them per batch from the slot
    dtype_of = {n: dt for n, dt, _ in schema}
    lengths: Dict[str, str] = {}
    for c in length_columns_needed(analyzers):
        if dtype_of.get(c) in STRING_DTYPES:
            lengths[c] = length_column_name(c, [n for n, _, _ in schema])
            schema.append((lengths[c], "i32", True))
    exprs = _merge(analyzer_expressions(analyzers, schema))
    schema, expr_names = derived_schema(exprs, schema)
    plan = ScanPlan(analyzers, schema, length_columns=lengths, expr_columns=expr_names)
    if slot_bytes <= 0:
        # (a dictionary column's narrow indices take 4 bytes per row in the slot)
        slot_bytes = max(max(b.get_total_buffer_size() * 2 + 4 * b.num_rows * len(schema) for b in batches), 1 << 20)
    sc = ArrowScanner(plan, slot_bytes, n_slots, length_columns=lengths,
                      expressions={expr_names[t]: e for t, e in exprs.items()})
    try:
        for b in batches:
            sc.scan(b)
        return plan.finish()
    finally:
        sc.close()
        plan.close()


def _decoded_dtype(batch, name: str) -> str:
    import pyarrow as pa

    return "large_utf8" if batch.schema.field(name).type.value_type == pa.large_string() else "utf8"


def host_columns(batch) -> Dict[str, HostColumn]:
    """dq_arrow_import of every column of a batch (host only; for tests / diagnostics); a dictionary-encoded
    column's entry is its index column, its entries' column is under name + ".dictionary"."""
    import pyarrow as pa

    out = {}
    for f in batch.schema:
        arr = batch.column(batch.schema.get_field_index(f.name))
        arr = arr.combine_chunks() if hasattr(arr, "combine_chunks") else arr
        if pa.types.is_dictionary(f.type):
            im = ImportedDictionaryArray(arr)
            out[f.name + ".dictionary"] = im.dictionary
        else:
            im = ImportedArray(arr)
        out[f.name] = im.host
        im.close()
    return out
