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
from typing import Dict, List, Sequence

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


class ArrowScanner:
    """Scan pyarrow record batches with a ScanPlan: upload chunk k + 1 while chunk k scans."""

    def __init__(self, plan, slot_bytes: int, n_slots: int = 2, host_threads: int = 0):
        import torch

        self.plan = plan
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

        cols = [batch.column(batch.schema.get_field_index(n)) for n in self.plan.columns]
        cols = [c.combine_chunks() if hasattr(c, "combine_chunks") else c for c in cols]
        imported = [ImportedDictionaryArray(c) if pa.types.is_dictionary(c.type) else ImportedArray(c) for c in cols]
        plan_dtype = {n: dt for n, dt, _ in getattr(self.plan, "schema", [])}
        try:
            hosts = (HostColumn * max(1, len(imported)))(*[i.host for i in imported])
            views = (L.ColumnView * max(1, len(imported)))()
            L.check(self.lib.dq_upload(self.h, hosts, len(imported), views))
            dicts = {n: self._dictionary(n, i) for n, i in zip(self.plan.columns, imported)
                     if isinstance(i, ImportedDictionaryArray)}
        finally:
            for i in imported:
                i.close()
        L.check(self.lib.dq_upload_fence(self.h, self.stream))
        self._keep = []
        for k, n in enumerate(self.plan.columns):
            if n not in dicts:
                continue
            if plan_dtype.get(n) == "dict_utf8":
                views[k].offsets = dicts[n].entry_table().data_ptr()
                views[k].reserved = dicts[n].n_entries
            else:  # (on the scan's stream, after the fence: the slot's indices are there)
                col = dicts[n].decode_buffers(n, batch.num_rows, views[k].values, views[k].validity)
                self._keep.append(col)
                views[k] = col.view()
        L.check(L.lib.dq_scan(self.plan.handle, views, batch.num_rows, self.plan.chunk))
        self.plan.chunk += 1
        L.check(self.lib.dq_upload_release(self.h, self.stream))

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

    batches = list(batches)
    schema = arrow_schema(batches[0])
    # the dictionary columns this run reads as bytes are decoded on the device, per batch (ArrowScanner.scan)
    decode = dictionary_columns_to_decode(schema, analyzers)
    schema = [(n, {"dict_utf8": _decoded_dtype(batches[0], n)}.get(dt, dt) if n in decode else dt, nl)
              for n, dt, nl in schema]
    plan = ScanPlan(analyzers, schema)
    if slot_bytes <= 0:
        # (a dictionary column's narrow indices take 4 bytes per row in the slot)
        slot_bytes = max(max(b.get_total_buffer_size() * 2 + 4 * b.num_rows * len(schema) for b in batches), 1 << 20)
    sc = ArrowScanner(plan, slot_bytes, n_slots)
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
