"""Referential integrity: do the rows of one table occur among the keys of another?

"Every order.customer_id exists in customer.id", "every (country, zip) of this feed occurs in the master list": the
rule upstream Deequ expresses with ReferentialIntegrity / doesDatasetMatch and Spark users write as a left semi-join.
Here the other table's keys are a KeySet -- the self-contained frequency table of its key columns (dq_freq_build +
dq_freq_materialize), built once and reused across runs -- and the match is one dq_freq_contains_rows per chunk: a
per-row bitmap of the rows whose tuple is a group of the key set.

Semantics (include/dqscan.h): a NULL in any key column is "not contained" and still counts in the denominator (SQL
IN / semi-join); types must agree exactly, but for the offset width of string columns -- nothing is widened
implicitly (cast an i32 column before matching it against i64 keys); a `where` selects the rows that count.

Dataset match: does a row EQUAL the other table's row with the same key?  ("a migrated table against its source",
"today's snapshot against yesterday's": upstream's DataSynchronization.columnMatch / doesDatasetMatch with
matchColumnMappings.)  The other table is a KeyedRows -- its KeySet plus the payload, the compare columns gathered
into group order (payload row g belongs to key group g) -- and the match is two launches per chunk:
dq_freq_lookup_rows (the probe above, saying WHICH group a row hit) and dq_rows_match (the row's compare columns
against payload row group[r]).  Equality is null-safe (NULL equals NULL, NULL differs from any value); values compare
as grouping keys do (by their bits: every NaN the same, -0.0 and 0.0 apart; strings by length and bytes); a row whose
key is missing -- a NULL key included -- does not match and counts in the denominator.  The reference's keys must be
unique.  These semantics are this project's (the reference implementation at this version has no such analyzer);
tests/test_datamatch_gpu.py pins them.

Not done here: duplicate reference keys, a reference given as chunks or streamed, a tolerance on floats, implicit type
widening, fusing lookup and compare into one launch, probing inside the fused scan, byte images of a payload.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple, Union

from . import _lib as L
from .analyzers import Analyzer, Preconditions, _opt, data_schema
from .grouping import _TYPES, FreqTable, _gpu_type, build_frequencies
from .metrics import (DoubleMetric, Entity, NoSuchColumnException, UnsupportedOnGpuPathException,
                      WrongColumnTypeException)
from .states import NumMatchesAndCount
from .table import Table, plain_utf8

probe_calls = 0  # dq_freq_contains_rows launches of the process (tests count them, as expressions.eval_calls)
lookup_calls = 0  # dq_freq_lookup_rows launches of the process
match_calls = 0   # dq_rows_match launches of the process

MAX_MATCH_COLUMNS = 16  # dq_rows_match's n_cols limit

_STRINGS = ("utf8", "large_utf8", "dict_utf8")


def _dtype_of(code: int) -> str:
    """The column dtype of a grouping type code (a DQ_DECIMAL128 code carries precision and scale)."""
    if code & 0xFF == L.TYPE_DECIMAL128:
        return f"decimal({(code >> 8) & 0xFF},{(code >> 16) & 0xFF})"
    return {v: k for k, v in _TYPES.items()}[code]


def types_match(dtype: str, key_dtype: str) -> bool:
    """The ABI's rule: the same type, or two string columns (the offset width is free, a dictionary-encoded column is
    read through its decoded column)."""
    return dtype == key_dtype or (dtype in _STRINGS and key_dtype in _STRINGS)


class KeySet:
    """The distinct key tuples of a reference table, on the device: a self-contained frequency table (its counts are
    not used).  Column k of a probe is matched with column k of the key set; the names are the reference table's."""

    def __init__(self, table: FreqTable, columns: Sequence[str]):
        self.table = table
        self.columns: Tuple[str, ...] = tuple(columns)
        if len(self.columns) != len(table.types):
            raise ValueError(f"a key set over {len(table.types)} columns, {len(self.columns)} names")
        self.dtypes: Tuple[str, ...] = tuple(_dtype_of(t) for t in table.types)

    @staticmethod
    def from_data(data, columns: Union[str, Sequence[str]]) -> "KeySet":
        """The key set of `columns` of `data` -- a Table, a list of chunk Tables, or Arrow data.  Rows with a NULL
        in a key column make no key."""
        from .runner import arrow_data

        columns = [columns] if isinstance(columns, str) else list(columns)
        if not columns:
            raise ValueError("At least one column needs to be specified!")
        data = arrow_data(data)
        for cond in [Preconditions.hasColumn(c) for c in columns]:
            cond(data_schema(data))
        state = build_frequencies(data, columns).materialize()
        return KeySet(state.frequencies, columns)

    @property
    def num_keys(self) -> int:
        return int(L.lib.dq_freq_num_groups(self.table.handle))

    def to_bytes(self) -> bytes:
        """The key set's byte image (dq_freq_to_bytes); the column names are not part of it."""
        return self.table.to_bytes()

    @staticmethod
    def from_bytes(data: bytes, columns: Optional[Sequence[str]] = None) -> "KeySet":
        """dq_freq_from_bytes on the current torch device; columns: the names (default key0, key1, ...)."""
        table = FreqTable.from_bytes(data)
        return KeySet(table, columns if columns is not None else [f"key{k}" for k in range(len(table.types))])

    def __str__(self):
        return f"{self.num_keys} keys"

    def check_columns(self, schema, columns: Sequence[str]) -> None:
        """The preconditions of a probe of `columns` of data with `schema`: every column exists, as many columns as
        the key set has, every type the key set's (types_match).  Raises before anything is launched."""
        for c in columns:
            Preconditions.hasColumn(c)(schema)
        if len(columns) != len(self.columns):
            raise ValueError(f"{len(columns)} columns ({', '.join(columns)}) cannot be matched with a key set over "
                             f"{len(self.columns)} ({', '.join(self.columns)})")
        by_name = {c[0]: c[1] for c in schema}
        for c, kc, kt in zip(columns, self.columns, self.dtypes):
            if not types_match(by_name[c], kt):
                raise WrongColumnTypeException(
                    f"Expected type of column {c} to be {kt}, the type of column {kc} of the key set, but found "
                    f"{by_name[c]} instead! (no implicit widening: cast the column first)")

    def contains_rows(self, table: Table, columns: Sequence[str], filter=None, want_applies: bool = False):
        """One chunk: (contained bitmap, applies bitmap or None, num_contained, num_applies) -- device uint8 tensors
        of whole 64-bit words plus one zero word, the layout of the row-level results.  filter: such a bitmap of the
        rows to look at, or None for every row."""
        global probe_calls
        import torch

        columns = list(columns)
        self.check_columns(table.schema, columns)
        t = plain_utf8(table, columns)
        n, words = t.num_rows, (t.num_rows + 63) // 64
        dev = t.columns[columns[0]].values.device
        contained = torch.zeros((words + 1) * 8, dtype=torch.uint8, device=dev)
        applies = torch.zeros((words + 1) * 8, dtype=torch.uint8, device=dev) if want_applies else None
        types = (ctypes.c_int32 * len(columns))(*[_gpu_type(t.columns[c].dtype) for c in columns])
        views = (L.ColumnView * len(columns))(*[t.columns[c].view() for c in columns])
        nc, na = ctypes.c_int64(0), ctypes.c_int64(0)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            probe_calls += 1
            L.check(L.lib.dq_freq_contains_rows(self.table.handle, types, views, n,
                                                None if filter is None else filter.data_ptr(), contained.data_ptr(),
                                                None if applies is None else applies.data_ptr(), stream,
                                                ctypes.byref(nc), ctypes.byref(na)))
        return contained, applies, nc.value, na.value


class StoredKeySet:
    """What a metrics repository keeps of a key set: its number of keys.  An analyzer loaded from a repository
    carries one: it keys the stored metrics and refuses to run."""

    def __init__(self, num_keys: int):
        self.num_keys = int(num_keys)

    def __str__(self):
        return f"{self.num_keys} keys"


def where_bitmaps(chunks: List[Table], where: str) -> list:
    """Per chunk the bitmap of the rows for which `where` is TRUE (rowlevel.predicate_bitmaps: the row program the
    row-level results use); a text outside the GPU grammar is UnsupportedOnGpuPathException, as everywhere else."""
    from .predicates import UnsupportedPredicate
    from .rowlevel import predicate_bitmaps

    try:
        return predicate_bitmaps(chunks, where)
    except UnsupportedPredicate as e:
        raise UnsupportedOnGpuPathException(
            f"where `{where}` is outside the GPU-eligible set ({e}); a Spark integration keeps it on data.agg") from e


class ReferentialIntegrity(Analyzer):
    """The fraction of rows -- of those `where` keeps -- whose tuple over `columns` is a key of `reference`.  A NULL
    in a key column is not contained and counts in the denominator.  State NumMatchesAndCount, so chunk lists,
    aggregateWith / saveStatesWith and runOnAggregatedStates work as for Compliance; no applying row gives the empty
    state, as Compliance's.

    Identity: two analyzers are equal when columns and `where` are equal and they hold the same KeySet object; an
    analyzer loaded from a metrics repository (reference: StoredKeySet) equals any analyzer over equal columns and
    `where` whose key set has that many keys, which is what keys a history of stored metrics."""
    name = "ReferentialIntegrity"
    grouping = True  # not part of the fused scan: AnalysisRunner calls calculate()
    direct = True

    def __init__(self, columns: Union[str, Sequence[str]], reference, where: Optional[str] = None):
        self.columns: List[str] = [columns] if isinstance(columns, str) else list(columns)
        self.reference = reference
        self.where = where

    def _fields(self):
        return (tuple(self.columns), self.where, self.reference.num_keys)

    def __eq__(self, other):
        if type(self) is not type(other) or self._fields() != other._fields():
            return False
        stored = isinstance(self.reference, StoredKeySet) or isinstance(other.reference, StoredKeySet)
        return stored or self.reference is other.reference

    __hash__ = Analyzer.__hash__

    def __str__(self):
        return f"ReferentialIntegrity({','.join(self.columns)},{self.reference},{_opt(self.where)})"

    __repr__ = __str__

    @property
    def entity(self):
        return Entity.Column if len(self.columns) == 1 else Entity.Mutlicolumn

    @property
    def instance(self):
        return ",".join(self.columns)

    def groupingColumns(self) -> List[str]:
        return list(self.columns)

    def _lower_op(self) -> int:  # the state's image (HdfsStateProvider): NumMatchesAndCount, as Compliance's
        return L.OP_COMPLIANCE

    def preconditions(self):
        def at_least_one(schema):
            if not self.columns:
                raise ValueError("At least one column needs to be specified!")

        def runnable(schema):
            if isinstance(self.reference, StoredKeySet):
                raise ValueError(f"{self} was loaded from a metrics repository, which keeps the key set's size only: "
                                 "it keys stored metrics and cannot run")

        def matches(schema):
            self.reference.check_columns(schema, self.columns)
        return [at_least_one, runnable, matches]

    def probe(self, chunks: List[Table], want_applies: bool = False):
        """Per chunk (contained, applies or None, num_contained, num_applies): one dq_freq_contains_rows each."""
        filters = where_bitmaps(chunks, self.where) if self.where is not None else [None] * len(chunks)
        return [self.reference.contains_rows(t, self.columns, f, want_applies) for t, f in zip(chunks, filters)]

    def computeStateFrom(self, data) -> Optional[NumMatchesAndCount]:
        from .runner import _chunks

        res = self.probe(_chunks(data))
        contained, applies = sum(r[2] for r in res), sum(r[3] for r in res)
        # sum(CASE WHEN where THEN contained END) over no applying row is NULL: the empty state, as Compliance's
        return NumMatchesAndCount(contained, applies) if applies > 0 else None

    def calculate(self, data, aggregateWith=None, saveStatesWith=None) -> DoubleMetric:
        try:
            from .runner import arrow_data

            data = arrow_data(data)
            for cond in self.preconditions():
                cond(data_schema(data))
            return self.calculateMetric(self.computeStateFrom(data), aggregateWith, saveStatesWith)
        except Exception as e:
            return self.toFailureMetric(e)


# ---- dataset match -------------------------------------------------------------------------------------------------

def _lookup(key_set: KeySet, table: Table, columns: Sequence[str], filter=None):
    """One chunk: (group, num_found) -- a device int32 tensor, group[r] = the index of row r's key among the key
    set's sorted keys or -1 (dq_freq_lookup_rows: the search dq_freq_contains_rows does)."""
    global lookup_calls
    import torch

    columns = list(columns)
    t = plain_utf8(table, columns)
    n = t.num_rows
    dev = t.columns[columns[0]].values.device
    group = torch.full((max(n, 1) + 3,), -1, dtype=torch.int32, device=dev)
    types = (ctypes.c_int32 * len(columns))(*[_gpu_type(t.columns[c].dtype) for c in columns])
    views = (L.ColumnView * len(columns))(*[t.columns[c].view() for c in columns])
    nf = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        lookup_calls += 1
        L.check(L.lib.dq_freq_lookup_rows(key_set.table.handle, types, views, n,
                                          None if filter is None else filter.data_ptr(), group.data_ptr(), stream,
                                          ctypes.byref(nf)))
    return group, nf.value


class KeyedRows:
    """A reference table for DatasetMatch, on the device: the KeySet of its key columns and a payload Table of its
    compare columns in group order -- payload row g is the reference row whose key is group g of the key set.
    Reference rows with a NULL key make no key and their payload is dropped.  A byte image of the payload
    (to_bytes / from_bytes, as a KeySet has) is out of scope: rebuild it from the reference data."""

    def __init__(self, key_set: KeySet, payload: Table):
        self.key_set = key_set
        self.payload = payload

    @staticmethod
    def from_data(reference, keys: Union[str, Sequence[str]], columns: Optional[Sequence[str]] = None) -> "KeyedRows":
        """reference: ONE table -- a Table, a one-element chunk list, or Arrow data (Table.from_arrow makes one table of
        it).  keys: its key columns, which must be unique over its rows; columns: the payload columns (default: every
        other column).  A dict_utf8 payload column is kept as its decoded column."""
        import torch

        from .ingest import is_arrow
        from .schema import take_column
        from .table import decoded

        keys = [keys] if isinstance(keys, str) else list(keys)
        if not keys:
            raise ValueError("At least one column needs to be specified!")
        if not isinstance(reference, Table) and is_arrow(reference):
            reference = Table.from_arrow(reference)
        if not isinstance(reference, Table):
            chunks = list(reference)
            if len(chunks) != 1:
                raise ValueError(f"the reference of a dataset match must be one table, got {len(chunks)} chunks: "
                                 "concatenate them first (Table.from_arrow makes one table of Arrow batches)")
            reference = chunks[0]
        names = [c[0] for c in reference.schema]
        columns = [c for c in names if c not in keys] if columns is None else list(columns)
        if not columns:
            raise ValueError("a dataset match needs at least one column to compare beyond the keys")
        for cond in [Preconditions.hasColumn(c) for c in keys + columns]:
            cond(reference.schema)
        key_set = KeySet.from_data(reference, keys)
        G = key_set.num_keys
        group, num_found = _lookup(key_set, reference, keys)
        n = reference.num_rows
        group = group[:n].long()
        hit = group >= 0
        if num_found != G:  # (every key is found at least once: more found rows than keys means a key on several rows)
            dup = int((torch.bincount(group[hit], minlength=max(G, 1)) > 1).sum().item())
            raise ValueError(f"{dup} keys of the reference occur on more than one of its rows ({num_found} rows with a "
                             f"key, {G} distinct keys): the match would be ambiguous")
        rows = torch.zeros(max(G, 1), dtype=torch.int64, device=group.device)  # group -> row
        rows[group[hit]] = torch.arange(n, dtype=torch.int64, device=group.device)[hit]
        payload = Table([take_column(decoded(reference.columns[c]), rows, G) for c in columns])
        return KeyedRows(key_set, payload)

    @property
    def num_keys(self) -> int:
        return self.key_set.num_keys

    @property
    def key_columns(self) -> Tuple[str, ...]:
        return self.key_set.columns

    @property
    def columns(self) -> Tuple[str, ...]:
        return tuple(self.payload.columns)

    @property
    def dtypes(self) -> Tuple[str, ...]:
        return tuple(c.dtype for c in self.payload.columns.values())

    @property
    def nbytes(self) -> int:
        """Device bytes of the payload's buffers (the key set's are its frequency table's)."""
        total = 0
        for c in self.payload.columns.values():
            for t in (c.values, c.validity, c.offsets):
                if t is not None:
                    total += t.numel() * t.element_size()
        return total

    def __str__(self):
        return f"{self.num_keys} keys"

    def check_columns(self, schema, key_columns: Sequence[str], mapping: Sequence[Tuple[str, str]]) -> None:
        """The preconditions of a match: the key columns against the key set (KeySet.check_columns), 1 .. 16 compare
        pairs (data column, payload column), every column present on its side, every pair's types in agreement
        (types_match: no widening).  Raises before anything is launched."""
        self.key_set.check_columns(schema, list(key_columns))
        if not 1 <= len(mapping) <= MAX_MATCH_COLUMNS:
            raise ValueError(f"a dataset match compares 1 to {MAX_MATCH_COLUMNS} columns, got {len(mapping)}")
        by_name = {c[0]: c[1] for c in schema}
        ref = dict(zip(self.columns, self.dtypes))
        for c, rc in mapping:
            Preconditions.hasColumn(c)(schema)
            if rc not in ref:
                raise NoSuchColumnException(f"The reference does not include column {rc}! (it holds "
                                            f"{', '.join(self.columns)})")
            if not types_match(by_name[c], ref[rc]):
                raise WrongColumnTypeException(
                    f"Expected type of column {c} to be {ref[rc]}, the type of column {rc} of the reference, but found "
                    f"{by_name[c]} instead! (no implicit widening: cast the column first)")

    def match_rows(self, table: Table, key_columns: Sequence[str], mapping: Sequence[Tuple[str, str]], filter=None,
                   want_found: bool = False, want_applies: bool = False, want_columns: bool = False):
        """One chunk: one dq_freq_lookup_rows and one dq_rows_match.  Returns a dict: matched / found / applies
        (device bitmaps in the row-level layout; found / applies None unless wanted), num_matched, num_found,
        num_applies, mismatch (per compare pair the found rows that differ in it; None unless want_columns), group
        (the lookup's int32 tensor: the payload row of every row, or -1)."""
        global match_calls
        import torch

        mapping = [tuple(m) for m in mapping]
        self.check_columns(table.schema, key_columns, mapping)
        cols = [m[0] for m in mapping]
        t = plain_utf8(table, cols)
        group, _ = _lookup(self.key_set, table, key_columns, filter)
        n, words, k = t.num_rows, (t.num_rows + 63) // 64, len(mapping)
        dev = group.device

        def bitmap(wanted=True):
            return torch.zeros((words + 1) * 8, dtype=torch.uint8, device=dev) if wanted else None

        matched, found, applies = bitmap(), bitmap(want_found), bitmap(want_applies)
        types = (ctypes.c_int32 * k)(*[_gpu_type(t.columns[c].dtype) for c in cols])
        views = (L.ColumnView * k)(*[t.columns[c].view() for c in cols])
        ptypes = (ctypes.c_int32 * k)(*[_gpu_type(self.payload.columns[rc].dtype) for _, rc in mapping])
        pviews = (L.ColumnView * k)(*[self.payload.columns[rc].view() for _, rc in mapping])
        nm, nf, na = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        mis = (ctypes.c_int64 * k)() if want_columns else None
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            match_calls += 1
            L.check(L.lib.dq_rows_match(types, views, ptypes, pviews, k, n, self.payload.num_rows, group.data_ptr(),
                                        None if filter is None else filter.data_ptr(), matched.data_ptr(),
                                        None if found is None else found.data_ptr(),
                                        None if applies is None else applies.data_ptr(),
                                        dev.index if dev.index is not None else torch.cuda.current_device(), stream,
                                        ctypes.byref(nm), ctypes.byref(nf), ctypes.byref(na), mis))
        return {"matched": matched, "found": found, "applies": applies, "group": group[:n], "num_matched": nm.value,
                "num_found": nf.value, "num_applies": na.value, "mismatch": None if mis is None else list(mis)}


class StoredKeyedRows(StoredKeySet):
    """What a metrics repository keeps of a KeyedRows: its number of keys (a DatasetMatch loaded from a repository
    carries one: it keys the stored metrics and refuses to run)."""


def _compare_mapping(compareColumns, reference) -> Optional[Tuple[Tuple[str, str], ...]]:
    """compareColumns as pairs (data column, reference column): a list of names present on both sides, a dict
    {data column: reference column}, or None for every payload column of the reference by name (kept as None for a
    stored reference, which has no payload to name)."""
    if compareColumns is None:
        cols = getattr(reference, "columns", None)
        return None if cols is None else tuple((c, c) for c in cols)
    if isinstance(compareColumns, str):
        return ((compareColumns, compareColumns),)
    if isinstance(compareColumns, dict):
        return tuple((str(k), str(v)) for k, v in compareColumns.items())
    return tuple((m[0], m[1]) if isinstance(m, (tuple, list)) else (m, m) for m in compareColumns)


class DatasetMatch(Analyzer):
    """The fraction of rows -- of those `where` keeps -- that equal the reference's row with the same key: key column k
    is matched with key k of `reference` (a KeyedRows), and every compare column equals (null-safe) the reference's.
    compareColumns: a list of names present on both sides, a dict {data column: reference column}, or None for every
    payload column by name.  A row whose key the reference lacks (a NULL key included) does not match and counts in
    the denominator.  State NumMatchesAndCount, the empty state when no row applies -- as ReferentialIntegrity, so
    chunk lists, Arrow data, aggregateWith / saveStatesWith and runOnAggregatedStates work the same way.

    Identity follows ReferentialIntegrity: equal key columns, compare mapping and `where`, and the same KeyedRows
    object; an analyzer loaded from a metrics repository (reference: StoredKeyedRows) equals any analyzer with equal
    fields whose reference has that many keys."""
    name = "DatasetMatch"
    grouping = True  # not part of the fused scan: AnalysisRunner calls calculate()
    direct = True

    def __init__(self, keyColumns: Union[str, Sequence[str]], compareColumns, reference, where: Optional[str] = None):
        self.keyColumns: List[str] = [keyColumns] if isinstance(keyColumns, str) else list(keyColumns)
        self.reference = reference
        self.mapping = _compare_mapping(compareColumns, reference)
        self.where = where

    @property
    def compareColumns(self) -> List[str]:
        return [m[0] for m in self.mapping or ()]

    def _fields(self):
        return (tuple(self.keyColumns), self.mapping, self.where, self.reference.num_keys)

    def __eq__(self, other):
        if type(self) is not type(other) or self._fields() != other._fields():
            return False
        stored = isinstance(self.reference, StoredKeySet) or isinstance(other.reference, StoredKeySet)
        return stored or self.reference is other.reference

    __hash__ = Analyzer.__hash__

    def _mapping_str(self) -> str:
        return ",".join(c if c == rc else f"{c}->{rc}" for c, rc in self.mapping or ())

    def __str__(self):
        return (f"DatasetMatch({','.join(self.keyColumns)},{self._mapping_str()},{self.reference},"
                f"{_opt(self.where)})")

    __repr__ = __str__

    @property
    def entity(self):
        return Entity.Mutlicolumn

    @property
    def instance(self):
        return ",".join(self.keyColumns + self.compareColumns)

    def groupingColumns(self) -> List[str]:
        return list(self.keyColumns) + self.compareColumns

    def _lower_op(self) -> int:  # the state's image (HdfsStateProvider): NumMatchesAndCount, as Compliance's
        return L.OP_COMPLIANCE

    def preconditions(self):
        def at_least_one(schema):
            if not self.keyColumns:
                raise ValueError("At least one column needs to be specified!")

        def runnable(schema):
            if isinstance(self.reference, StoredKeySet):
                raise ValueError(f"{self} was loaded from a metrics repository, which keeps the reference's size only: "
                                 "it keys stored metrics and cannot run")

        def matches(schema):
            self.reference.check_columns(schema, self.keyColumns, self.mapping)
        return [at_least_one, runnable, matches]

    def match(self, chunks: List[Table], want_found=False, want_applies=False, want_columns=False) -> list:
        """Per chunk KeyedRows.match_rows' dict: one lookup and one match launch each."""
        filters = where_bitmaps(chunks, self.where) if self.where is not None else [None] * len(chunks)
        return [self.reference.match_rows(t, self.keyColumns, self.mapping, f, want_found, want_applies, want_columns)
                for t, f in zip(chunks, filters)]

    def probe(self, chunks: List[Table], want_applies: bool = False):
        """The row-level form, in ReferentialIntegrity.probe's shape: per chunk (matched, applies or None,
        num_matched, num_applies)."""
        return [(r["matched"], r["applies"], r["num_matched"], r["num_applies"])
                for r in self.match(chunks, want_applies=want_applies)]

    def breakdown(self, data) -> dict:
        """Where the rows went: matched + value_mismatch + key_missing = applies, and per compare column (named as the
        data names it) the found rows that differ in it -- "which column drifted"."""
        from .runner import _chunks, arrow_data

        data = arrow_data(data)
        for cond in self.preconditions():
            cond(data_schema(data))
        res = self.match(_chunks(data), want_columns=True)
        matched, found, applies = (sum(r[k] for r in res) for k in ("num_matched", "num_found", "num_applies"))
        by_col = {c: sum(r["mismatch"][i] for r in res) for i, c in enumerate(self.compareColumns)}
        return {"matched": matched, "key_missing": applies - found, "value_mismatch": found - matched,
                "applies": applies, "mismatch_by_column": by_col}

    def computeStateFrom(self, data) -> Optional[NumMatchesAndCount]:
        from .runner import _chunks

        res = self.match(_chunks(data))
        matched, applies = sum(r["num_matched"] for r in res), sum(r["num_applies"] for r in res)
        return NumMatchesAndCount(matched, applies) if applies > 0 else None  # (the empty state, as Compliance's)

    def calculate(self, data, aggregateWith=None, saveStatesWith=None) -> DoubleMetric:
        try:
            from .runner import arrow_data

            data = arrow_data(data)
            for cond in self.preconditions():
                cond(data_schema(data))
            return self.calculateMetric(self.computeStateFrom(data), aggregateWith, saveStatesWith)
        except Exception as e:
            return self.toFailureMetric(e)
