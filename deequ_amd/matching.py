"""Referential integrity: do the rows of one table occur among the keys of another?

"Every order.customer_id exists in customer.id", "every (country, zip) of this feed occurs in the master list": the
rule upstream Deequ expresses with ReferentialIntegrity / doesDatasetMatch and Spark users write as a left semi-join.
Here the other table's keys are a KeySet -- the self-contained frequency table of its key columns (dq_freq_build +
dq_freq_materialize), built once and reused across runs -- and the match is one dq_freq_contains_rows per chunk: a
per-row bitmap of the rows whose tuple is a group of the key set.

Semantics (include/dqscan.h): a NULL in any key column is "not contained" and still counts in the denominator (SQL
IN / semi-join); types must agree exactly, but for the offset width of string columns -- nothing is widened
implicitly (cast an i32 column before matching it against i64 keys); a `where` selects the rows that count.

Not done here: match columns beyond the keys (upstream's matchColumnMappings), key-uniqueness checks on either side,
implicit type widening, probing inside the fused scan.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple, Union

from . import _lib as L
from .analyzers import Analyzer, Preconditions, _opt, data_schema
from .grouping import _TYPES, FreqTable, _gpu_type, build_frequencies
from .metrics import DoubleMetric, Entity, UnsupportedOnGpuPathException, WrongColumnTypeException
from .states import NumMatchesAndCount
from .table import Table, plain_utf8

probe_calls = 0  # dq_freq_contains_rows launches of the process (tests count them, as expressions.eval_calls)

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
