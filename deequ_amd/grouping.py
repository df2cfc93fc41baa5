"""Grouping analyzers on the GPU (analyzers/GroupingAnalyzers.scala and the frequency-based
analyzers): Uniqueness, Distinctness, CountDistinct, Entropy, UniqueValueRatio.

FrequencyBasedAnalyzer.computeFrequencies (GroupingAnalyzers.scala:44-82) becomes dq_freq_build: a
sort-based GROUP BY ... COUNT(*) over the rows whose grouping columns are all non-null, held on the
device as (key, count) groups.  The state is FrequenciesAndNumRows (frequencies + numRows) and sums
as the reference's outer join (:118-138) via dq_freq_merge; each metric is computed from the
summary (groups, groups of count 1, entropy) exactly as its aggregationFunctions prescribe.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Union

from . import _lib as L
from .analyzers import Analyzer, Preconditions, data_schema
from .metrics import DoubleMetric, EmptyStateException, Entity, Failure, Success, wrap_if_necessary
from .states import State

_TYPES = {"f64": L.TYPE_F64, "i64": L.TYPE_I64, "i32": L.TYPE_I32, "utf8": L.TYPE_UTF8,
          "large_utf8": L.TYPE_LARGE_UTF8, "f32": L.TYPE_F32, "i16": L.TYPE_I16, "i8": L.TYPE_I8,
          "bool": L.TYPE_BOOL, "date32": L.TYPE_DATE32, "timestamp": L.TYPE_TIMESTAMP}


def _gpu_type(dtype: str) -> int:
    """The grouping / quantile kernels' column type code (a DecimalType's carries its precision / scale)."""
    from .table import decimal_ps

    ps = decimal_ps(dtype)
    if ps:
        return L.decimal_type(*ps)
    t = _TYPES.get(dtype)
    if t is None:
        from .metrics import UnsupportedOnGpuPathException

        raise UnsupportedOnGpuPathException(f"column type {dtype} is not a GPU column type")
    return t


def _java_decimal_to_string(u: int, scale: int) -> str:
    """java.math.BigDecimal.toString of unscaled u at scale >= 0 (Spark's CAST(decimal AS STRING)): plain notation
    unless the adjusted exponent digits - 1 - scale is below -6, then "1.5E-7" / "0E-18"."""
    sign = "-" if u < 0 else ""
    coeff = str(abs(u))
    adjusted = len(coeff) - 1 - scale
    if scale == 0:
        return sign + coeff
    if adjusted >= -6:
        if len(coeff) > scale:
            return f"{sign}{coeff[:-scale]}.{coeff[-scale:]}"
        return f"{sign}0.{'0' * (scale - len(coeff))}{coeff}"
    return f"{sign}{coeff[0]}{'.' + coeff[1:] if len(coeff) > 1 else ''}E{adjusted}"


def _java_float_to_string(f: float) -> str:
    """java.lang.Float.toString (CAST(float AS STRING)): Double.toString's forms with float's shortest digits."""
    import math

    import numpy as np

    if math.isnan(f) or math.isinf(f) or f == 0.0:
        return _java_double_to_string(f)
    if 1e-3 <= abs(f) < 1e7:
        r = np.format_float_positional(np.float32(f), unique=True)
        return r + "0" if r.endswith(".") else r
    m, e = np.format_float_scientific(np.float32(f), unique=True, exp_digits=1).split("e")
    return f"{m + '0' if m.endswith('.') else m}E{int(e)}"


def _render_fixed(dtype: str, key: int) -> str:
    """CAST(value AS STRING) of a fixed-width grouping key (value bits, integers sign-extended; timestamps in UTC
    as Spark's DateTimeUtils.timestampToString with the session zone UTC)."""
    import datetime

    import numpy as np

    v = int(np.uint64(key).astype(np.int64))
    if dtype == "f64":
        return _java_double_to_string(float(np.uint64(key).view(np.float64)))
    if dtype == "f32":
        return _java_float_to_string(float(np.uint32(key & 0xFFFFFFFF).view(np.float32)))
    if dtype == "bool":
        return "true" if v else "false"
    if dtype == "date32":
        return (datetime.date(1970, 1, 1) + datetime.timedelta(days=v)).isoformat()
    if dtype == "timestamp":
        t = datetime.datetime(1970, 1, 1) + datetime.timedelta(microseconds=v)
        frac = f"{t.microsecond:06d}".rstrip("0")
        return t.strftime("%Y-%m-%d %H:%M:%S") + ("." + frac if frac else "")
    return str(v)


class FreqTable:
    """Owner of a device dq_freq_table (sorted distinct keys + counts)."""

    def __init__(self, handle: ctypes.c_void_p, types: Sequence[int]):
        self.handle = handle
        self.types = tuple(types)

    def summary(self, num_rows: int) -> L.FreqSummary:
        s = L.FreqSummary()
        L.check(L.lib.dq_freq_summarize(self.handle, num_rows, ctypes.byref(s)))
        return s

    def merged(self, other: "FreqTable") -> "FreqTable":
        h = ctypes.c_void_p()
        L.check(L.lib.dq_freq_merge(self.handle, other.handle, ctypes.byref(h)))
        return FreqTable(h, self.types)

    def export(self):
        import numpy as np

        n = L.lib.dq_freq_num_groups(self.handle)
        keys = np.zeros(max(1, n), dtype=np.uint64)
        counts = np.zeros(max(1, n), dtype=np.int64)
        L.check(L.lib.dq_freq_export(self.handle, keys.ctypes.data_as(ctypes.c_void_p),
                                     counts.ctypes.data_as(ctypes.c_void_p), max(1, n)))
        return keys[:n], counts[:n]

    def self_contained(self) -> bool:
        """True when the table owns its groups' values (an unhashed table's keys are its values; a hashed one after
        materialize / from_bytes / a merge of two such tables)."""
        return bool(L.lib.dq_freq_self_contained(self.handle))

    def to_bytes(self) -> bytes:
        """dq_freq_to_bytes: the table's byte image (include/dqscan.h); DQ_E_STATE unless self-contained."""
        n = L.lib.dq_freq_to_bytes(self.handle, None, 0)
        if n < 0:
            L.check(int(n))
        buf = (ctypes.c_uint8 * max(1, n))()
        n2 = L.lib.dq_freq_to_bytes(self.handle, buf, n)
        if n2 < 0:
            L.check(int(n2))
        return bytes(buf)[:n]

    @staticmethod
    def from_bytes(data: bytes) -> "FreqTable":
        """dq_freq_from_bytes on the current torch device and stream (the image is checked on the host first)."""
        import torch

        h = ctypes.c_void_p()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(L.lib.dq_freq_from_bytes(data, len(data), torch.cuda.current_device(), stream, ctypes.byref(h)))
        img_cols = int.from_bytes(data[12:16], "little")
        types = [int.from_bytes(data[16 + 4 * c:20 + 4 * c], "little") for c in range(img_cols)]
        return FreqTable(h, types)

    def take_values(self, keys, col: int = 0):
        """The stored values of column col for the groups with these keys, in their order (dq_freq_take_values):
        a list of bytes objects -- a string's bytes, or a fixed-width value's little-endian bytes."""
        import numpy as np

        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = len(keys)
        kp = keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        offs = (ctypes.c_int64 * (n + 1))()
        need = ctypes.c_int64()
        L.check(L.lib.dq_freq_take_values(self.handle, kp, n, col, None, 0, offs, ctypes.byref(need)))
        buf = (ctypes.c_uint8 * max(1, need.value))()
        L.check(L.lib.dq_freq_take_values(self.handle, kp, n, col, buf, need.value, offs, ctypes.byref(need)))
        raw = bytes(buf)[:need.value]
        t = self.types[col]
        if t in (L.TYPE_UTF8, L.TYPE_LARGE_UTF8):
            return [raw[offs[i]:offs[i + 1]] for i in range(n)]
        w = need.value // n if n else 0
        return [raw[i * w:(i + 1) * w] for i in range(n)]

    def mutual_information(self, num_rows: int) -> Optional[float]:
        """dq_freq_mutual_information of a self-contained two-column table; None when it has no group."""
        value, defined = ctypes.c_double(), ctypes.c_int32()
        L.check(L.lib.dq_freq_mutual_information(self.handle, num_rows, ctypes.byref(value), ctypes.byref(defined)))
        return value.value if defined.value else None

    def __del__(self):
        try:
            if self.handle:
                L.lib.dq_freq_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def _views(chunks, columns: Sequence[str]):
    """The chunk-major column views and row counts dq_freq_build / dq_freq_materialize take."""
    views = (L.ColumnView * max(1, len(chunks) * len(columns)))()
    rows = (ctypes.c_int64 * max(1, len(chunks)))()
    for k, t in enumerate(chunks):
        rows[k] = t.num_rows
        for c, name in enumerate(columns):
            views[k * len(columns) + c] = t.columns[name].view()
    return views, rows


# times a `where` text was turned into per-chunk bitmaps (tests read it, as they read expressions.eval_calls)
selection_builds = 0


class Selection:
    """The rows of a chunk list for which a `where` is TRUE: per chunk the device bitmap (64-bit words, LSB first: the
    layout dq_take_index reads) and its number of set bits.  The data the filtered analyzers see is these rows."""

    def __init__(self, where: str, bitmaps: Sequence, counts: Sequence[int]):
        self.where, self.bitmaps, self.counts = where, list(bitmaps), [int(c) for c in counts]

    @property
    def num_rows(self) -> int:
        return sum(self.counts)

    def pointers(self):
        """One selection pointer per chunk, as the _where entry points take them."""
        return (ctypes.c_void_p * max(1, len(self.bitmaps)))(*[b.data_ptr() for b in self.bitmaps])


def _where_columns(schema, where: str) -> set:
    """The columns a `where` text names outside its arithmetic operands (host only)."""
    from .analyzers import PlanBuilder

    b = PlanBuilder([(n, "utf8" if dt == "dict_utf8" else dt, nl) for n, dt, nl in schema], collect_exprs=True)
    b.pred(where)
    return set(b.columns)


def selection_of(data, where: Optional[str], analyzer=None, cache: Optional[dict] = None) -> Optional[Selection]:
    """The Selection of `where` over `data` (None for no filter), through rowlevel.predicate_selection: arithmetic
    operands and dictionary columns as the row-level checks handle them.  cache: a run's {where text: Selection} --
    every analyzer of the run that carries the text shares one evaluation.  A text outside the GPU grammar raises the
    UnsupportedOnGpuPathException the scan analyzers' failure metrics carry, a missing column what Compliance's
    `where` fails with; both before anything is launched."""
    if where is None:
        return None
    if cache is not None and where in cache:
        return cache[where]
    global selection_builds
    from .metrics import NoSuchColumnException, UnsupportedOnGpuPathException
    from .predicates import UnsupportedPredicate
    from .rowlevel import predicate_selection
    from .runner import _chunks

    try:
        pairs = predicate_selection(_chunks(data), where)
    except UnsupportedPredicate as e:
        raise UnsupportedOnGpuPathException(
            f"{analyzer} is outside the GPU-eligible set ({e}); a Spark integration keeps it on data.agg") from e
    except NoSuchColumnException as e:
        if isinstance(e.__cause__, KeyError):  # the predicate compiler's own error: what Compliance fails with
            raise e.__cause__
        raise
    selection_builds += 1
    sel = Selection(where, [p[0] for p in pairs], [p[1] for p in pairs])
    if cache is not None:
        cache[where] = sel
    return sel


def index_path_dictionaries(chunks, columns: Sequence[str]):
    """The distinct Dictionary objects of a grouping that is computed on dictionary indices, else None.  The index
    path takes a grouping over exactly one column that is dict_utf8 in every chunk, when the distinct dictionaries
    together hold no more entries than the chunks hold rows (beyond that the entries are more work than the rows).
    Everything else -- tuples of columns, a mix of plain and dictionary chunks -- reads the decoded column."""
    if len(columns) != 1 or not chunks:
        return None
    cols = [t.columns.get(columns[0]) for t in chunks]
    if any(c is None or c.dtype != "dict_utf8" for c in cols):
        return None
    dicts = list({id(c.dictionary): c.dictionary for c in cols}.values())
    if len({d.entries.dtype for d in dicts}) != 1:  # (one table type: utf8 or large_utf8 entries throughout)
        return None
    if sum(d.n_entries for d in dicts) > sum(t.num_rows for t in chunks):
        return None
    return dicts


def _frequencies_from_indices(chunks, column: str, dicts, selection: Optional[Selection] = None) -> "FrequenciesAndNumRows":
    """The frequency table of a dictionary column without its strings' bytes per row: the rows of every chunk counted
    per entry (dq_dict_count, one int64 array per distinct dictionary), then dq_freq_build_weighted over the
    dictionaries' entries -- one input chunk per dictionary -- with those counts as weights.  Entries no row carries
    and NULL entries make no group, entries of equal bytes (in one dictionary or in two) make one.  The state's
    representative rows point into the entries, which are its source tables.  selection: only its rows are counted
    (dq_dict_count_where) and numRows is their number."""
    import dataclasses

    import torch

    from .table import Table

    dev = torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    counts = {id(d): torch.zeros(max(1, d.n_entries), dtype=torch.int64, device=d.entries.values.device) for d in dicts}
    for k, t in enumerate(chunks):
        col = t.columns[column]
        view = col.view()
        if selection is None:
            L.check(L.lib.dq_dict_count(ctypes.byref(view), t.num_rows, counts[id(col.dictionary)].data_ptr(), dev,
                                        stream))
        else:
            L.check(L.lib.dq_dict_count_where(ctypes.byref(view), t.num_rows, selection.bitmaps[k].data_ptr(),
                                              counts[id(col.dictionary)].data_ptr(), dev, stream))
    entry_chunks = [Table([dataclasses.replace(d.entries, name=column)]) for d in dicts]
    types = (ctypes.c_int32 * 1)(_gpu_type(dicts[0].entries.dtype))
    views, rows = _views(entry_chunks, [column])
    weights = (ctypes.c_void_p * len(dicts))(*[counts[id(d)].data_ptr() for d in dicts])
    h = ctypes.c_void_p()
    L.check(L.lib.dq_freq_build_weighted(types, 1, views, rows, weights, len(dicts), dev, stream, ctypes.byref(h)))
    num_rows = sum(t.num_rows for t in chunks) if selection is None else selection.num_rows
    return FrequenciesAndNumRows(FreqTable(h, list(types)), num_rows, source=(entry_chunks, [column]))


def build_frequencies(data, columns: Sequence[str], where: Optional[str] = None, analyzer=None,
                      selections: Optional[dict] = None) -> "FrequenciesAndNumRows":
    """computeFrequencies(data, columns) + numRows = data.count() on the GPU.  A single dictionary-encoded column is
    grouped on its indices (index_path_dictionaries); the table is the one its decoded column gives.
    where: the frequencies and numRows of the rows for which the predicate is TRUE, as if the data held those rows
    alone (dq_freq_build_where: the selection bitmaps join the validity in the kernels' row test; no column is
    copied).  The index path is kept when the filter does not read the grouping column, and left when it does.
    analyzer: named in the failure of a refused predicate; selections: a run's cache for selection_of."""
    from .runner import _chunks
    from .table import plain_utf8

    chunks = _chunks(data)
    selection = selection_of(chunks, where, analyzer, selections)
    dicts = index_path_dictionaries(chunks, columns)
    if dicts is not None and selection is not None and columns[0] in _where_columns(chunks[0].schema, where):
        dicts = None
    if dicts is not None:
        return _frequencies_from_indices(chunks, columns[0], dicts, selection)
    # a dictionary-encoded column among the grouping's own columns is read as the plain column it stands for; the
    # table's other dictionary columns are not touched
    chunks = plain_utf8(chunks, columns)
    import torch

    schema = {name: dt for name, dt, _ in chunks[0].schema}
    types = (ctypes.c_int32 * len(columns))(*[_gpu_type(schema[c]) for c in columns])
    views, rows = _views(chunks, columns)
    h = ctypes.c_void_p()
    dev = torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if selection is None:
        L.check(L.lib.dq_freq_build(types, len(columns), views, rows, len(chunks), dev, stream, ctypes.byref(h)))
        num_rows = sum(t.num_rows for t in chunks)
    else:
        L.check(L.lib.dq_freq_build_where(types, len(columns), views, rows, selection.pointers(), len(chunks), dev,
                                          stream, ctypes.byref(h)))
        num_rows = selection.num_rows
    return FrequenciesAndNumRows(FreqTable(h, list(types)), num_rows, source=(chunks, list(columns)))


class FrequenciesAndNumRows(State):
    """GroupingAnalyzers.scala:118-138 (the frequencies live on the device).

    A state built from data over strings, decimals or several columns names its groups' values by row ids into the
    tables it was built from, and remembers those tables: while an unmaterialised state lives, its input tables stay
    alive.  materialize() copies the values into the table (dq_freq_materialize) once and drops that reference; sum
    and HdfsStateProvider.persist materialise first, so merged, persisted and loaded states are self-contained."""

    OP = -1

    def __init__(self, frequencies: FreqTable, numRows: int, source=None):
        self.frequencies = frequencies
        self.numRows = int(numRows)
        self._source = source  # (chunks, columns) the table was built from, until materialize()

    def materialize(self) -> "FrequenciesAndNumRows":
        src, self._source = self._source, None
        if src is not None:
            try:
                chunks, columns = src
                views, rows = _views(chunks, columns)
                L.check(L.lib.dq_freq_materialize(self.frequencies.handle, views, rows, len(chunks)))
            except Exception:
                self._source = src
                raise
        return self

    def sum(self, other: "FrequenciesAndNumRows") -> "FrequenciesAndNumRows":
        self.materialize()
        other.materialize()
        return FrequenciesAndNumRows(self.frequencies.merged(other.frequencies), self.numRows + other.numRows)

    def __eq__(self, other):
        if not isinstance(other, FrequenciesAndNumRows) or self.numRows != other.numRows:
            return False
        a, b = self.frequencies.export(), other.frequencies.export()
        return a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()

    __hash__ = None

    def _to_c(self):
        raise TypeError("FrequenciesAndNumRows has no fixed-size dq_state (HdfsStateProvider stores the table's "
                        "image: FreqTable.to_bytes)")


class FrequencyBasedAnalyzer(Analyzer):
    """ScanShareableFrequencyBasedAnalyzer (GroupingAnalyzers.scala:84-116)."""

    grouping = True

    def __init__(self, columns: Union[str, Sequence[str]], where: Optional[str] = None):
        self.columns: List[str] = [columns] if isinstance(columns, str) else list(columns)
        self.where = where

    def _fields(self):  # (an unfiltered analyzer's identity is the one it had before filters)
        return (tuple(self.columns),) if self.where is None else (tuple(self.columns), ("where", self.where))

    def _where_str(self) -> str:
        return "" if self.where is None else f",Some({self.where})"

    def __str__(self):
        return f"{type(self).__name__}(List({', '.join(self.columns)}){self._where_str()})"

    __repr__ = __str__

    @property
    def entity(self):
        return Entity.Column if len(self.columns) == 1 else Entity.Mutlicolumn

    @property
    def instance(self):
        return ",".join(self.columns)

    def groupingColumns(self) -> List[str]:
        return list(self.columns)

    def preconditions(self):
        def at_least_one(schema):
            if not self.columns:
                raise ValueError("At least one column needs to be specified!")
        return [at_least_one] + [Preconditions.hasColumn(c) for c in self.columns]

    def computeStateFrom(self, data) -> Optional[FrequenciesAndNumRows]:
        return build_frequencies(data, self.columns, self.where, self)

    def _value(self, s: L.FreqSummary, num_rows: int) -> Optional[float]:
        raise NotImplementedError

    def computeMetricFrom(self, state: Optional[FrequenciesAndNumRows]) -> DoubleMetric:
        if state is None:
            return self._empty()
        v = self._value(state.frequencies.summary(state.numRows), state.numRows)
        if v is None:  # the SQL aggregate over an empty frequencies table is NULL
            return self._empty()
        return DoubleMetric(self.entity, self.name, self.instance, Success(v))

    def _empty(self) -> DoubleMetric:
        return self.toFailureMetric(EmptyStateException(
            f"Empty state for analyzer {self}, all input values were NULL."))

    def toFailureMetric(self, e: BaseException) -> DoubleMetric:
        return DoubleMetric(self.entity, self.name, self.instance, Failure(wrap_if_necessary(e)))

    def calculate(self, data, aggregateWith=None, saveStatesWith=None) -> DoubleMetric:
        try:
            for cond in self.preconditions():
                cond(data_schema(data))
            return self.calculateMetric(self.computeStateFrom(data), aggregateWith, saveStatesWith)
        except Exception as e:
            return self.toFailureMetric(e)


class Uniqueness(FrequencyBasedAnalyzer):  # Uniqueness.scala:24-36: sum(count == 1) / numRows
    name = "Uniqueness"

    def _value(self, s, n):
        return None if s.num_groups == 0 else s.num_unique / n


class Distinctness(FrequencyBasedAnalyzer):  # Distinctness.scala:26-38: sum(count >= 1) / numRows
    name = "Distinctness"

    def _value(self, s, n):
        return None if s.num_groups == 0 else s.num_groups / n


class CountDistinct(FrequencyBasedAnalyzer):  # CountDistinct.scala:22-38: count(*), never NULL
    name = "CountDistinct"

    def _value(self, s, n):
        return float(s.num_groups)


class UniqueValueRatio(FrequencyBasedAnalyzer):  # UniqueValueRatio.scala:22-43
    name = "UniqueValueRatio"

    def _value(self, s, n):
        # Row.getDouble of a NULL sum unboxes to 0.0 (no isNullAt check here): 0.0 / 0 -> NaN
        num_unique = float(s.num_unique) if s.num_groups else 0.0
        return num_unique / s.num_groups if s.num_groups else float("nan")


class Entropy(FrequencyBasedAnalyzer):  # Entropy.scala:26-44 (single column)
    name = "Entropy"

    def __init__(self, column: str, where: Optional[str] = None):
        super().__init__([column], where)

    def __str__(self):
        return f"Entropy({self.columns[0]}{self._where_str()})"

    __repr__ = __str__

    def _value(self, s, n):
        return None if s.num_groups == 0 else s.entropy




class MutualInformation(FrequencyBasedAnalyzer):  # MutualInformation.scala:32-80
    """sum over the joint groups of (pxy/N) ln((pxy/N) / ((px/N)(py/N))), marginals summed from the joint
    counts (rows with both values), N = numRows.  calculate(data) alone is one device pass over the rows
    (dq_mutual_information); with a loader or persister the state is the joint frequencies of the two columns
    (build_frequencies, made self-contained) and the metric comes from it (dq_freq_mutual_information), as do
    runOnAggregatedStates and loadStateAndComputeMetric."""
    name = "MutualInformation"
    direct = True
    shares_selections = True  # calculate(..., selections=): the run's cache of `where` bitmaps (selection_of)

    def __init__(self, columnA, columnB: Optional[str] = None, where: Optional[str] = None):
        super().__init__(list(columnA) if columnB is None else [columnA, columnB], where)

    @property
    def entity(self):
        return Entity.Mutlicolumn

    def preconditions(self):
        def exactly_two(schema):  # Preconditions.exactlyNColumns(columns, 2)
            if len(self.columns) != 2:
                raise ValueError(f"{self.columns} has {len(self.columns)} columns, but exactly 2 are required")
        return [exactly_two] + [Preconditions.hasColumn(c) for c in self.columns]

    def compute(self, data, selections: Optional[dict] = None) -> DoubleMetric:
        import torch

        from .runner import _chunks

        chunks = _chunks(data)
        selection = selection_of(chunks, self.where, self, selections)
        schema = {name: dt for name, dt, _ in chunks[0].schema}
        types = (ctypes.c_int32 * 2)(*[_gpu_type(schema[c]) for c in self.columns])
        views = (L.ColumnView * max(1, 2 * len(chunks)))()
        rows = (ctypes.c_int64 * max(1, len(chunks)))()
        for k, t in enumerate(chunks):
            rows[k] = t.num_rows
            for c, name in enumerate(self.columns):
                views[2 * k + c] = t.columns[name].view()
        value, defined = ctypes.c_double(), ctypes.c_int32()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if selection is None:
            L.check(L.lib.dq_mutual_information(types, views, rows, len(chunks), sum(t.num_rows for t in chunks),
                                                torch.cuda.current_device(), stream, ctypes.byref(value),
                                                ctypes.byref(defined)))
        else:
            L.check(L.lib.dq_mutual_information_where(types, views, rows, selection.pointers(), len(chunks),
                                                      selection.num_rows, torch.cuda.current_device(), stream,
                                                      ctypes.byref(value), ctypes.byref(defined)))
        if not defined.value:
            return self._empty()
        return DoubleMetric(self.entity, self.name, self.instance, Success(value.value))

    def calculate(self, data, aggregateWith=None, saveStatesWith=None, selections: Optional[dict] = None) -> DoubleMetric:
        try:
            for cond in self.preconditions():
                cond(data_schema(data))
            if aggregateWith is not None or saveStatesWith is not None:
                state = build_frequencies(data, self.columns, self.where, self, selections)
                return self.calculateMetric(state, aggregateWith, saveStatesWith)
            return self.compute(data, selections)
        except Exception as e:
            return self.toFailureMetric(e)

    def computeMetricFrom(self, state: Optional[FrequenciesAndNumRows]) -> DoubleMetric:
        if state is None:
            return self._empty()
        v = state.materialize().frequencies.mutual_information(state.numRows)
        if v is None:
            return self._empty()
        return DoubleMetric(self.entity, self.name, self.instance, Success(v))


def _java_double_to_string(d: float) -> str:
    """java.lang.Double.toString (Spark's CAST(double AS STRING)): plain decimal for 1e-3 <= |d| < 1e7,
    computerized scientific notation otherwise; digits from the shortest round-trip repr (Java 8 can
    print one more digit in rare cases)."""
    import math

    if math.isnan(d):
        return "NaN"
    if math.isinf(d):
        return "Infinity" if d > 0 else "-Infinity"
    if d == 0.0:
        return "-0.0" if math.copysign(1.0, d) < 0 else "0.0"
    if 1e-3 <= abs(d) < 1e7:
        r = repr(d)
        return r if "." in r else r + ".0"
    from decimal import Decimal

    t = Decimal(repr(abs(d))).as_tuple()  # the shortest round-trip digits
    digits = "".join(map(str, t.digits)).lstrip("0")
    exp10 = t.exponent + len(t.digits) - 1 - (len(t.digits) - len("".join(map(str, t.digits)).lstrip("0")))
    digits = digits.rstrip("0") or "0"
    mant = digits[0] + "." + (digits[1:] or "0")
    return f"{'-' if d < 0 else ''}{mant}E{exp10}"


class Histogram(Analyzer):  # Histogram.scala:33-99
    """Counts of the column's values cast to string (NULL -> "NullValue"): the maxDetailBins largest
    groups (ties in key order; Spark's rdd.top leaves them unspecified) with ratio count / numRows, and
    the number of bins.  The frequencies are the device table of build_frequencies; values are
    rendered on the host only for the returned bins.

    binning: a binning.Bins, the declarative stand-in for binningUdf (which runs in Spark, not here).  The numeric
    column is counted into the declared bins in one device pass (dq_bin_count) and the groups are the bins' labels,
    as Spark's groupBy over a UDF returning those labels builds them: a bin no row fell into makes no group, so
    numberOfBins counts the non-empty bins (and "NullValue").  The binning is part of str(analyzer), which names the
    persisted state: two binnings of one column never share a state.  The state's keys are plain strings, so merging
    states that were built with different bins cannot be detected: it is the caller's error."""
    name = "Histogram"
    grouping = True
    direct = True
    shares_selections = True
    NullFieldReplacement = "NullValue"
    MaximumAllowedDetailBins = 1000

    def __init__(self, column: str, binningUdf=None, maxDetailBins: int = 1000, binning=None, *,
                 where: Optional[str] = None):
        from .binning import Bins

        if binning is not None and not isinstance(binning, Bins):
            raise TypeError(f"binning: a Bins is needed (Bins.edges / Bins.equal_width), got {type(binning).__name__}")
        self.column = column
        self.binningUdf = binningUdf
        self.maxDetailBins = maxDetailBins
        self.binning = binning
        self.where = where

    def _fields(self):
        base = (self.column, id(self.binningUdf) if self.binningUdf is not None else None, self.maxDetailBins)
        if self.binning is not None:
            base += (self.binning,)
        return base if self.where is None else base + (("where", self.where),)

    def __str__(self):
        udf = "None" if self.binningUdf is None else "Some(udf)"
        w = "" if self.where is None else f",Some({self.where})"
        if self.binning is not None:
            return f"Histogram({self.column},{udf},{self.maxDetailBins},{self.binning}{w})"
        return f"Histogram({self.column},{udf},{self.maxDetailBins}{w})"

    __repr__ = __str__

    @property
    def instance(self):
        return self.column

    def groupingColumns(self):
        return [self.column]

    def preconditions(self):
        from .metrics import IllegalAnalyzerParameterException

        def param_check(schema):
            if self.maxDetailBins > Histogram.MaximumAllowedDetailBins:
                raise IllegalAnalyzerParameterException(
                    f"Cannot return histogram values for more than {Histogram.MaximumAllowedDetailBins} values")
            if self.binningUdf is not None and self.binning is not None:
                raise IllegalAnalyzerParameterException(
                    "Histogram takes a binningUdf or a binning, not both")
        if self.binning is not None:  # the bins are over numbers: the reference's wrong-column-type failure
            return [param_check, Preconditions.hasColumn(self.column), Preconditions.isNumeric(self.column)]
        return [param_check, Preconditions.hasColumn(self.column)]

    def toFailureMetric(self, e: BaseException):
        from .metrics import HistogramMetric

        return HistogramMetric(self.column, Failure(wrap_if_necessary(e)))

    def _render(self, data, dtype: str, key: int, rep: int) -> str:
        import numpy as np

        from .table import decimal_ps

        ps = decimal_ps(dtype)
        if dtype not in ("utf8", "large_utf8") and not ps:
            return _render_fixed(dtype, key)
        if rep == (1 << 64) - 1:
            raise NotImplementedError("Histogram of a merged string / decimal frequency table (no representative rows)")
        from .runner import _chunks

        col = _chunks(data)[rep >> 40].columns[self.column]
        r = rep & ((1 << 40) - 1)
        if ps:  # the representative row's 16-byte unscaled value, as Decimal.toString
            u = int.from_bytes(bytes(col.values[16 * r:16 * r + 16].cpu().numpy()), "little", signed=True)
            return _java_decimal_to_string(u, ps[1])
        width = 8 if col.dtype == "large_utf8" else 4
        o = col.offsets[r * width:(r + 2) * width].cpu().numpy().view(np.int64 if width == 8 else np.int32)
        return bytes(col.values[int(o[0]):int(o[1])].cpu().numpy()).decode("utf-8", "replace")

    def computeMetricFrom(self, state: Optional["FrequenciesAndNumRows"]):
        """The metric from a state alone (runOnAggregatedStates, loadStateAndComputeMetric): a self-contained table
        renders its bins from its own values."""
        if state is None:
            return self.toFailureMetric(EmptyStateException(
                f"Empty state for analyzer {self}, all input values were NULL."))
        return self.computeMetricFromState(state.materialize(), None)

    def computeMetricFromState(self, state: "FrequenciesAndNumRows", data):
        from .metrics import Distribution, DistributionValue, HistogramMetric
        from .table import decimal_ps

        n = self.maxDetailBins
        keys = (ctypes.c_uint64 * max(1, n))()
        counts = (ctypes.c_int64 * max(1, n))()
        reps = (ctypes.c_uint64 * max(1, n))()
        got = ctypes.c_int32()
        L.check(L.lib.dq_freq_top(state.frequencies.handle, n, keys, counts, reps, ctypes.byref(got)))
        t0 = state.frequencies.types[0]
        dtype = ({v: k for k, v in _TYPES.items()}.get(t0) or
                 f"decimal({(t0 >> 8) & 0xFF},{(t0 >> 16) & 0xFF})")  # (a DQ_DECIMAL128 code carries p, s)
        ps = decimal_ps(dtype)
        if (dtype in ("utf8", "large_utf8") or ps) and state.frequencies.self_contained():
            # strings / decimals of a table that owns its values: the selected groups' values from its store
            vals = state.frequencies.take_values([keys[i] for i in range(got.value)], 0)
            names = [_java_decimal_to_string(int.from_bytes(v, "little", signed=True), ps[1]) if ps
                     else v.decode("utf-8", "replace") for v in vals]
            bins = [(names[i], int(counts[i])) for i in range(got.value)]
        else:  # fixed-width keys are the values; an unmaterialised table reads its representative rows
            bins = [(self._render(data, dtype, keys[i], reps[i]), int(counts[i])) for i in range(got.value)]
        summary = state.frequencies.summary(state.numRows)
        nulls = state.numRows - summary.num_values
        bin_count = summary.num_groups
        if nulls > 0:  # .na.fill("NullValue"): the NULLs are one more group
            merged = False
            for i, (k, c) in enumerate(bins):
                if k == Histogram.NullFieldReplacement:  # a literal "NullValue" string joins them
                    bins[i] = (k, c + nulls)
                    merged = True
            if not merged:
                bins.append((Histogram.NullFieldReplacement, nulls))
                bin_count += 1
            bins.sort(key=lambda kc: -kc[1])
            bins = bins[:n]
        values = {k: DistributionValue(c, c / state.numRows) for k, c in bins}
        return HistogramMetric(self.column, Success(Distribution(values, numberOfBins=bin_count)))

    def calculate(self, data, aggregateWith=None, saveStatesWith=None, selections: Optional[dict] = None):
        try:
            for cond in self.preconditions():
                cond(data_schema(data))
            if self.binningUdf is not None:
                from .metrics import UnsupportedOnGpuPathException

                raise UnsupportedOnGpuPathException(f"{self}: a binning UDF runs in Spark, not on the GPU path")
            if self.binning is not None:
                from .binning import binned_frequencies
                from .runner import _chunks

                chunks = _chunks(data)
                state = binned_frequencies(chunks, self.column, self.binning,
                                           selection_of(chunks, self.where, self, selections))
            else:
                state = build_frequencies(data, [self.column], self.where, self, selections)
            if aggregateWith is not None or saveStatesWith is not None:
                state.materialize()  # once, before the merge and the first persist
            if aggregateWith is not None:
                prev = aggregateWith.load(self)
                if prev is not None:
                    state = state.sum(prev)
            if saveStatesWith is not None:
                saveStatesWith.persist(self, state)
            # the bins' values are rendered from the tables the state's representative rows point into: the chunks (a
            # dictionary column read as bytes: its decoded twin), or the entries of a column grouped on its indices
            return self.computeMetricFromState(state, state._source[0] if state._source is not None else data)
        except Exception as e:
            return self.toFailureMetric(e)
