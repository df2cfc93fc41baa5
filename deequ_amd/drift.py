"""Distribution drift: how far is a column's distribution from the one it had in another table?

"Today's feed against last month's", "a training set against its serving traffic", "a migrated table against its
source": the question after referential integrity (does the key exist there?) and dataset match (is the row equal
there?) when no key exists and row-wise equality is too strict.  Upstream Deequ answers it with
Distance.categoricalDistance (L-infinity) and numericalDistance; TFDV and Great Expectations ship L-infinity,
Jensen-Shannon and Kolmogorov-Smirnov comparators.

The reference is a ReferenceDistribution -- the frozen, self-contained frequency table of the other table's columns,
as a matching.KeySet is its key set -- and the data's side is the FrequenciesAndNumRows every grouping analyzer
builds and shares per (columns, where).  The comparison is one device join of the two tables (dq_freq_distance,
dq_freq_ks: csrc/dq_dist.hip); nothing but the result leaves the device.

Semantics (include/dqscan.h; these are this project's -- the reference implementation at this version has no such
analyzer -- and tests/test_drift_gpu.py pins them).  N is a table's number of non-NULL tuples: NULL rows are part of
neither distribution (their drift is Completeness's job).  p = count / N on the data's side, q on the reference's, 0
for a group a side lacks.  Groups are equal when their values are: strings by length and bytes, decimals by their 16
bytes, everything else by value bits (every NaN one group, -0.0 and 0.0 two); two tuples under one 64-bit hash are two
groups.  Types must agree exactly but for the string offset width (an i32 column is not matched with an i64
reference: cast it first).

    linf  max |p - q|                                          bit for bit the IEEE expression
    tv    1/2 sum |p - q|
    js    1/2 sum [p ln(p/m) + q ln(q/m)], m = (p + q) / 2     natural logarithm, in [0, ln 2]
    ks    max_x |F_data(x) - F_ref(x)|                         one ordered fixed-width column; floats order with
                                                               -0.0 below 0.0 and NaN greatest; bit for bit

With binning=Bins... the distribution is the one over the bins' labels (binning.binned_frequencies: the labels'
table, NULL rows in no slot), and the reference must carry an equal Bins.

Not in scope: PSI or chi-square (they need a smoothing convention for empty groups); a p-value for KS; approximate KS
from ApproxQuantileState digests; a reference given as a stream; profiler or suggestion rules that propose drift
checks; a multi-GPU combine of frequency states; the per-group list of shifts beyond the single linf_group of
breakdown().
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple, Union

from . import _lib as L
from .analyzers import Preconditions, data_schema
from .grouping import FreqTable, FrequenciesAndNumRows, FrequencyBasedAnalyzer, build_frequencies, selection_of
from .matching import _dtype_of, types_match
from .metrics import DoubleMetric, Success, WrongColumnTypeException

METHODS = ("linf", "tv", "js", "ks")
KS_DTYPES = ("f64", "f32", "i64", "i32", "i16", "i8", "date32", "timestamp")  # dq_freq_ks's ordered column types

distance_calls = 0  # dq_freq_distance launches of the process (tests count them, as matching.probe_calls)
ks_calls = 0        # dq_freq_ks launches of the process


def _stream():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def freq_distance(a: FreqTable, b: FreqTable) -> Optional[L.FreqDistanceResult]:
    """dq_freq_distance of two self-contained tables (a: the data's, b: the reference's); None when either has no
    value."""
    global distance_calls
    out = L.FreqDistanceResult()
    distance_calls += 1
    L.check(L.lib.dq_freq_distance(a.handle, b.handle, _stream(), ctypes.byref(out)))
    return out if out.defined else None


def freq_ks(a: FreqTable, b: FreqTable) -> Optional[float]:
    """dq_freq_ks of two unhashed single-column tables; None when either has no value."""
    global ks_calls
    value, defined = ctypes.c_double(), ctypes.c_int32()
    ks_calls += 1
    L.check(L.lib.dq_freq_ks(a.handle, b.handle, _stream(), ctypes.byref(value), ctypes.byref(defined)))
    return value.value if defined.value else None


def _check_binning(binning):
    from .binning import Bins

    if binning is not None and not isinstance(binning, Bins):
        raise TypeError(f"binning: a Bins is needed (Bins.edges / Bins.equal_width), got {type(binning).__name__}")


class ReferenceDistribution:
    """The frozen distribution of a reference table's columns, on the device: a self-contained frequency table.
    Column k of the data is compared with column k of the reference; the names are the reference table's.  binning:
    the Bins the table's labels were counted with (the table is then the one over the labels)."""

    def __init__(self, table: FreqTable, columns: Sequence[str], binning=None):
        _check_binning(binning)
        self.table = table
        self.columns: Tuple[str, ...] = tuple(columns)
        if len(self.columns) != len(table.types):
            raise ValueError(f"a distribution over {len(table.types)} columns, {len(self.columns)} names")
        if not table.self_contained():
            raise ValueError("a reference distribution owns its values: materialize() the state first")
        self.dtypes: Tuple[str, ...] = tuple(_dtype_of(t) for t in table.types)
        self.binning = binning
        self.num_groups = int(L.lib.dq_freq_num_groups(table.handle))
        self.num_values = int(table.summary(1).num_values)
        if self.num_values == 0:
            raise ValueError("the reference has no non-NULL value: it has no distribution to compare with")

    @staticmethod
    def from_data(data, columns: Union[str, Sequence[str]], where: Optional[str] = None,
                  binning=None) -> "ReferenceDistribution":
        """The distribution of `columns` of `data` -- a Table, a list of chunk Tables, or Arrow data -- over the rows
        `where` keeps.  Rows with a NULL in one of the columns are no part of it.  binning: one numeric column counted
        into the Bins' labels."""
        from .runner import _chunks, arrow_data

        columns = [columns] if isinstance(columns, str) else list(columns)
        if not columns:
            raise ValueError("At least one column needs to be specified!")
        _check_binning(binning)
        data = arrow_data(data)
        for cond in [Preconditions.hasColumn(c) for c in columns]:
            cond(data_schema(data))
        if binning is not None:
            from .binning import binned_frequencies

            if len(columns) != 1:
                raise ValueError(f"a binning is over one column, got {len(columns)}")
            Preconditions.isNumeric(columns[0])(data_schema(data))
            chunks = _chunks(data)
            state = binned_frequencies(chunks, columns[0], binning, selection_of(chunks, where))
        else:
            state = build_frequencies(data, columns, where)
        return ReferenceDistribution(state.materialize().frequencies, columns, binning)

    @staticmethod
    def from_state(state: FrequenciesAndNumRows, columns: Optional[Sequence[str]] = None,
                   binning=None) -> "ReferenceDistribution":
        """A FrequenciesAndNumRows as the reference -- e.g. the one HdfsStateProvider loads: yesterday's saved state is
        today's reference.  columns: the names (default col0, col1, ...)."""
        table = state.materialize().frequencies
        names = columns if columns is not None else [f"col{k}" for k in range(len(table.types))]
        return ReferenceDistribution(table, [names] if isinstance(names, str) else names, binning)

    def to_bytes(self) -> bytes:
        """The table's byte image (dq_freq_to_bytes); names and binning are not part of it."""
        return self.table.to_bytes()

    @staticmethod
    def from_bytes(data: bytes, columns: Optional[Sequence[str]] = None, binning=None) -> "ReferenceDistribution":
        """dq_freq_from_bytes on the current torch device; columns: the names (default col0, col1, ...)."""
        table = FreqTable.from_bytes(data)
        names = columns if columns is not None else [f"col{k}" for k in range(len(table.types))]
        return ReferenceDistribution(table, [names] if isinstance(names, str) else names, binning)

    def __str__(self):
        return f"{self.num_groups} groups of {self.num_values} values"

    def check_columns(self, schema, columns: Sequence[str], binning=None) -> None:
        """The preconditions of a comparison of `columns` of data with `schema`: as many columns as the reference
        has, an equal binning, every type the reference's (matching.types_match; with a binning, a numeric column).
        Raises before anything is launched."""
        if len(columns) != len(self.columns):
            raise ValueError(f"{len(columns)} columns ({', '.join(columns)}) cannot be compared with a distribution "
                             f"over {len(self.columns)} ({', '.join(self.columns)})")
        if binning != self.binning:
            raise ValueError(f"the reference was built with binning {self.binning}, the analyzer has {binning}: "
                             "distributions over different bins cannot be compared")
        by_name = {c[0]: c[1] for c in schema}
        if binning is not None:
            Preconditions.isNumeric(columns[0])(schema)
            return
        for c, rc, rt in zip(columns, self.columns, self.dtypes):
            if not types_match(by_name[c], rt):
                raise WrongColumnTypeException(
                    f"Expected type of column {c} to be {rt}, the type of column {rc} of the reference distribution, "
                    f"but found {by_name[c]} instead! (no implicit widening: cast the column first)")


class StoredDistribution:
    """What a metrics repository keeps of a reference distribution: its numbers of groups and values.  An analyzer
    loaded from a repository carries one: it keys the stored metrics and refuses to run."""

    def __init__(self, num_groups: int, num_values: int):
        self.num_groups, self.num_values = int(num_groups), int(num_values)

    def __str__(self):
        return f"{self.num_groups} groups of {self.num_values} values"


def _render_value(dtype: str, raw: bytes):
    """A stored value (FreqTable.take_values) as a Python value."""
    import struct

    from .table import decimal_ps

    ps = decimal_ps(dtype)
    if dtype in ("utf8", "large_utf8"):
        return raw.decode("utf-8", "replace")
    if ps:
        from decimal import Decimal

        return Decimal(int.from_bytes(raw, "little", signed=True)).scaleb(-ps[1])
    if dtype == "f64":
        return struct.unpack("<d", raw)[0]
    if dtype == "f32":
        return struct.unpack("<f", raw)[0]
    if dtype == "bool":
        return bool(raw[0])
    return int.from_bytes(raw, "little", signed=True)


def _group_of(table: FreqTable, key: int) -> tuple:
    """The tuple of the group with key word `key`: an unhashed table's key is its value's bits, a hashed table's value
    comes from its store."""
    dtypes = [_dtype_of(t) for t in table.types]
    if len(dtypes) == 1 and dtypes[0] not in ("utf8", "large_utf8") and not dtypes[0].startswith("decimal("):
        width = {"f32": 4, "i32": 4, "date32": 4, "i16": 2, "i8": 1, "bool": 1}.get(dtypes[0], 8)
        return (_render_value(dtypes[0], (key & ((1 << (8 * width)) - 1)).to_bytes(width, "little")),)
    return tuple(_render_value(dt, table.take_values([key], c)[0]) for c, dt in enumerate(dtypes))


class DistributionDistance(FrequencyBasedAnalyzer):
    """The distance between the distribution of `columns` -- over the rows `where` keeps -- and `reference`'s, by
    `method`: "linf", "tv", "js" or "ks" (the module docstring defines them).

    Without a binning this is an ordinary grouping analyzer: the runner builds one frequency state per (columns,
    where) and shares it with Uniqueness, Entropy and the others over the same columns; aggregateWith /
    saveStatesWith / runOnAggregatedStates work as for them.  With binning=Bins... it makes its own pass, as a binned
    Histogram does: the state is the frequency table of the column's bin labels.  No applying non-NULL row gives the
    empty-state failure of the other frequency analyzers.

    Identity follows ReferentialIntegrity: equal columns, method, binning and `where`, and the same
    ReferenceDistribution object; an analyzer loaded from a metrics repository (reference: StoredDistribution) equals
    any analyzer with equal fields whose reference has that many groups and values."""
    name = "DistributionDistance"
    shares_selections = True  # calculate(..., selections=): the run's cache of `where` bitmaps (the binned pass)

    def __init__(self, columns: Union[str, Sequence[str]], reference, method: str = "linf", binning=None,
                 where: Optional[str] = None):
        super().__init__(columns, where)
        if method not in METHODS:
            raise ValueError(f"method: one of {', '.join(METHODS)} is needed, got {method!r}")
        _check_binning(binning)
        if method == "ks" and binning is not None:
            raise ValueError("method ks compares the values' order: it takes no binning")
        if method == "ks" and len(self.columns) != 1:
            raise ValueError(f"method ks is over one ordered column, got {len(self.columns)}")
        if binning is not None and len(self.columns) != 1:
            raise ValueError(f"a binning is over one column, got {len(self.columns)}")
        self.reference = reference
        self.method = method
        self.binning = binning

    @property
    def direct(self) -> bool:  # (the runner: a direct analyzer makes its own device pass)
        return self.binning is not None

    def _fields(self):
        return (tuple(self.columns), self.method, self.binning, self.where, self.reference.num_groups,
                self.reference.num_values)

    def __eq__(self, other):
        if type(self) is not type(other) or self._fields() != other._fields():
            return False
        stored = isinstance(self.reference, StoredDistribution) or isinstance(other.reference, StoredDistribution)
        return stored or self.reference is other.reference

    __hash__ = FrequencyBasedAnalyzer.__hash__

    def __str__(self):
        binning = "" if self.binning is None else f",{self.binning}"
        return (f"DistributionDistance(List({', '.join(self.columns)}),{self.method},{self.reference}{binning}"
                f"{self._where_str()})")

    __repr__ = __str__

    def preconditions(self):
        def at_least_one(schema):
            if not self.columns:
                raise ValueError("At least one column needs to be specified!")

        def runnable(schema):
            if isinstance(self.reference, StoredDistribution):
                raise ValueError(f"{self} was loaded from a metrics repository, which keeps the reference's size "
                                 "only: it keys stored metrics and cannot run")

        def matches(schema):
            self.reference.check_columns(schema, self.columns, self.binning)

        def ordered(schema):
            dtype = {c[0]: c[1] for c in schema}[self.columns[0]]
            if self.method == "ks" and dtype not in KS_DTYPES:
                raise WrongColumnTypeException(
                    f"Expected type of column {self.columns[0]} to be one of ({', '.join(KS_DTYPES)}) for method ks, "
                    f"but found {dtype} instead!")
        return [at_least_one, runnable] + [Preconditions.hasColumn(c) for c in self.columns] + [matches, ordered]

    def computeStateFrom(self, data, selections: Optional[dict] = None) -> Optional[FrequenciesAndNumRows]:
        if self.binning is None:
            return build_frequencies(data, self.columns, self.where, self, selections)
        from .binning import binned_frequencies
        from .runner import _chunks

        chunks = _chunks(data)
        return binned_frequencies(chunks, self.columns[0], self.binning,
                                  selection_of(chunks, self.where, self, selections))

    def _compare(self, state: FrequenciesAndNumRows):
        if isinstance(self.reference, StoredDistribution):
            raise ValueError(f"{self} keys stored metrics and cannot run")
        return freq_distance(state.materialize().frequencies, self.reference.table)

    def computeMetricFrom(self, state: Optional[FrequenciesAndNumRows]) -> DoubleMetric:
        if state is None:
            return self._empty()
        if self.method == "ks":
            if isinstance(self.reference, StoredDistribution):
                raise ValueError(f"{self} keys stored metrics and cannot run")
            v = freq_ks(state.frequencies, self.reference.table)
        else:
            r = self._compare(state)
            v = None if r is None else getattr(r, self.method)
        if v is None:  # no applying non-NULL row on the data's side
            return self._empty()
        return DoubleMetric(self.entity, self.name, self.instance, Success(v))

    def calculate(self, data, aggregateWith=None, saveStatesWith=None, selections: Optional[dict] = None) -> DoubleMetric:
        try:
            from .runner import arrow_data

            data = arrow_data(data)
            for cond in self.preconditions():
                cond(data_schema(data))
            state = self.computeStateFrom(data, selections)
            if aggregateWith is not None or saveStatesWith is not None:
                state.materialize()  # once, before the merge and the first persist
            return self.calculateMetric(state, aggregateWith, saveStatesWith)
        except Exception as e:
            return self.toFailureMetric(e)

    def breakdown(self, data) -> dict:
        """What drifted: the sizes of the join's three parts, the probability mass outside the common groups on either
        side, the three distances and the group attaining L-infinity, as a tuple of Python values."""
        from .runner import arrow_data

        data = arrow_data(data)
        for cond in self.preconditions():
            cond(data_schema(data))
        state = self.computeStateFrom(data).materialize()
        r = self._compare(state)
        if r is None:
            raise ValueError(f"Empty state for analyzer {self}, all input values were NULL.")
        side = state.frequencies if r.linf_side == 0 else self.reference.table
        n_data = int(state.frequencies.summary(max(1, state.numRows)).num_values)
        return {"common": int(r.n_common), "only_data": int(r.n_only_a), "only_reference": int(r.n_only_b),
                "mass_only_data": r.count_only_a / n_data,
                "mass_only_reference": r.count_only_b / self.reference.num_values,
                "linf": r.linf, "tv": r.tv, "js": r.js, "linf_group": _group_of(side, int(r.linf_key))}
