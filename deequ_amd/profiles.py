"""ColumnProfiler on the GPU path (profiles/ColumnProfiler.scala, profiles/ColumnProfile.scala).

Three scans plus the cast, as the reference's three passes:
  1. Size, Completeness, ApproxCountDistinct and -- string columns -- DataType in one fused AnalysisRunner run;
  2. the numeric-string cast (casts.py) and Minimum / Maximum / Mean / StandardDeviation / Sum / ApproxQuantiles of
     every column whose type is Integral or Fractional, native numeric columns included (:219-235);
  3. the histograms of all low-cardinality string and boolean columns in one dq_cat_hist_build call
     (computeHistograms, :518-565): counting tables in LDS, no sort (csrc/dq_cathist.hip).
The metrics-repository parameters are out of scope here: passing one raises NotImplementedError.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

from . import _lib as L
from .analyzers import (ApproxCountDistinct, Completeness, DataType, DataTypeInstances, Maximum, Mean, Minimum, Size,
                        StandardDeviation, Sum, determineType)
from .casts import cast_numeric_string_columns, second_pass_analyzers
from .metrics import Distribution, DistributionValue, UnsupportedOnGpuPathException
from .quantiles import ApproxQuantiles
from .runner import AnalysisRunner, AnalyzerContext, _chunks, arrow_data
from .table import Table, decimal_ps

DEFAULT_CARDINALITY_THRESHOLD = 120
NULL_FIELD_REPLACEMENT = "NullValue"  # Histogram.NullFieldReplacement
MAX_COLUMNS_PER_CALL = 1024           # dq_cat_hist_build's column limit (include/dqscan.h)
_STRING = ("utf8", "large_utf8", "dict_utf8")  # (a dictionary-encoded column is a StringType column)


@dataclass(eq=True)
class StandardColumnProfile:  # ColumnProfile.scala:34-42
    column: str
    completeness: float
    approximateNumDistinctValues: int
    dataType: str
    isDataTypeInferred: bool
    typeCounts: Dict[str, int]
    histogram: Optional[Distribution]


@dataclass(eq=True)
class NumericColumnProfile:  # ColumnProfile.scala:44-58
    column: str
    completeness: float
    approximateNumDistinctValues: int
    dataType: str
    isDataTypeInferred: bool
    typeCounts: Dict[str, int]
    histogram: Optional[Distribution]
    mean: Optional[float]
    maximum: Optional[float]
    minimum: Optional[float]
    sum: Optional[float]
    stdDev: Optional[float]
    approxPercentiles: Optional[List[float]]
    # the equal-width distribution between minimum and maximum (withNumericDistributions; None: not asked for, or the
    # column has no finite minimum < maximum)
    distribution: Optional[Distribution] = None


ColumnProfile = Union[StandardColumnProfile, NumericColumnProfile]


@dataclass(eq=True)
class ColumnProfiles:  # ColumnProfile.scala:60-62
    profiles: Dict[str, ColumnProfile]
    numRecords: int

    @staticmethod
    def toJson(columnProfiles: Sequence[ColumnProfile]) -> str:
        """ColumnProfiles.toJson (ColumnProfile.scala:67-146).  As there, typeCounts is not written (the reference
        builds its object and never adds it) and isDataTypeInferred is a string."""
        import json

        columns = []
        for p in columnProfiles:
            c = {"column": p.column, "dataType": p.dataType,
                 "isDataTypeInferred": "true" if p.isDataTypeInferred else "false", "completeness": p.completeness,
                 "approximateNumDistinctValues": p.approximateNumDistinctValues}
            if p.histogram is not None:
                c["histogram"] = [{"value": k, "count": v.absolute, "ratio": v.ratio}
                                  for k, v in p.histogram.values.items()]
            if isinstance(p, NumericColumnProfile):
                for key, v in (("mean", p.mean), ("maximum", p.maximum), ("minimum", p.minimum), ("sum", p.sum),
                               ("stdDev", p.stdDev)):
                    if v is not None:
                        c[key] = v
                c["approxPercentiles"] = list(p.approxPercentiles or [])
                if p.distribution is not None:
                    c["distribution"] = [{"value": k, "count": v.absolute, "ratio": v.ratio}
                                         for k, v in p.distribution.values.items()]
            columns.append(c)
        return json.dumps({"columns": columns}, indent=2)


@dataclass
class GenericColumnStatistics:  # ColumnProfiler.scala:31-42
    numRecords: int
    inferredTypes: Dict[str, str]
    knownTypes: Dict[str, str]
    typeDetectionHistograms: Dict[str, Dict[str, int]]
    approximateNumDistincts: Dict[str, int]
    completenesses: Dict[str, float]

    def typeOf(self, column: str) -> str:
        return {**self.inferredTypes, **self.knownTypes}[column]  # inferredTypes ++ knownTypes


@dataclass
class NumericColumnStatistics:  # ColumnProfiler.scala:44-51
    means: Dict[str, float]
    stdDevs: Dict[str, float]
    minima: Dict[str, float]
    maxima: Dict[str, float]
    sums: Dict[str, float]
    approxPercentiles: Dict[str, List[float]]


def known_type(dtype: str) -> str:
    """extractGenericStatistics' knownTypes (:376-392) of a non-string column type: Short / Int / Long -> Integral,
    Decimal / Float / Double -> Fractional, Boolean -> Boolean, Timestamp -> String, everything else (Byte and Date
    included) -> Unknown."""
    I = DataTypeInstances
    if dtype in ("i16", "i32", "i64"):
        return I.Integral
    if dtype in ("f32", "f64") or decimal_ps(dtype):
        return I.Fractional
    if dtype == "bool":
        return I.Boolean
    if dtype == "timestamp":
        return I.String
    return I.Unknown


def generic_stats_analyzers(schema, relevant: Sequence[str]) -> List:
    """getAnalyzersForGenericStats (:200-217)."""
    out = []
    for name, dtype, _ in schema:
        if name in relevant:
            out += [Completeness(name), ApproxCountDistinct(name)]
            if dtype in _STRING:
                out.append(DataType(name))
    return out


def extract_generic_statistics(columns: Sequence[str], schema, results: AnalyzerContext) -> GenericColumnStatistics:
    """extractGenericStatistics (:341-396).  Like the reference's metric.value.get, a failed first-pass metric raises."""
    num_records = int([m.value.get() for a, m in results.metricMap.items() if isinstance(a, Size)][0])
    inferred, histograms, distincts, completenesses = {}, {}, {}, {}
    for a, m in results.metricMap.items():
        if isinstance(a, DataType):
            dist = m.value.get()
            inferred[a.column] = determineType(dist)
            histograms[a.column] = {k: v.absolute for k, v in dist.values.items()}
        elif isinstance(a, ApproxCountDistinct):
            distincts[a.column] = int(m.value.get())  # .toLong
        elif isinstance(a, Completeness):
            completenesses[a.column] = m.value.get()
    known = {name: known_type(dtype) for name, dtype, _ in schema if name in columns and dtype not in _STRING}
    return GenericColumnStatistics(num_records, inferred, known, histograms, distincts, completenesses)


def extract_numeric_statistics(results: AnalyzerContext) -> NumericColumnStatistics:
    """extractNumericStatistics (:420-485): the successful metrics only."""
    out = NumericColumnStatistics({}, {}, {}, {}, {}, {})
    slots = {Mean: out.means, StandardDeviation: out.stdDevs, Minimum: out.minima, Maximum: out.maxima, Sum: out.sums}
    for a, m in results.metricMap.items():
        if not m.value.isSuccess:
            continue
        if isinstance(a, ApproxQuantiles):
            out.approxPercentiles[a.column] = sorted(m.value.get().values())
        elif type(a) in slots:
            slots[type(a)][a.column] = m.value.get()
    return out


def find_target_columns_for_histograms(schema, stats: GenericColumnStatistics, threshold: int) -> List[str]:
    """findTargetColumnsForHistograms (:492-516): string / boolean columns typed String or Boolean with at most
    `threshold` approximate distinct values."""
    original = {name for name, dtype, _ in schema if dtype in _STRING or dtype == "bool"}
    I = DataTypeInstances
    return [c for c, count in stats.approximateNumDistincts.items()
            if c in original and stats.typeOf(c) in (I.String, I.Boolean) and count <= threshold]


def _render_string(chunks, column: str, rep: int) -> str:
    """The string of a representative row (chunk << 40 | row), as Histogram._render."""
    import numpy as np

    col = chunks[rep >> 40].columns[column]
    r = rep & ((1 << 40) - 1)
    width = 8 if col.dtype == "large_utf8" else 4
    o = col.offsets[r * width:(r + 2) * width].cpu().numpy().view(np.int64 if width == 8 else np.int32)
    return bytes(col.values[int(o[0]):int(o[1])].cpu().numpy()).decode("utf-8", "replace")


def _distribution(counts: Dict[str, int], nulls: int) -> Distribution:
    """Counts per rendered value plus the NULLs under "NullValue" (joining a literal "NullValue" string's count);
    ratio = count / the column's sum, numberOfBins = the number of values (:549-563)."""
    if nulls > 0:
        counts[NULL_FIELD_REPLACEMENT] = counts.get(NULL_FIELD_REPLACEMENT, 0) + nulls
    total = sum(counts.values())
    return Distribution({k: DistributionValue(c, c / total) for k, c in counts.items()}, numberOfBins=len(counts))


def _indices_distribution(data, column: str) -> Distribution:
    """A dictionary column counted on its indices (grouping.index_path_dictionaries): its table from the entry
    counts, under the fused pass's capacity rule applied to the table's groups -- the distinct non-NULL values some
    row carries.  At most dq_cat_hist_capacity() of them: the counts from one export and the values from one
    dq_freq_take_values call over the materialised table (the entries the groups stand for), as the fused pass exports
    a plain column.  More: the fallback of a plain column over capacity, on the same table."""
    from .grouping import build_frequencies

    state = build_frequencies(data, [column])
    if int(L.lib.dq_freq_num_groups(state.frequencies.handle)) > int(L.lib.dq_cat_hist_capacity()):
        return _fallback_distribution(data, column, state)
    nulls = state.numRows - state.frequencies.summary(state.numRows).num_values
    keys, cnts = state.frequencies.export()
    if len(keys) == 0:
        return _distribution({}, nulls)
    values = state.materialize().frequencies.take_values(keys, 0)
    return _distribution({v.decode("utf-8", "replace"): int(c) for v, c in zip(values, cnts)}, nulls)


def _fallback_distribution(data, column: str, state=None) -> Distribution:
    """A column over the fused pass's capacity, through the grouping path: every group of build_frequencies (or of
    `state`, that call's result)."""
    from .grouping import Histogram, build_frequencies

    if state is None:
        state = build_frequencies(data, [column])
    if state._source is not None:  # (the tables the representative rows point into: see Histogram.calculate)
        data = state._source[0]
    n = int(L.lib.dq_freq_num_groups(state.frequencies.handle))
    keys = (ctypes.c_uint64 * max(1, n))()
    cnts = (ctypes.c_int64 * max(1, n))()
    reps = (ctypes.c_uint64 * max(1, n))()
    got = ctypes.c_int32()
    L.check(L.lib.dq_freq_top(state.frequencies.handle, n, keys, cnts, reps, ctypes.byref(got)))
    dtype = {name: dt for name, dt, _ in _chunks(data)[0].schema}[column]
    render = Histogram(column)._render
    counts = {render(data, dtype, keys[i], reps[i]): int(cnts[i]) for i in range(got.value)}
    return _distribution(counts, state.numRows - state.frequencies.summary(state.numRows).num_values)


def build_cat_hist(data, columns: Sequence[str]):
    """One dq_cat_hist_build over `columns` (string / boolean): per column (status, n_null, counts, rep_rows) with
    status 0 ok / 1 over capacity (then no counts).  A hash collision raises what build_frequencies raises."""
    import numpy as np
    import torch

    chunks = _chunks(data)
    k = len(columns)
    schema = {name: dt for name, dt, _ in chunks[0].schema} if chunks else {}
    types = (ctypes.c_int32 * max(1, k))(*[L.TYPE_BOOL if schema[c] == "bool" else
                                           {"utf8": L.TYPE_UTF8, "large_utf8": L.TYPE_LARGE_UTF8}.get(schema[c], -1)
                                           for c in columns])
    for c, t in zip(columns, types):
        if t < 0:
            raise UnsupportedOnGpuPathException(f"histogram pass: column {c} is {schema[c]}, not a string or boolean column")
    views = (L.ColumnView * max(1, len(chunks) * k))()
    rows = (ctypes.c_int64 * max(1, len(chunks)))()
    for i, t in enumerate(chunks):
        rows[i] = t.num_rows
        for c, name in enumerate(columns):
            views[i * k + c] = t.columns[name].view()
    h = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib.dq_cat_hist_build(types, k, views, rows, len(chunks), torch.cuda.current_device(), stream,
                                    ctypes.byref(h)))
    out = []
    try:
        for c in range(k):
            status, nulls, nv = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
            L.check(L.lib.dq_cat_hist_column(h, c, ctypes.byref(status), ctypes.byref(nulls), ctypes.byref(nv)))
            counts = np.zeros(max(1, nv.value), dtype=np.int64)
            reps = np.zeros(max(1, nv.value), dtype=np.uint64)
            if status.value == 0:
                L.check(L.lib.dq_cat_hist_export(h, c, counts.ctypes.data_as(ctypes.c_void_p),
                                                 reps.ctypes.data_as(ctypes.c_void_p), max(1, nv.value)))
            out.append((status.value, nulls.value, counts[:nv.value], reps[:nv.value]))
    finally:
        L.lib.dq_cat_hist_destroy(h)
    return out


def compute_histograms(data, columns: Sequence[str]) -> Dict[str, Distribution]:
    """computeHistograms (:518-565) on the device: the Distribution of every target column from one fused pass (at
    most MAX_COLUMNS_PER_CALL columns per call); a column over the pass's capacity goes through build_frequencies and
    gives the same Distribution.  A dictionary-encoded column that build_frequencies groups on its indices
    (grouping.index_path_dictionaries) gets its Distribution from the entry counts (_indices_distribution: the same
    capacity rule over its distinct values, the same fallback), its strings are not decoded; any other dictionary
    column is read as the plain column it stands for."""
    from .grouping import index_path_dictionaries
    from .table import plain_utf8

    requested = list(columns)
    chunks = _chunks(data)
    on_indices = [c for c in requested if index_path_dictionaries(chunks, [c]) is not None]
    columns = [c for c in requested if c not in on_indices]
    data = plain_utf8(chunks, columns)
    chunks = _chunks(data)
    schema = {name: dt for name, dt, _ in chunks[0].schema} if chunks else {}
    out: Dict[str, Distribution] = {c: _indices_distribution(data, c) for c in on_indices}
    for b in range(0, len(columns), MAX_COLUMNS_PER_CALL):
        batch = columns[b:b + MAX_COLUMNS_PER_CALL]
        for name, (status, nulls, counts, reps) in zip(batch, build_cat_hist(data, batch)):
            if status != 0:
                out[name] = _fallback_distribution(data, name)
            elif schema[name] == "bool":
                out[name] = _distribution({"true" if int(r) else "false": int(c) for c, r in zip(counts, reps)}, nulls)
            else:
                out[name] = _distribution({_render_string(chunks, name, int(r)): int(c) for c, r in zip(counts, reps)},
                                          nulls)
    return {c: out[c] for c in requested}


def numeric_distributions(data, numeric: NumericColumnStatistics, columns: Sequence[str],
                          numberOfBuckets: int) -> Dict[str, Distribution]:
    """Per numeric column with a finite minimum < maximum: the Distribution of Histogram(column, binning =
    Bins.equal_width(minimum, maximum, numberOfBuckets)) over `data`, the columns pass 2 read (a numeric string column:
    its cast).  Every non-NULL value lies between the two, so the slots below and above stay empty; a column whose
    histogram fails is left out."""
    import math

    from .binning import Bins
    from .grouping import Histogram

    out: Dict[str, Distribution] = {}
    for name in columns:
        lo, hi = numeric.minima.get(name), numeric.maxima.get(name)
        if lo is None or hi is None or not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            continue
        try:
            bins = Bins.equal_width(lo, hi, numberOfBuckets)
        except ValueError:  # (the range is too narrow for that many distinct edges)
            continue
        metric = Histogram(name, binning=bins).calculate(data)
        if metric.value.isSuccess:
            out[name] = metric.value.get()
    return out


def create_profiles(columns: Sequence[str], generic: GenericColumnStatistics, numeric: NumericColumnStatistics,
                    histograms: Dict[str, Distribution],
                    distributions: Optional[Dict[str, Distribution]] = None) -> ColumnProfiles:
    """createProfiles (:617-670)."""
    profiles: Dict[str, ColumnProfile] = {}
    I = DataTypeInstances
    for name in columns:
        common = (name, generic.completenesses[name], generic.approximateNumDistincts[name], generic.typeOf(name),
                  name in generic.inferredTypes, generic.typeDetectionHistograms.get(name, {}), histograms.get(name))
        if generic.typeOf(name) in (I.Integral, I.Fractional):
            profiles[name] = NumericColumnProfile(*common, numeric.means.get(name), numeric.maxima.get(name),
                                                  numeric.minima.get(name), numeric.sums.get(name),
                                                  numeric.stdDevs.get(name), numeric.approxPercentiles.get(name),
                                                  (distributions or {}).get(name))
        else:
            profiles[name] = StandardColumnProfile(*common)
    return ColumnProfiles(profiles, generic.numRecords)


class ColumnProfiler:  # ColumnProfiler.scala:66-188
    DEFAULT_CARDINALITY_THRESHOLD = DEFAULT_CARDINALITY_THRESHOLD

    @staticmethod
    def profile(data, restrictToColumns: Optional[Sequence[str]] = None, printStatusUpdates: bool = False,
                lowCardinalityHistogramThreshold: int = DEFAULT_CARDINALITY_THRESHOLD, metricsRepository=None,
                reuseExistingResultsUsingKey=None, failIfResultsForReusingMissing: bool = False,
                saveInMetricsRepositoryUsingKey=None,
                numericDistributionBuckets: Optional[int] = None) -> ColumnProfiles:
        """numericDistributionBuckets (ColumnProfilerRunBuilder.withNumericDistributions; None: off): every numeric
        column with a finite minimum < maximum also gets `distribution`, that many equal-width bins between the two."""
        if numericDistributionBuckets is not None:
            from .binning import MAX_BINS

            if (not isinstance(numericDistributionBuckets, int) or isinstance(numericDistributionBuckets, bool)
                    or not 1 <= numericDistributionBuckets <= MAX_BINS):
                raise ValueError(f"numberOfBuckets = {numericDistributionBuckets!r}: an integer in 1..{MAX_BINS} is needed")
        if (metricsRepository is not None or reuseExistingResultsUsingKey is not None or failIfResultsForReusingMissing
                or saveInMetricsRepositoryUsingKey is not None):
            raise NotImplementedError("ColumnProfiler.profile: the metrics repository is not part of the GPU path")
        data = arrow_data(data)
        if not isinstance(data, Table):
            data = list(data)  # (an iterator of chunks is read once)
            if not data:
                raise ValueError("ColumnProfiler.profile: no chunks")
        schema = _chunks(data)[0].schema
        names = [name for name, _, _ in schema]
        for column in restrictToColumns or []:
            if column not in names:
                raise ValueError(f"requirement failed: Unable to find column {column}")
        relevant = [n for n in names if restrictToColumns is None or n in restrictToColumns]

        if printStatusUpdates:
            print("### PROFILING: Computing generic column statistics in pass (1/3)...")
        first = AnalysisRunner.onData(data).addAnalyzers(generic_stats_analyzers(schema, relevant) + [Size()]).run()
        generic = extract_generic_statistics(relevant, schema, first)

        if printStatusUpdates:
            print("### PROFILING: Computing numeric column statistics in pass (2/3)...")
        I = DataTypeInstances
        numeric_columns = [n for n in relevant if generic.typeOf(n) in (I.Integral, I.Fractional)]
        numeric = NumericColumnStatistics({}, {}, {}, {}, {}, {})
        distributions: Dict[str, Distribution] = {}
        if numeric_columns:
            # castNumericStringColumns: the string columns among them become i64 / f64; native ones are read as they are
            casted = cast_numeric_string_columns(data, {n: generic.typeOf(n) for n in numeric_columns})
            second = AnalysisRunner.onData(casted).addAnalyzers(second_pass_analyzers(numeric_columns)).run()
            numeric = extract_numeric_statistics(second)
            if numericDistributionBuckets is not None:
                distributions = numeric_distributions(casted, numeric, numeric_columns, numericDistributionBuckets)

        if printStatusUpdates:
            print("### PROFILING: Computing histograms of low-cardinality columns in pass (3/3)...")
        targets = find_target_columns_for_histograms(schema, generic, lowCardinalityHistogramThreshold)
        histograms = compute_histograms(data, targets) if targets else {}
        return create_profiles(relevant, generic, numeric, histograms, distributions)


class ColumnProfilerRunner:  # profiles/ColumnProfilerRunner.scala:42-48
    def onData(self, data) -> "ColumnProfilerRunBuilder":
        return ColumnProfilerRunBuilder(data)


class ColumnProfilerRunBuilder:  # profiles/ColumnProfilerRunBuilder.scala:27-105 (the options of the GPU path)
    def __init__(self, data):
        self.data = arrow_data(data)
        self._restrictToColumns: Optional[Sequence[str]] = None
        self._printStatusUpdates = False
        self._threshold = DEFAULT_CARDINALITY_THRESHOLD
        self._distribution_buckets: Optional[int] = None

    def restrictToColumns(self, columns: Sequence[str]) -> "ColumnProfilerRunBuilder":
        self._restrictToColumns = list(columns)
        return self

    def printStatusUpdates(self, on: bool) -> "ColumnProfilerRunBuilder":
        self._printStatusUpdates = on
        return self

    def withLowCardinalityHistogramThreshold(self, threshold: int) -> "ColumnProfilerRunBuilder":
        self._threshold = threshold
        return self

    def withNumericDistributions(self, numberOfBuckets: int = 100) -> "ColumnProfilerRunBuilder":
        """Opt in (default off): NumericColumnProfile.distribution, numberOfBuckets equal-width bins between a numeric
        column's minimum and maximum, counted in one device pass per column (Histogram's `binning`)."""
        self._distribution_buckets = numberOfBuckets
        return self

    def run(self) -> ColumnProfiles:
        return ColumnProfiler.profile(self.data, restrictToColumns=self._restrictToColumns,
                                      printStatusUpdates=self._printStatusUpdates,
                                      lowCardinalityHistogramThreshold=self._threshold,
                                      numericDistributionBuckets=self._distribution_buckets)
