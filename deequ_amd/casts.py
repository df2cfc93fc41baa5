"""The ColumnProfiler's numeric-string cast and its second pass (profiles/ColumnProfiler.scala:133-151, 219-235,
330-339, 399-417) on the device.

A string column that pass 1's DataType analyzer found Integral or Fractional is re-typed with Spark 2.2's
Cast(StringType -> LongType / DoubleType) -- dq_cast_utf8 (include/dqscan.h), which materialises the derived
column as `withColumn(... cast ...)` does -- and Minimum, Maximum, Mean, StandardDeviation, Sum and ApproxQuantiles
then read it as any other i64 / f64 column.  There is no host fallback: a cast the library rejects raises.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence, Union

from . import _lib as L
from .analyzers import (DataType, DataTypeInstances, Maximum, Mean, Minimum, StandardDeviation, Sum, determineType)
from .metrics import UnsupportedOnGpuPathException
from .quantiles import ApproxQuantiles
from .runner import AnalysisRunner, AnalyzerContext
from .table import Column, Table

_TARGETS = {"i64": L.TYPE_I64, "f64": L.TYPE_F64}
# castNumericStringColumns: Integral -> LongType, Fractional -> DoubleType (ColumnProfiler.scala:409-413)
_CAST_OF = {DataTypeInstances.Integral: "i64", DataTypeInstances.Fractional: "f64"}


def cast_column(col: Column, to: str) -> Column:
    """Cast(col, LongType | DoubleType) of a utf8 / large_utf8 column: a new i64 / f64 Column of the same name and
    length whose row is NULL where the source row is NULL or the cast fails (buffers padded as
    table.column_from_numpy pads them)."""
    import torch

    if to not in _TARGETS:
        raise ValueError(f"cast target {to!r}: expected 'i64' or 'f64'")
    if col.dtype not in ("utf8", "large_utf8"):
        raise TypeError(f"cast_column: column {col.name!r} is {col.dtype}, not a string column")
    n = col.n_rows
    dev = col.values.device
    # values: 8 n bytes rounded up to 16, + 16; validity: whole 64-bit words + 1 (table.pack_validity)
    # (the cast writes every value and every validity word of the n rows: only the padding is cleared)
    words = (n + 63) // 64
    values = torch.empty(max(16, (8 * n + 15) // 16 * 16 + 16), dtype=torch.uint8, device=dev)
    validity = torch.empty((words + 1) * 8, dtype=torch.uint8, device=dev)
    values[8 * n:].zero_()
    validity[8 * words:].zero_()
    view = col.view()
    if not col.nullable:
        view.validity = None
    nulls = ctypes.c_int64(0)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(dev).cuda_stream
    try:
        L.check(L.lib.dq_cast_utf8(col.type_code, ctypes.byref(view), n, _TARGETS[to], values.data_ptr(),
                                   validity.data_ptr(), index, stream, ctypes.byref(nulls)))
    except L.DQError as e:
        if e.status == L.DQ_E_UNSUPPORTED:
            raise UnsupportedOnGpuPathException(e.message) from e
        raise
    return Column(col.name, to, n, values, validity, None, nullable=True)


def cast_numeric_string_columns(data: Union[Table, Sequence[Table]], inferred: Dict[str, str]):
    """castNumericStringColumns over a Table or a list of chunk Tables: every string column whose inferred type
    (DataTypeHistogram.determineType) is Integral becomes i64, Fractional f64; the others and the column order are
    kept (castColumn's withColumn / drop / rename keeps the name; the order is kept here for every column)."""
    from .table import plain_utf8

    # (a dictionary-encoded column that is cast is read as the plain column it stands for; the others stay encoded)
    data = plain_utf8(data, [n for n, t in inferred.items() if _CAST_OF.get(t)])

    def one(t: Table) -> Table:
        cols = []
        for c in t.columns.values():
            to = _CAST_OF.get(inferred.get(c.name))
            cols.append(cast_column(c, to) if to and c.dtype in ("utf8", "large_utf8") else c)
        return Table(cols)

    return one(data) if isinstance(data, Table) else [one(t) for t in data]


def inferred_types(pass1_context: AnalyzerContext) -> Dict[str, str]:
    """extractGenericStatistics' inferredTypes (ColumnProfiler.scala:352-356): determineType of every successful
    DataType metric of the first pass."""
    out = {}
    for a, m in pass1_context.metricMap.items():
        if isinstance(a, DataType) and m.value.isSuccess:
            out[a.column] = determineType(m.value.get())
    return out


def second_pass_analyzers(columns: Sequence[str]) -> List:
    """getAnalyzersForSecondPass (ColumnProfiler.scala:219-235) for the numeric columns given."""
    percentiles = [i / 100 for i in range(1, 101)]
    out = []
    for name in columns:
        out += [Minimum(name), Maximum(name), Mean(name), StandardDeviation(name), Sum(name),
                ApproxQuantiles(name, percentiles)]
    return out


def profile_pass2(data: Union[Table, Sequence[Table]], pass1_context: AnalyzerContext) -> AnalyzerContext:
    """Pass 2 of ColumnProfiler.profile for the string columns pass 1 typed: determineType on the DataType metrics,
    the cast, then getAnalyzersForSecondPass's analyzers in one AnalysisRunner run over the cast data."""
    inferred = inferred_types(pass1_context)
    if not isinstance(data, Table):
        data = list(data)  # (an iterator of chunks is read once)
        if not data:
            raise ValueError("profile_pass2: no chunks")
    first = data if isinstance(data, Table) else data[0]
    numeric = [name for name in first.columns if inferred.get(name) in _CAST_OF]
    casted = cast_numeric_string_columns(data, inferred)
    return AnalysisRunner.onData(casted).addAnalyzers(second_pass_analyzers(numeric)).run()
