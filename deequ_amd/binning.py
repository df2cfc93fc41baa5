"""Declared numeric bins: the declarative stand-in for Histogram's binning UDF.

A `Bins` is k + 1 finite, strictly increasing binary64 edges giving k bins (1 <= k <= 4096), and optionally a label
per bin.  The slot of a value is decided after conversion to binary64 as Spark's cast does it (f32 widens exactly,
integers round to nearest-even, a decimal is the correctly rounded quotient), with e the stored edges:

    e[i] <= x < e[i+1]            bin i
    x == e[k]                     the last bin, which is closed on the right
    x < e[0], including -inf      below
    x > e[k], including +inf      above
    NaN                           nan

-0.0 compares as 0.0.  NULL rows are in no slot.  The bin of a value is defined only by comparisons against the stored
edges, never by a division.  The counting itself is dq_bin_count (csrc/dq_bin.hip): one pass over the column.
"""
from __future__ import annotations

import ctypes
import json
import math
from typing import List, Optional, Sequence

from . import _lib as L

MAX_BINS = 4096


class Bins:
    """Immutable, hashable; equal when edges and labels are equal.  Build one with Bins.edges or Bins.equal_width.

    bin_edges: the k + 1 edges (floats; an edge -0.0 is stored as 0.0, which it compares as).
    bin_labels: the k labels given, or None for the default ones.
    slot_labels(): the k + 3 labels in dq_bin_count's slot order [below, bin 0 .. bin k-1, above, nan]."""

    __slots__ = ("bin_edges", "bin_labels")

    def __init__(self, edges: Sequence[float], labels: Optional[Sequence[str]] = None):
        try:
            given = list(edges)
        except TypeError:
            raise ValueError("edges: a sequence of numbers is needed") from None
        k = len(given) - 1
        if k < 1:
            raise ValueError(f"edges: at least 2 edges (1 bin) are needed, got {len(given)}")
        if k > MAX_BINS:
            raise ValueError(f"edges: {k} bins, at most {MAX_BINS}")
        out: List[float] = []
        for i, e in enumerate(given):
            try:
                f = float(e)
            except (TypeError, ValueError, OverflowError):
                raise ValueError(f"edges[{i}] is not finite") from None
            if not math.isfinite(f):
                raise ValueError(f"edges[{i}] is not finite")
            if i > 0 and not f > out[-1]:
                raise ValueError(f"edges[{i}] is not greater than edges[{i - 1}]")
            out.append(f + 0.0)  # (-0.0 -> 0.0)
        if labels is not None:
            labels = list(labels)
            if len(labels) != k:
                raise ValueError(f"labels: {len(labels)} labels for {k} bins")
            for i, s in enumerate(labels):
                if not isinstance(s, str):
                    raise ValueError(f"labels[{i}] is not a string")
        object.__setattr__(self, "bin_edges", tuple(out))
        object.__setattr__(self, "bin_labels", None if labels is None else tuple(labels))

    @staticmethod
    def edges(edges: Sequence[float], labels: Optional[Sequence[str]] = None) -> "Bins":
        return Bins(edges, labels)

    @staticmethod
    def equal_width(lo: float, hi: float, n: int) -> "Bins":
        """n bins between lo and hi: the edges lo + i * ((hi - lo) / n) for i < n, computed once here, and hi itself
        as the last one.  From there it is Bins.edges: no division decides a value's bin."""
        if not isinstance(n, int) or isinstance(n, bool) or n < 1:
            raise ValueError(f"equal_width: n = {n!r} is not a positive integer")
        if n > MAX_BINS:
            raise ValueError(f"edges: {n} bins, at most {MAX_BINS}")
        lo, hi = float(lo), float(hi)
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"edges[{0 if not math.isfinite(lo) else n}] is not finite")
        width = (hi - lo) / n
        return Bins([lo + i * width for i in range(n)] + [hi])

    def __setattr__(self, name, value):
        raise AttributeError("Bins is immutable")

    def __delattr__(self, name):
        raise AttributeError("Bins is immutable")

    @property
    def num_bins(self) -> int:
        return len(self.bin_edges) - 1

    def __eq__(self, other):
        return isinstance(other, Bins) and self.bin_edges == other.bin_edges and self.bin_labels == other.bin_labels

    def __hash__(self):
        return hash((self.bin_edges, self.bin_labels))

    def __str__(self):
        """Deterministic from edges and labels (it is part of str(Histogram), which names the persisted state): the
        edges as java.lang.Double.toString, shortest round-trip digits, so distinct edges print distinctly."""
        from .grouping import _java_double_to_string

        edges = ", ".join(_java_double_to_string(e) for e in self.bin_edges)
        labels = "None" if self.bin_labels is None else json.dumps(list(self.bin_labels), ensure_ascii=True)
        return f"Bins(edges=[{edges}],labels={labels})"

    __repr__ = __str__

    def slot_labels(self) -> List[str]:
        from .grouping import _java_double_to_string

        e = [_java_double_to_string(x) for x in self.bin_edges]
        k = self.num_bins
        if self.bin_labels is not None:
            bins = list(self.bin_labels)
        else:
            bins = [f"[{e[i]}, {e[i + 1]})" for i in range(k - 1)] + [f"[{e[k - 1]}, {e[k]}]"]
        return [f"< {e[0]}"] + bins + [f"> {e[k]}", "NaN"]


class _DeviceBins:
    """Owner of a dq_bins handle (the edges on the device)."""

    def __init__(self, bins: Bins, device: int):
        arr = (ctypes.c_double * len(bins.bin_edges))(*bins.bin_edges)
        self.handle = ctypes.c_void_p()
        L.check(L.lib.dq_bins_create(arr, len(bins.bin_edges), device, ctypes.byref(self.handle)))

    def close(self):
        if self.handle:
            L.lib.dq_bins_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def bin_counts(chunks, column: str, bins: Bins, selection=None):
    """The int64[k + 3] device tensor of slot counts of `column` over the chunks: one dq_bin_count per chunk into one
    array.  selection (a grouping.Selection): only its rows are counted (dq_bin_count_where), and the result is
    (counts, the number of selected rows as the kernel counted them)."""
    import torch

    from .grouping import _gpu_type

    dev = torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    counts = torch.zeros(bins.num_bins + 3, dtype=torch.int64, device=f"cuda:{dev}")
    n_selected = None if selection is None else torch.zeros(1, dtype=torch.int64, device=f"cuda:{dev}")
    with _DeviceBins(bins, dev) as d:
        for k, t in enumerate(chunks):
            col = t.columns[column]
            view = col.view()
            if selection is None:
                L.check(L.lib.dq_bin_count(d.handle, _gpu_type(col.dtype), ctypes.byref(view), t.num_rows,
                                           counts.data_ptr(), dev, stream))
            else:
                L.check(L.lib.dq_bin_count_where(d.handle, _gpu_type(col.dtype), ctypes.byref(view), t.num_rows,
                                                 selection.bitmaps[k].data_ptr(), counts.data_ptr(),
                                                 n_selected.data_ptr(), dev, stream))
    return counts if selection is None else (counts, int(n_selected.item()))


def binned_frequencies(chunks, column: str, bins: Bins, selection=None):
    """The FrequenciesAndNumRows of `column` binned by `bins`: the slot counts (bin_counts) as the weights of a small
    utf8 table of the k + 3 slot labels (dq_freq_build_weighted).  A slot no row fell into makes no group, slots of
    equal labels make one; numRows counts every row, so the NULLs are numRows minus the table's values.  The state's
    representative rows point into the label table, which is its source.  selection: the rows that are the data;
    numRows is their number."""
    import torch

    from .grouping import FreqTable, FrequenciesAndNumRows, _views
    from .table import Table, utf8_column

    dev = torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if selection is None:
        counts, num_rows = bin_counts(chunks, column, bins), sum(t.num_rows for t in chunks)
    else:
        counts, num_rows = bin_counts(chunks, column, bins, selection)
    labels = [s.encode("utf-8") for s in bins.slot_labels()]
    entries = [Table([utf8_column(column, labels, device=f"cuda:{dev}", nullable=False)])]
    types = (ctypes.c_int32 * 1)(L.TYPE_UTF8)
    views, rows = _views(entries, [column])
    weights = (ctypes.c_void_p * 1)(counts.data_ptr())
    h = ctypes.c_void_p()
    L.check(L.lib.dq_freq_build_weighted(types, 1, views, rows, weights, 1, dev, stream, ctypes.byref(h)))
    return FrequenciesAndNumRows(FreqTable(h, [L.TYPE_UTF8]), num_rows, source=(entries, [column]))


def bins_to_json(bins: Bins) -> dict:
    """The repository's "binning" member: the edges as floats (written as java.lang.Double.toString: they read back
    bit for bit) and the labels or null."""
    return {"edges": list(bins.bin_edges), "labels": None if bins.bin_labels is None else list(bins.bin_labels)}


def bins_from_json(node: dict) -> Bins:
    labels = node.get("labels")
    return Bins([float(e) for e in node["edges"]], labels)
