"""Segmented metrics: the scan analyzers per group of a key column.

"In which country is the completeness of `email` bad?", Mean(amount) per merchant, Compliance("price >= 0") per feed
partition: one run gives every metric once per segment -- per distinct tuple of the segment columns -- instead of one
filtered analyzer per segment value.

    ctx = AnalysisRunner.onData(data).segmentBy("country").addAnalyzer(Completeness("email")).run()
    ctx.segments, ctx.values(Completeness("email"))

The defining rule (tests/segment_ref.py restates it, tests/test_segment_gpu.py pins it): the metric of analyzer A for
segment s is the metric A gives on the table that holds exactly the rows of s.  Segments are the distinct tuples of the
segment columns over ALL rows, never over an analyzer's `where`; a segment in which a filtered analyzer has no applying
row gets that analyzer's usual empty-state failure and still exists.  Rows with a NULL in any segment column form the
single trailing segment None (this project's semantics: SQL's GROUP BY would make one group per NULL pattern).

How: once per run grouping.build_frequencies over the segment columns and a matching.KeySet of it; per chunk one
dq_freq_lookup_rows (the segment of every row), one dq_segment_order (the rows sorted by segment: `order_calls`
counts them) shared by every analyzer, and one dq_segment_scan per 64 slots (csrc/dq_segment.hip: a slot is a column
or predicate bitmap under an optional `where` bitmap).  Each distinct `where` / predicate text becomes bitmaps once per
run.  The chunks' per-segment states merge in chunk order with the column scan's algebra, vectorised over the
segments; the metrics are arrays over the segments.

Supported: Size, Completeness, Compliance, Sum, Mean, StandardDeviation, Minimum, Maximum, each with its `where`.
Completeness reads validity only and takes any column type; the others take f64 / f32 / i64 / i32 / i16 / i8 /
date32 / timestamp columns that pass their own preconditions.  Any other analyzer, and a decimal column under
anything but Completeness, is a Failure metric in every segment, decided before any launch.

Not done: grouping, distinct-count and quantile analyzers per segment; persisted or incremental segmented states; the
multi-GPU combine; the metrics repository; anomaly checks per segment; row-level results per segment.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from . import _lib as L
from .analyzers import (Analyzer, Completeness, Compliance, Maximum, Mean, Minimum, Preconditions, Size,
                        StandardDeviation, Sum, data_schema)
from .metrics import DoubleMetric, EmptyStateException, Success, UnsupportedOnGpuPathException
from .table import Table, decimal_ps, decoded

TILE = int(L.lib.dq_segment_tile())  # rows of a reduction tile (DQ_SEGMENT_TILE): tests place their sizes around it
MAX_SLOTS = L.SEGMENT_MAX_SLOTS
SUPPORTED = (Size, Completeness, Compliance, Sum, Mean, StandardDeviation, Minimum, Maximum)
STATS_DTYPES = ("f64", "f32", "i64", "i32", "i16", "i8", "date32", "timestamp")
_STATE = np.dtype(L.SEGMENT_STATE_FIELDS)

order_calls = 0  # dq_segment_order launches of the process (tests count them, as matching.lookup_calls)
scan_calls = 0   # dq_segment_scan launches of the process


class UnsupportedInSegmentedRunException(UnsupportedOnGpuPathException):
    """The analyzer, or its column's type, has no segmented form."""


def unsupported_reason(analyzer: Analyzer, schema) -> Optional[Exception]:
    """Why `analyzer` cannot run per segment over data with `schema`, or None.  Host only."""
    if type(analyzer) not in SUPPORTED:
        return UnsupportedInSegmentedRunException(
            f"{analyzer} is not supported in segmented runs (supported: {', '.join(c.__name__ for c in SUPPORTED)})")
    err = Preconditions.findFirstFailing(schema, analyzer.preconditions())
    if err is not None:
        return err
    column = getattr(analyzer, "column", None)
    if column is not None and not isinstance(analyzer, Completeness):
        dtype = {c[0]: c[1] for c in schema}[column]
        if decimal_ps(dtype) or dtype not in STATS_DTYPES:
            return UnsupportedInSegmentedRunException(
                f"type {dtype} of column {column} is not supported in segmented runs under {analyzer.name} "
                f"(supported: {', '.join(STATS_DTYPES)}; Completeness takes any type)")
    return None


def _key_set(chunks: List[Table], columns: List[str]):
    """(KeySet of the segment columns, its number of keys, whether a row has a NULL key): one build_frequencies."""
    from .grouping import build_frequencies
    from .matching import KeySet

    state = build_frequencies(chunks, columns).materialize()
    ks = KeySet(state.frequencies, columns)
    G = ks.num_keys
    keyed = int(state.frequencies.summary(max(1, state.numRows)).num_values) if G else 0
    return ks, G, keyed < state.numRows


def _stream():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def segment_order(seg, n_rows: int, G: int):
    """dq_segment_order of one chunk: (perm int32[n_rows], offsets int64[G + 2]), device tensors."""
    global order_calls
    import torch

    perm = torch.empty(max(1, n_rows), dtype=torch.int32, device=seg.device)
    offsets = torch.zeros(G + 2, dtype=torch.int64, device=seg.device)
    with torch.cuda.device(seg.device):
        order_calls += 1
        L.check(L.lib.dq_segment_order(seg.data_ptr(), n_rows, G, perm.data_ptr(), offsets.data_ptr(), _stream()))
    return perm, offsets


def segment_scan(slots: Sequence[L.SegmentSlot], perm, offsets, G1: int) -> np.ndarray:
    """dq_segment_scan over any number of slots (split into launches of MAX_SLOTS): a (len(slots), G1) record array of
    dq_segment_state."""
    global scan_calls
    import torch

    out = np.empty((len(slots), G1), dtype=_STATE)
    with torch.cuda.device(perm.device):
        for lo in range(0, len(slots), MAX_SLOTS):
            part = slots[lo:lo + MAX_SLOTS]
            arr = (L.SegmentSlot * len(part))(*part)
            dev = torch.empty(len(part) * G1 * _STATE.itemsize, dtype=torch.uint8, device=perm.device)
            scan_calls += 1
            L.check(L.lib.dq_segment_scan(arr, len(part), perm.data_ptr(), offsets.data_ptr(), G1, dev.data_ptr(),
                                          _stream()))
            out[lo:lo + len(part)] = dev.cpu().numpy().view(_STATE).reshape(len(part), G1)
    return out


def _min_of(a, b):
    return np.where((a < b) | ((a == b) & np.signbit(a)), a, b)  # (-0.0 below 0.0, as v_min_f64)


def _max_of(a, b):
    return np.where((a > b) | ((a == b) & ~np.signbit(a)), a, b)


def merge_states(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a (+) b per element: the column scan's merge of two partials (csrc/dq_colstats.h stats_merge), vectorised.  An
    empty state (n = 0, count = 0) is neutral."""
    o = a.copy()
    with np.errstate(all="ignore"):
        n = a["n"] + b["n"]
        both, only_b = (a["n"] != 0) & (b["n"] != 0), (a["n"] == 0) & (b["n"] != 0)
        delta = b["mean"] - a["mean"]
        r = np.where(both, b["n"] / np.where(n == 0, 1.0, n), 0.0)
        o["mean"] = np.where(both, a["mean"] + delta * r, np.where(only_b, b["mean"], a["mean"]))
        o["m2"] = np.where(both, a["m2"] + b["m2"] + delta * delta * a["n"] * r, np.where(only_b, b["m2"], a["m2"]))
        o["n"] = n
        o["sum"] = a["sum"] + b["sum"]
        o["isum"] = (a["isum"].view(np.uint64) + b["isum"].view(np.uint64)).view(np.int64)  # wrapping
        for f in ("count", "nan_count", "pinf_count", "ninf_count", "applies"):
            o[f] = a[f] + b[f]
        o["fmin"], o["fmax"] = _min_of(a["fmin"], b["fmin"]), _max_of(a["fmax"], b["fmax"])
    return o


def empty_states(shape) -> np.ndarray:
    s = np.zeros(shape, dtype=_STATE)
    s["fmin"], s["fmax"] = np.inf, -np.inf
    return s


class _Plan:
    """The slots of a run: each distinct (kind, validity source, filter source) once, and per analyzer which slots it
    reads.  A source is None, ("col", name), ("true", text) or ("nn", text) -- the rows where the text is TRUE / is
    not NULL."""

    def __init__(self):
        self.slots: List[tuple] = []
        self.index: Dict[tuple, int] = {}

    def slot(self, kind: str, source, filt) -> int:
        key = (kind, source, filt)
        if key not in self.index:
            self.index[key] = len(self.slots)
            self.slots.append(key)
        return self.index[key]

    def texts(self) -> List[tuple]:
        out = []
        for _, source, filt in self.slots:
            for s in (source, filt):
                if s is not None and s[0] in ("true", "nn") and s not in out:
                    out.append(s)
        return out

    def add(self, a: Analyzer, float_column: bool) -> dict:
        w = None if a.where is None else ("true", a.where)
        need = {"nn_where": None if a.where is None else self.slot("count", None, ("nn", a.where))}
        if isinstance(a, Size):
            need["main"] = None if a.where is None else self.slot("count", None, w)
        elif isinstance(a, Completeness):
            need["main"] = self.slot("count", ("col", a.column), w)
        elif isinstance(a, Compliance):
            need["main"] = self.slot("count", ("true", a.predicate), w)
            need["nn_pred"] = self.slot("count", ("nn", a.predicate), w)
        else:
            need["main"] = self.slot("stats", ("col", a.column), w)
            need["float"] = float_column
        return need


def _finish(a: Analyzer, need: dict, states: np.ndarray, rows: np.ndarray):
    """(values float64[S], empty bool[S]) of analyzer `a` from the merged states: dq_finish and dq_state_metric of the
    column scan, per segment."""
    S = len(rows)
    nn_where = states[need["nn_where"]]["applies"] > 0 if need["nn_where"] is not None else np.ones(S, dtype=bool)
    m = states[need["main"]] if need["main"] is not None else None
    with np.errstate(all="ignore"):
        if isinstance(a, Size):
            if m is None:
                return rows.astype(np.float64), np.zeros(S, dtype=bool)
            return m["applies"].astype(np.float64), ~nn_where
        if isinstance(a, (Completeness, Compliance)):
            cnt = m["applies"].astype(np.float64)
            v = np.where(cnt == 0, np.nan, m["count"].astype(np.float64) / np.where(cnt == 0, 1.0, cnt))
            defined = nn_where & (rows > 0)
            if isinstance(a, Compliance):
                defined = nn_where & (states[need["nn_pred"]]["count"] > 0)
            return v, ~defined
        count, empty = m["count"], m["count"] == 0
        if isinstance(a, (Sum, Mean)):
            if need["float"]:
                v = m["sum"].copy()
                v[m["pinf_count"] > 0] += np.inf
                v[m["ninf_count"] > 0] += -np.inf
            else:
                v = m["isum"].astype(np.float64)
            if isinstance(a, Mean):
                v = v / np.where(empty, 1, count).astype(np.float64)
            return v, empty
        if isinstance(a, StandardDeviation):
            n, m2 = m["n"].copy(), m["m2"].copy()
            pos = n > 0
            safe = np.where(pos, n, 1.0)
            m2 = np.where(pos, m2 + m["mean"] * (m["mean"] / safe) * 0.0 * n, m2)  # (dq_finish: Spark's zero-buffer merge)
            inf = m["pinf_count"] + m["ninf_count"] > 0
            n = np.where(inf, count.astype(np.float64), n)
            m2 = np.where(inf, np.nan, m2)
            return np.sqrt(m2 / np.where(n > 0, n, 1.0)), ~(n > 0)
        if isinstance(a, Minimum):
            return np.where(m["nan_count"] == count, np.nan, m["fmin"]), empty
        return np.where(m["nan_count"] > 0, np.nan, m["fmax"]), empty


class SegmentedAnalyzerContext:
    """The metrics of a segmented run: per analyzer one value per segment."""

    def __init__(self, columns: Sequence[str], key_set, G: int, rows: np.ndarray, analyzers: Sequence[Analyzer],
                 values: Dict[Analyzer, np.ndarray], empty: Dict[Analyzer, np.ndarray],
                 failed: Dict[Analyzer, BaseException]):
        self.columns = tuple(columns)
        self._key_set, self._G = key_set, G
        self.has_null_segment = bool(len(rows) > G)
        self.rows_per_segment = np.asarray(rows, dtype=np.int64)
        self.analyzers = list(analyzers)
        self._values, self._empty, self._failed = values, empty, failed
        self._segments: Optional[list] = None

    @property
    def num_segments(self) -> int:
        return len(self.rows_per_segment)

    @property
    def segments(self) -> list:
        """The key tuples in the key set's sorted order; a last entry None iff some row has a NULL segment key."""
        if self._segments is None:
            from .drift import _render_value

            out: List[Optional[tuple]] = []
            if self._G:
                table = self._key_set.table
                keys, _ = table.export()
                dtypes = self._key_set.dtypes
                if len(dtypes) == 1 and dtypes[0] not in ("utf8", "large_utf8") and not decimal_ps(dtypes[0]):
                    width = {"f32": 4, "i32": 4, "date32": 4, "i16": 2, "i8": 1, "bool": 1}.get(dtypes[0], 8)
                    mask = (1 << (8 * width)) - 1
                    out = [(_render_value(dtypes[0], (int(k) & mask).to_bytes(width, "little")),) for k in keys]
                else:
                    cols = [[_render_value(dt, raw) for raw in table.take_values(keys, c)] for c, dt in enumerate(dtypes)]
                    out = list(zip(*cols))
            self._segments = out + ([None] if self.has_null_segment else [])
        return self._segments

    def _index(self, segment) -> int:
        if isinstance(segment, (int, np.integer)) and not isinstance(segment, bool):
            if not -self.num_segments <= segment < self.num_segments:
                raise IndexError(f"segment {segment} of {self.num_segments}")
            return int(segment) % self.num_segments
        if segment is not None and not isinstance(segment, tuple):
            segment = (segment,)
        try:
            return self.segments.index(segment)
        except ValueError:
            raise KeyError(f"no segment {segment!r}") from None

    def _known(self, analyzer: Analyzer) -> Analyzer:
        if analyzer not in self._values and analyzer not in self._failed:
            raise KeyError(f"{analyzer} was not part of this run")
        return analyzer

    def values(self, analyzer: Analyzer) -> np.ndarray:
        """One metric per segment (NaN where failures() has an entry)."""
        a = self._known(analyzer)
        if a in self._failed:
            return np.full(self.num_segments, np.nan)
        return np.where(self._empty[a], np.nan, self._values[a])

    def _empty_state(self, a: Analyzer) -> BaseException:
        return EmptyStateException(f"Empty state for analyzer {a}, all input values were NULL.")

    def failures(self, analyzer: Analyzer) -> Dict[int, BaseException]:
        """{segment index: exception} of the segments whose metric is a Failure."""
        a = self._known(analyzer)
        if a in self._failed:
            return {i: self._failed[a] for i in range(self.num_segments)}
        return {int(i): self._empty_state(a) for i in np.flatnonzero(self._empty[a])}

    def metric(self, analyzer: Analyzer, segment) -> DoubleMetric:
        a, i = self._known(analyzer), self._index(segment)
        if a in self._failed:
            return a.toFailureMetric(self._failed[a])
        if self._empty[a][i]:
            return a.toFailureMetric(self._empty_state(a))
        return DoubleMetric(a.entity, a.name, a.instance, Success(float(self._values[a][i])))

    def context(self, segment):
        """An ordinary AnalyzerContext of one segment (its index, its key tuple, a single key value, or None)."""
        from .runner import AnalyzerContext

        i = self._index(segment)
        return AnalyzerContext({a: self.metric(a, i) for a in self.analyzers})

    def successMetricsAsRows(self) -> List[dict]:
        """AnalyzerContext.successMetricsAsJson's rows with the segment's values in front: per segment and successful
        metric {segment column: value, ..., entity, instance, name, value}; the None segment has None in every segment
        column."""
        out = []
        segs = self.segments
        for i in range(self.num_segments):
            key = dict(zip(self.columns, segs[i] if segs[i] is not None else (None,) * len(self.columns)))
            for a in self.analyzers:
                if a in self._failed or self._empty[a][i]:
                    continue
                out.append({**key, "entity": a.entity.value, "instance": a.instance, "name": a.name,
                            "value": float(self._values[a][i])})
        return out


def run_segmented(data, columns: Union[str, Sequence[str]], analyzers: Sequence[Analyzer],
                  maxSegments: Optional[int] = None) -> SegmentedAnalyzerContext:
    """Every analyzer once per distinct tuple of `columns` (the module docstring has the rule).  maxSegments: refuse,
    before any grouped launch, data with more segments (ValueError naming the count)."""
    from .matching import _lookup, where_bitmaps
    from .runner import _chunks, arrow_data

    columns = [columns] if isinstance(columns, str) else list(columns)
    if not columns:
        raise ValueError("At least one column needs to be specified!")
    data = arrow_data(data)
    schema = data_schema(data)
    for c in columns:
        Preconditions.hasColumn(c)(schema)
    analyzers = list(dict.fromkeys(analyzers))
    by_name = {c[0]: c[1] for c in schema}
    failed: Dict[Analyzer, BaseException] = {}
    plan, needs = _Plan(), {}
    for a in analyzers:
        err = unsupported_reason(a, schema)
        if err is not None:
            failed[a] = err
            continue
        column = getattr(a, "column", None)
        needs[a] = plan.add(a, column is not None and by_name[column] in ("f64", "f32"))
    chunks = _chunks(data)
    key_set, G, has_null = _key_set(chunks, columns)
    found = G + (1 if has_null else 0)
    if maxSegments is not None and found > maxSegments:
        raise ValueError(f"{found} segments of ({', '.join(columns)}) found, more than maxSegments = {maxSegments}")
    G1 = G + 1
    live = [t for t in chunks if t.num_rows > 0]
    # each distinct text once per run: the TRUE bitmaps, and for the counts that decide a NULL sum the NOT NULL ones
    # (TRUE or FALSE: the text's and its negation's TRUE rows)
    bitmaps: Dict[tuple, list] = {}
    bad_text: Dict[tuple, BaseException] = {}
    if live:
        for src in plan.texts():
            try:
                true = bitmaps.get(("true", src[1]))
                if true is None:
                    true = bitmaps[("true", src[1])] = where_bitmaps(live, src[1])
                if src[0] == "nn":
                    neg = where_bitmaps(live, f"NOT ({src[1]})")
                    bitmaps[src] = [t | f for t, f in zip(true, neg)]
            except Exception as e:
                bad_text[src] = e
    for a, need in list(needs.items()):
        used = [s for i in need.values() if isinstance(i, int) and not isinstance(i, bool)
                for s in plan.slots[i][1:] if s in bad_text]
        if used:
            failed[a] = bad_text[used[0]]
            del needs[a]
    states = empty_states((max(1, len(plan.slots)), G1))
    rows = np.zeros(G1, dtype=np.int64)
    keep = []  # (the tensors a launch reads stay alive until it returns)
    for k, t in enumerate(live):
        seg, _ = _lookup(key_set, t, columns)
        perm, offsets = segment_order(seg, t.num_rows, G)
        off = offsets.cpu().numpy()
        rows += off[1:] - off[:-1]
        slots = []
        for kind, source, filt in plan.slots:
            s = L.SegmentSlot()
            s.op = L.SEG_STATS if kind == "stats" else L.SEG_COUNT
            if source is not None and source[0] == "col":
                col = t.columns[source[1]]
                if kind == "stats":
                    s.col.values = col.values.data_ptr()
                    s.type = col.type_code
                else:
                    col = decoded(col)  # (a dictionary entry may be NULL: the decoded column's validity says so)
                    keep.append(col)
                s.col.validity = col.validity.data_ptr() if col.validity is not None else None
            elif source is not None:
                s.col.validity = bitmaps[source][k].data_ptr()
            if filt is not None:
                s.filter = bitmaps[filt][k].data_ptr()
            slots.append(s)
        if slots:
            states = merge_states(states, segment_scan(slots, perm, offsets, G1))
    S = G1 if rows[G] > 0 else G
    rows, states = rows[:S], states[:, :S]
    values, empty = {}, {}
    for a, need in needs.items():
        values[a], empty[a] = _finish(a, need, states, rows)
    return SegmentedAnalyzerContext(columns, key_set, G, rows, analyzers, values, empty, failed)


class SegmentedAnalysisRunBuilder:
    """AnalysisRunner.onData(data).segmentBy(columns): addAnalyzer(s), then run() -> SegmentedAnalyzerContext."""

    def __init__(self, data, columns, analyzers: Sequence[Analyzer] = (), maxSegments: Optional[int] = None):
        self.data, self.columns, self.maxSegments = data, columns, maxSegments
        self.analyzers: List[Analyzer] = list(analyzers)

    def addAnalyzer(self, a: Analyzer) -> "SegmentedAnalysisRunBuilder":
        self.analyzers.append(a)
        return self

    def addAnalyzers(self, analyzers) -> "SegmentedAnalysisRunBuilder":
        self.analyzers.extend(analyzers)
        return self

    def run(self) -> SegmentedAnalyzerContext:
        return run_segmented(self.data, self.columns, self.analyzers, self.maxSegments)


class SegmentedVerificationResult:
    """The checks of a run evaluated once per segment (a host loop over the segments)."""

    def __init__(self, checks, context: SegmentedAnalyzerContext):
        from .checks import CheckStatus

        self.checks = list(checks)
        self.context = context
        self._results = [{c: c.evaluate(context.context(i)) for c in self.checks} for i in range(context.num_segments)]
        self.status_by_segment = [CheckStatus(max((r.status for r in res.values()), default=CheckStatus.Success))
                                  for res in self._results]
        self.status = CheckStatus(max(self.status_by_segment, default=CheckStatus.Success))

    @property
    def segments(self) -> list:
        return self.context.segments

    def check_results(self, segment) -> dict:
        """{check: CheckResult} of one segment (index, key tuple, single key value or None)."""
        return self._results[self.context._index(segment)]

    def failing_segments(self, check=None) -> list:
        """The segments (as `segments` names them) in which `check` -- or any check -- is not a Success."""
        from .checks import CheckStatus

        segs = self.segments
        if check is None:
            return [segs[i] for i, s in enumerate(self.status_by_segment) if s != CheckStatus.Success]
        return [segs[i] for i, res in enumerate(self._results) if res[check].status != CheckStatus.Success]


class SegmentedVerificationRunBuilder:
    """VerificationSuite().onData(data).segmentBy(columns, maxSegments): addCheck(s), then run()."""

    def __init__(self, data, columns, maxSegments: int = 10000, checks=(), required=()):
        self.data, self.columns, self.maxSegments = data, columns, maxSegments
        self.checks, self.required = list(checks), list(required)

    def addCheck(self, check) -> "SegmentedVerificationRunBuilder":
        self.checks.append(check)
        return self

    def addChecks(self, checks) -> "SegmentedVerificationRunBuilder":
        self.checks.extend(checks)
        return self

    def addRequiredAnalyzer(self, a: Analyzer) -> "SegmentedVerificationRunBuilder":
        self.required.append(a)
        return self

    def run(self) -> SegmentedVerificationResult:
        analyzers = list(self.required) + [a for c in self.checks for a in c.requiredAnalyzers()]
        return SegmentedVerificationResult(self.checks, run_segmented(self.data, self.columns, analyzers, self.maxSegments))
