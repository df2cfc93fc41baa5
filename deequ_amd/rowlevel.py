"""Row-level results: which rows pass each constraint and each check, as device bitmaps.

Deequ's VerificationResult.rowLevelResultsAsDataFrame gives one boolean column per check and per constraint; here the
same outcomes are bitmaps on the device (64-bit words, LSB first: the layout dq_take_index reads), so that "give me
the failing rows" is one schema.take_rows away.  The outcome of a constraint does not depend on its assertion, as
upstream: a row passes when the thing the metric counts holds for it.

  Completeness                      `col` IS NOT NULL
  Compliance (satisfies, ...)       the predicate is TRUE (NULL is not a pass)
  PatternMatch (hasPattern, ...)    regexp_extract(col, pattern, 0) != '' (a NULL value fails, as the metric counts it)
  Uniqueness (isUnique, ...)        the row's group has count 1 (a NULL key column: not unique)
  ReferentialIntegrity              the row's tuple is a key of the reference key set (a NULL key column: not contained)
  DatasetMatch                      the row equals the reference's row with the same key (a missing key: no match)

The first three run as row programs (dq_row_program_create / dq_row_outcomes: the predicate pass that stores rows
instead of counting them); Uniqueness probes the grouping's frequency table (dq_freq_unique_rows) and
ReferentialIntegrity the reference's key set (dq_freq_contains_rows, its `where` bitmap as the filter); DatasetMatch
looks its rows up there and compares them with the reference's (dq_freq_lookup_rows + dq_rows_match).  Every other
constraint has no row-level form and is listed in `skipped` with the reason; for a check's AND it counts as passing.
A predicate outside the GPU grammar is skipped the same way, with the compiler's reason -- never dropped silently.

Rows a constraint's `where` excludes: filteredRow="TRUE" (the default, as upstream) reports them as passing;
filteredRow="NULL" reports them as not applicable (the outcome carries an `applies` bitmap, as_bool a masked array).
A check's outcome is the AND of its constraints' outcomes with filtered rows passing; under "NULL" a row applies to
the check when it applies to at least one of its row-level constraints.

Planning (plan_row_level) runs on the host alone; evaluation takes a Table or a list of chunk Tables.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L
from .analyzers import Completeness, Compliance, PatternMatch, PlanBuilder
from .grouping import Uniqueness, _gpu_type, build_frequencies
from .matching import DatasetMatch, ReferentialIntegrity
from .metrics import NoSuchColumnException
from .predicates import UnsupportedPredicate
from .table import Table, plain_utf8

FILTERED_ROW = ("TRUE", "NULL")


def max_outputs() -> int:
    """Outputs, and distinct roots, one row program holds (dq_row_max_outputs: the device's kMaxRoots)."""
    return int(L.lib.dq_row_max_outputs())


@dataclass(frozen=True)
class RowForm:
    """The row-level form of one constraint.  kind "predicate": pred = ("sql", text) or ("regex", column, pattern),
    where = the `where` text or None.  kind "unique": columns = the grouping columns, where = the analyzer's filter
    (a selected row passes iff its tuple is unique among the selected rows).  kind "contains": analyzer =
    the ReferentialIntegrity analyzer (its columns, key set and `where`) or the DatasetMatch analyzer (pass = matched:
    the failing rows are the missing and the different ones)."""
    key: str
    kind: str
    pred: Optional[tuple] = None
    where: Optional[str] = None
    columns: Tuple[str, ...] = ()
    analyzer: object = None

    def roots(self) -> List[tuple]:
        return [self.pred] + ([("sql", self.where)] if self.where is not None else [])


def _quoted(column: str) -> str:
    return "`" + column.replace("`", "``") + "`"


def row_form(constraint) -> Union[RowForm, str]:
    """The row-level form of a constraint, or the reason it has none."""
    key = str(constraint)
    inner = getattr(constraint, "inner", constraint)
    analyzer = getattr(inner, "analyzer", None)
    if analyzer is None:
        return "not an analysis-based constraint"
    if key.startswith("AnomalyConstraint("):
        return "an anomaly check judges a metric against its history, not rows"
    if isinstance(analyzer, PatternMatch):
        return RowForm(key, "predicate", ("regex", analyzer.column, analyzer.pattern), analyzer.where)
    if isinstance(analyzer, Completeness):
        return RowForm(key, "predicate", ("sql", f"{_quoted(analyzer.column)} IS NOT NULL"), analyzer.where)
    if isinstance(analyzer, Compliance):
        return RowForm(key, "predicate", ("sql", analyzer.predicate), analyzer.where)
    if isinstance(analyzer, Uniqueness):
        return RowForm(key, "unique", where=analyzer.where, columns=tuple(analyzer.groupingColumns()))
    if isinstance(analyzer, ReferentialIntegrity):
        return RowForm(key, "contains", where=analyzer.where, columns=tuple(analyzer.columns), analyzer=analyzer)
    if isinstance(analyzer, DatasetMatch):
        return RowForm(key, "contains", where=analyzer.where, columns=tuple(analyzer.groupingColumns()),
                       analyzer=analyzer)
    return f"{type(analyzer).__name__} has no row-level form"


class RowProgram:
    """One dq_row_program over its own plan columns (host object; the device copy is made by its first evaluation)."""

    def __init__(self, forms: Sequence[RowForm], schema, expr_columns: Optional[dict] = None):
        self.forms = list(forms)
        b = PlanBuilder(schema, None, expr_columns)
        cache: Dict[tuple, int] = {}

        def root(r: tuple) -> int:
            if r not in cache:
                if r[0] == "regex":
                    from .table import type_code

                    col = b.col(r[1])
                    if type_code(b.by_name[r[1]][1]) not in (L.TYPE_UTF8, L.TYPE_LARGE_UTF8):
                        raise UnsupportedPredicate(f"PatternMatch on non-string column {r[1]} (Spark casts it to string)")
                    cache[r] = b.pool.add_regex(col, r[2], L.REGEX_EXTRACT_NONEMPTY)
                else:
                    cache[r] = b.pool.add(r[1])
            return cache[r]

        outs = (L.RowOutput * len(self.forms))()
        self.roots: List[Tuple[int, int]] = []  # (pred_root, where_root or -1) pool nodes per output
        for i, f in enumerate(self.forms):
            try:
                pr = root(f.pred)
                wr = -1 if f.where is None else root(("sql", f.where))
            except KeyError as e:  # the predicate compiler's "no such column"
                raise NoSuchColumnException(f"Input data does not include column {e.args[0]}!") from e
            outs[i].pred_root, outs[i].where_root = pr, wr
            self.roots.append((pr, wr))
        self.columns = list(b.columns)
        self.num_distinct_roots = len(cache)
        sch = b.schema_ctypes()
        pool, npred = b.pool.as_ctypes()
        pats, npats = b.pool.patterns_ctypes()
        self.handle = ctypes.c_void_p()
        status = L.lib.dq_row_program_create(sch, len(self.columns), pool, npred, pats, npats, outs, len(self.forms),
                                             ctypes.byref(self.handle))
        if status == L.DQ_E_UNSUPPORTED:
            raise UnsupportedPredicate(L.lib.dq_last_error().decode("utf-8", "replace"))
        L.check(status)

    def info(self) -> Tuple[int, int, int]:
        """(outputs, distinct roots after the library's deduplication, program instructions)."""
        a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        L.check(L.lib.dq_row_program_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def evaluate(self, table: Table, want_applies: Sequence[bool]):
        """One chunk: per output (pass bitmap, applies bitmap or None, num_pass, num_applies).  Bitmaps are device
        uint8 tensors of whole 64-bit words plus one zero word."""
        import torch

        n, words = table.num_rows, (table.num_rows + 63) // 64
        k = len(self.forms)
        views = (L.ColumnView * max(1, len(self.columns)))()
        for i, name in enumerate(self.columns):
            views[i] = table.columns[name].view()
        dev = torch.device("cuda", torch.cuda.current_device())
        for name in self.columns:
            dev = table.columns[name].values.device
            break
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        stream = torch.cuda.current_stream(dev).cuda_stream
        pass_t = [torch.zeros((words + 1) * 8, dtype=torch.uint8, device=dev) for _ in range(k)]
        app_t = [torch.zeros((words + 1) * 8, dtype=torch.uint8, device=dev) if w else None for w in want_applies]
        pp = (ctypes.c_void_p * k)(*[t.data_ptr() for t in pass_t])
        ap = (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in app_t])
        npass, napp = (ctypes.c_int64 * k)(), (ctypes.c_int64 * k)()
        L.check(L.lib.dq_row_outcomes(self.handle, views, n, pp, ap, index, ctypes.c_void_p(stream), npass, napp))
        return [(pass_t[i], app_t[i], int(npass[i]), int(napp[i])) for i in range(k)]

    def close(self) -> None:
        if getattr(self, "handle", None):
            L.lib.dq_row_program_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class RowLevelPlan:
    """What row_level_results will run: per check the keys of its row-level constraints, the form of every key, the
    row programs the predicate forms were split into, and the constraints without a row-level form."""
    checks: List[Tuple[str, List[str]]]
    forms: Dict[str, RowForm]
    programs: List[RowProgram]
    skipped: List[Tuple[str, str]]
    schema: list = field(default_factory=list)
    # canonical arithmetic expression -> the derived column the programs read (expressions.derived_schema); `schema`
    # holds those columns
    expr_columns: Dict[str, str] = field(default_factory=dict)

    def program_of(self, key: str) -> Tuple[int, int]:
        """(program, output) of a predicate form."""
        for p, prog in enumerate(self.programs):
            for i, f in enumerate(prog.forms):
                if f.key == key:
                    return p, i
        raise KeyError(key)

    def columns(self) -> List[str]:
        cols = [c for prog in self.programs for c in prog.columns]
        cols += [c for f in self.forms.values() for c in f.columns]
        return list(dict.fromkeys(cols))


def _plain_schema(schema):
    # a dictionary-encoded column is read by predicates and patterns as the plain string column it stands for
    return [(n, "utf8" if dt == "dict_utf8" else dt, nl) for n, dt, nl in schema]


def _split_programs(forms: List[RowForm], schema, cap: int, expr_columns: Optional[dict] = None) -> List[RowProgram]:
    """Greedy split: a program takes outputs while it holds at most `cap` outputs and `cap` distinct roots; a group
    the library still refuses for its size (program length, DFA budget, columns) is halved."""
    groups: List[List[RowForm]] = []
    cur: List[RowForm] = []
    roots: set = set()
    for f in forms:
        r = set(f.roots())
        if cur and (len(cur) + 1 > cap or len(roots | r) > cap):
            groups.append(cur)
            cur, roots = [], set()
        cur.append(f)
        roots |= r
    if cur:
        groups.append(cur)
    out: List[RowProgram] = []

    def build(group: List[RowForm]) -> None:
        try:
            out.append(RowProgram(group, schema, expr_columns))
        except UnsupportedPredicate:
            if len(group) == 1:
                raise
            build(group[:len(group) // 2])
            build(group[len(group) // 2:])

    for g in groups:
        build(g)
    return out


def _sql_texts(checks) -> List[str]:
    """The predicate and `where` texts of the checks' row-level forms."""
    out: List[str] = []
    for check in checks:
        for c in check.constraints:
            f = row_form(c)
            if isinstance(f, str):
                continue
            if f.kind == "predicate":
                out += [r[1] for r in f.roots() if r[0] == "sql"]
            elif f.kind in ("contains", "unique") and f.where is not None:
                out.append(f.where)
    return list(dict.fromkeys(out))


def plan_row_level(checks, schema, max_outputs_per_program: Optional[int] = None,
                   expr_columns: Optional[dict] = None) -> RowLevelPlan:
    """Host-only planning: which constraints get a row-level form, their keys and roots, the skipped ones with their
    reasons, and the split of the predicate forms into row programs.  Arithmetic operands of the predicates are
    planned as the derived columns an evaluation attaches for them (expr_columns: those the data carries already)."""
    from .expressions import derived_schema, text_expressions

    checks = list(checks)
    schema = _plain_schema(schema)
    schema, expr_columns = derived_schema(text_expressions(_sql_texts(checks), schema), schema, expr_columns)
    names = {c[0] for c in schema}
    cap = max_outputs() if max_outputs_per_program is None else min(int(max_outputs_per_program), max_outputs())
    per_check: List[Tuple[str, List[str]]] = []
    forms: Dict[str, RowForm] = {}
    skipped: List[Tuple[str, str]] = []
    for check in checks:
        keys: List[str] = []
        for c in check.constraints:
            f = row_form(c)
            key = str(c)
            if isinstance(f, str):
                skipped.append((key, f))
                continue
            if key not in forms:
                if f.kind == "unique":
                    missing = [x for x in f.columns if x not in names]
                    if missing:
                        skipped.append((key, f"NoSuchColumnException: Input data does not include column {missing[0]}!"))
                        continue
                    if f.where is not None:  # its `where` runs as a row program of its own (predicate_selection)
                        try:
                            RowProgram([RowForm(key, "predicate", ("sql", f.where))], schema, expr_columns).close()
                        except UnsupportedPredicate as e:
                            skipped.append((key, f"UnsupportedPredicate: {e}"))
                            continue
                        except NoSuchColumnException as e:
                            skipped.append((key, f"NoSuchColumnException: {e}"))
                            continue
                elif f.kind == "contains":
                    from .analyzers import Preconditions

                    err = Preconditions.findFirstFailing(schema, f.analyzer.preconditions())
                    if err is not None:
                        skipped.append((key, f"{type(err).__name__}: {err}"))
                        continue
                    if f.where is not None:  # its `where` runs as a row program of its own (predicate_bitmaps)
                        try:
                            RowProgram([RowForm(key, "predicate", ("sql", f.where))], schema, expr_columns).close()
                        except UnsupportedPredicate as e:
                            skipped.append((key, f"UnsupportedPredicate: {e}"))
                            continue
                        except NoSuchColumnException as e:
                            skipped.append((key, f"NoSuchColumnException: {e}"))
                            continue
                else:
                    try:  # alone first: what the GPU grammar (or the device stack) does not take is skipped, with the reason
                        RowProgram([f], schema, expr_columns).close()
                    except UnsupportedPredicate as e:
                        skipped.append((key, f"UnsupportedPredicate: {e}"))
                        continue
                    except NoSuchColumnException as e:
                        skipped.append((key, f"NoSuchColumnException: {e}"))
                        continue
                forms[key] = f
            keys.append(key)
        per_check.append((check.description, keys))
    programs = _split_programs([f for f in forms.values() if f.kind == "predicate"], schema, cap, expr_columns)
    return RowLevelPlan(per_check, forms, programs, skipped, list(schema), dict(expr_columns))


# ---- outcomes ------------------------------------------------------------------------------------------------------

_POPCOUNT = None


def _popcount(bitmap) -> int:
    import torch

    global _POPCOUNT
    if _POPCOUNT is None or _POPCOUNT.device != bitmap.device:
        _POPCOUNT = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=bitmap.device)
    return int(_POPCOUNT[bitmap.long()].sum().item())


def _row_mask(n: int, dev):
    """The bitmap of rows [0, n): whole words of ones, the last word's rows, one zero word."""
    import torch

    words = (n + 63) // 64
    m = torch.full((words + 1,), -1, dtype=torch.int64, device=dev)
    m[words] = 0
    if n % 64:
        v = (1 << (n % 64)) - 1
        m[words - 1] = v if v < (1 << 63) else v - (1 << 64)
    return m.view(torch.uint8)


def _words(b):
    import torch

    return b.view(torch.int64)


@dataclass
class ChunkOutcome:
    """One chunk of one outcome: `bitmap` bit r = row r passes (under filteredRow="TRUE" a filtered row passes; under
    "NULL" it does not and `applies` bit r is 0); `applies` None: every row applies."""
    bitmap: object
    applies: Optional[object]
    num_pass: int
    num_rows: int
    num_applies: int


class RowOutcome:
    def __init__(self, name: str, chunks: List[ChunkOutcome]):
        self.name, self.chunks = name, chunks

    @property
    def num_pass(self) -> int:
        return sum(c.num_pass for c in self.chunks)

    @property
    def num_rows(self) -> int:
        return sum(c.num_rows for c in self.chunks)

    @property
    def num_applies(self) -> int:
        return sum(c.num_applies for c in self.chunks)


def _bits(t, n: int) -> np.ndarray:
    return np.unpackbits(t.cpu().numpy(), bitorder="little")[:n].astype(bool)


class RowLevelResults:
    """Outcomes by constraint string and by check description, over the chunks they were computed from."""

    def __init__(self, data, filteredRow: str, constraints: Dict[str, RowOutcome], checks: Dict[str, RowOutcome],
                 skipped: List[Tuple[str, str]], plan: RowLevelPlan):
        self._single = isinstance(data, Table)
        self._chunks = [data] if self._single else list(data)
        self.filteredRow = filteredRow
        self.constraints, self.checks, self.skipped, self.plan = constraints, checks, skipped, plan

    def outcome(self, name: Optional[str] = None) -> RowOutcome:
        """A constraint's or a check's outcome; None: all checks ANDed."""
        if name is None:
            return _and_outcomes("*", list(self.checks.values()), self._chunks)
        if name in self.constraints:
            return self.constraints[name]
        if name in self.checks:
            return self.checks[name]
        raise KeyError(name)

    def as_bool(self, name: Optional[str] = None):
        """bool[numRows] over all chunks; under filteredRow="NULL" a masked array whose filtered rows are masked."""
        o = self.outcome(name)
        vals = np.concatenate([_bits(c.bitmap, c.num_rows) for c in o.chunks]) if o.chunks else np.zeros(0, bool)
        if self.filteredRow != "NULL":
            return vals
        app = [np.ones(c.num_rows, bool) if c.applies is None else _bits(c.applies, c.num_rows) for c in o.chunks]
        return np.ma.masked_array(vals, mask=~np.concatenate(app) if app else np.zeros(0, bool))

    def _take(self, name: Optional[str], passing: bool):
        from .schema import take_rows

        o = self.outcome(name)
        out = []
        for t, c in zip(self._chunks, o.chunks):
            if passing:
                sel, cnt = c.bitmap, c.num_pass
            else:  # the rows that apply and do not pass
                base = _row_mask(c.num_rows, c.bitmap.device) if c.applies is None else c.applies
                sel = (_words(base) & ~_words(c.bitmap)).view(c.bitmap.dtype)
                cnt = c.num_applies - c.num_pass
            out.append(take_rows(plain_utf8(t), sel, cnt))
        return out[0] if self._single else out

    def passing_rows(self, name: Optional[str] = None):
        """The rows that pass, in source order, as a Table (a list of Tables for chunked data)."""
        return self._take(name, True)

    def failing_rows(self, name: Optional[str] = None):
        """The rows that apply and do not pass, in source order."""
        return self._take(name, False)


def _and_outcomes(name: str, parts: List[RowOutcome], chunks: List[Table]) -> RowOutcome:
    """AND of outcomes with filtered rows passing; a row applies when it applies to one of them (none: all rows pass)."""
    import torch

    out = []
    for k, t in enumerate(chunks):
        n = t.num_rows
        cs = [p.chunks[k] for p in parts]
        dev = cs[0].bitmap.device if cs else torch.device("cuda", torch.cuda.current_device())
        mask = _words(_row_mask(n, dev))
        acc = mask.clone()
        app = None
        for c in cs:
            if c.applies is None:
                acc &= _words(c.bitmap)
                app = mask
            else:
                acc &= _words(c.bitmap) | (~_words(c.applies) & mask)
                app = _words(c.applies).clone() if app is None else (app | _words(c.applies))
        applies = None if app is None or app is mask else app.view(torch.uint8)
        if applies is not None:
            acc_report = acc & _words(applies)
        else:
            acc_report = acc
        # (filteredRow="TRUE" chunks carry no applies, so acc_report is acc there)
        bitmap = acc_report.view(torch.uint8)
        out.append(ChunkOutcome(bitmap, applies, _popcount(bitmap), n, n if applies is None else _popcount(applies)))
    return RowOutcome(name, out)


def _unique_outcome(form: RowForm, chunks: List[Table], null_mode: bool = False) -> RowOutcome:
    """pass = the row's tuple occurs once (among the selected rows, under a `where`: the frequencies are built from
    them and dq_freq_unique_rows_where leaves the unselected rows' bits 0); applies = the `where` bitmap."""
    import torch

    from .grouping import selection_of

    cols = list(form.columns)
    selection = selection_of(chunks, form.where, form.key)
    state = build_frequencies(chunks, cols, form.where, form.key, None if selection is None else {form.where: selection})
    probe = plain_utf8(chunks, cols)
    out = []
    for k, t in enumerate(probe):
        n, words = t.num_rows, (t.num_rows + 63) // 64
        dev = t.columns[cols[0]].values.device
        bitmap = torch.zeros((words + 1) * 8, dtype=torch.uint8, device=dev)
        types = (ctypes.c_int32 * len(cols))(*[_gpu_type(t.columns[c].dtype) for c in cols])
        views = (L.ColumnView * len(cols))(*[t.columns[c].view() for c in cols])
        nu = ctypes.c_int64(0)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if selection is None:
                L.check(L.lib.dq_freq_unique_rows(state.frequencies.handle, types, views, n, bitmap.data_ptr(), None,
                                                  stream, ctypes.byref(nu), None))
            else:
                L.check(L.lib.dq_freq_unique_rows_where(state.frequencies.handle, types, views, n,
                                                        selection.bitmaps[k].data_ptr(), bitmap.data_ptr(), None,
                                                        stream, ctypes.byref(nu), None))
        if selection is None:
            out.append(ChunkOutcome(bitmap, None, nu.value, n, n))
        else:
            out.append(_filtered_outcome(bitmap, selection.bitmaps[k], nu.value, selection.counts[k], n, null_mode))
    return RowOutcome(form.key, out)


def _filtered_outcome(p, a, npass: int, napp: int, n: int, null_mode: bool) -> ChunkOutcome:
    """One chunk's outcome from a pass bitmap p and the `where` bitmap a (None: no `where`)."""
    if a is None:
        return ChunkOutcome(p, None, npass, n, n)
    if null_mode:
        return ChunkOutcome(p, a, npass, n, napp)
    # a filtered row passes
    b = (_words(p) | (~_words(a) & _words(_row_mask(n, p.device)))).view(p.dtype)
    return ChunkOutcome(b, None, npass + (n - napp), n, n)


def _contains_outcome(form: RowForm, chunks: List[Table], null_mode: bool) -> RowOutcome:
    """pass = contained (DatasetMatch: matched), applies = the `where` bitmap: one dq_freq_contains_rows (one
    dq_freq_lookup_rows and one dq_rows_match) per chunk."""
    res = form.analyzer.probe(chunks, want_applies=form.where is not None)
    return RowOutcome(form.key, [_filtered_outcome(*r, t.num_rows, null_mode) for t, r in zip(chunks, res)])


def _prepared(chunks: List[Table], texts: Sequence[str], compile):
    """(the chunks as row programs over `texts` read them, what `compile` made of them).  The derived columns of the
    texts' arithmetic operands are attached -- one per distinct expression, once per chunk, on tables of this call's
    own (outcomes and row takes refer to the caller's chunks) -- then compile(schema, expr_columns) -> (compiled, its
    RowPrograms) runs, and the dictionary-encoded columns the programs touch are replaced by their decoded columns;
    where that changes a column's type (large_utf8 entries) the programs are closed and compiled again."""
    from .expressions import attach_expression_columns, text_expressions

    pred_chunks, failed = attach_expression_columns(chunks, text_expressions(texts, chunks[0].schema))
    if failed:
        raise next(iter(failed.values()))
    compiled, programs = compile(pred_chunks[0].schema, pred_chunks[0].expr_columns)
    touched = {c for prog in programs for c in prog.columns}
    dict_cols = {n for n, dt, _ in chunks[0].schema if dt == "dict_utf8"} & touched
    if dict_cols:
        before = _plain_schema(pred_chunks[0].schema)
        pred_chunks = plain_utf8(pred_chunks, dict_cols)
        if before != list(pred_chunks[0].schema):  # (large_utf8 entries)
            for prog in programs:
                prog.close()
            compiled, programs = compile(pred_chunks[0].schema, pred_chunks[0].expr_columns)
    return pred_chunks, compiled


def predicate_bitmaps(chunks: List[Table], text: str) -> list:
    """Per chunk the bitmap of the rows for which the SQL predicate `text` is TRUE: a one-output row program, its
    arithmetic operands and dictionary columns handled as row_level_results handles them (_prepared).  A text outside
    the GPU grammar raises UnsupportedPredicate."""
    return [p[0] for p in predicate_selection(chunks, text)]


def predicate_selection(chunks: List[Table], text: str) -> list:
    """predicate_bitmaps with each bitmap's number of set bits: per chunk (bitmap, rows for which `text` is TRUE)."""
    form = RowForm(text, "predicate", ("sql", text))

    def compile_one(schema, expr_columns):
        prog = RowProgram([form], _plain_schema(schema), expr_columns)
        return prog, [prog]

    pred_chunks, prog = _prepared(chunks, [text], compile_one)
    try:
        res = [prog.evaluate(t, [False])[0] for t in pred_chunks]
        return [(r[0], r[2]) for r in res]
    finally:
        prog.close()


def row_level_results(checks, data, filteredRow: str = "TRUE") -> RowLevelResults:
    """Per-row outcomes of the checks' constraints over `data` (a Table or a list of chunk Tables)."""
    if filteredRow not in FILTERED_ROW:
        raise ValueError(f"filteredRow must be one of {FILTERED_ROW}")
    from .runner import arrow_data

    checks = list(checks)
    data = arrow_data(data)
    chunks = [data] if isinstance(data, Table) else list(data)
    if not chunks:
        raise ValueError("row_level_results: no chunks")
    def compile_plan(schema, expr_columns):
        plan = plan_row_level(checks, schema, expr_columns=expr_columns)
        return plan, plan.programs

    pred_chunks, plan = _prepared(chunks, _sql_texts(checks), compile_plan)
    null_mode = filteredRow == "NULL"
    constraints: Dict[str, RowOutcome] = {}
    try:
        for prog in plan.programs:
            want = [f.where is not None for f in prog.forms]
            per_chunk = [prog.evaluate(t, want) for t in pred_chunks]
            for i, f in enumerate(prog.forms):
                outs = []
                for t, res in zip(pred_chunks, per_chunk):
                    outs.append(_filtered_outcome(*res[i], t.num_rows, null_mode))
                constraints[f.key] = RowOutcome(f.key, outs)
    finally:
        for prog in plan.programs:
            prog.close()
    for key, f in plan.forms.items():
        if f.kind == "unique":
            # (a filtered one reads the chunks that carry its `where`'s derived columns)
            constraints[key] = _unique_outcome(f, chunks if f.where is None else pred_chunks, null_mode)
        elif f.kind == "contains":
            constraints[key] = _contains_outcome(f, pred_chunks, null_mode)  # (its `where`'s derived columns)
    per_check = {desc: _and_outcomes(desc, [constraints[k] for k in keys], chunks) for desc, keys in plan.checks}
    return RowLevelResults(data, filteredRow, constraints, per_check, list(plan.skipped), plan)
