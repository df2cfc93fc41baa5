"""Arithmetic operands of predicates on the device: `a * b + c <= d`, `id % 2 = 0`, `a / b IS NULL`.

Spark evaluates such an operand as a derived expression under the comparison; here the predicate compiler turns it
into a postfix program (include/dqscan.h, dq_expr_program: the Spark 2.2 typing, wrapping, NULL and division rules),
dq_expr_eval materialises it once per chunk as an ordinary column -- as lengths.string_lengths does for length(col)
-- and the comparison reads that column, so the fused scan, the row programs and every comparison rule stay as they
are.  One derived column per distinct canonical expression of a run, however many predicates and `where`s use it,
under a reserved name no data column carries; Table.expr_columns maps canonical text to that name.  There is no host
fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

from . import _lib as L
from .metrics import UnsupportedOnGpuPathException
from .table import Column, Table

DTYPE_OF = {L.TYPE_I8: "i8", L.TYPE_I16: "i16", L.TYPE_I32: "i32", L.TYPE_I64: "i64", L.TYPE_F32: "f32",
            L.TYPE_F64: "f64"}
_SIZE = {"i8": 1, "i16": 2, "i32": 4, "i64": 8, "f32": 4, "f64": 8}

eval_calls = 0  # dq_expr_eval launches of the process (tests count them, as Dictionary.decode_calls)


@dataclass
class Expression:
    """One entry of a predicate pool's expression list: the canonical text, the program (a copy that outlives the
    pool), the names of its source columns in program order and the dtype of the derived column."""
    text: str
    program: L.ExprProgram
    columns: Tuple[str, ...]
    dtype: str

    @property
    def divides(self) -> bool:
        return bool(self.program.divides)

    def nullable(self, schema) -> bool:
        """The derived column is nullable whenever an input is, or when the program contains / or %."""
        by_name = {c[0]: c for c in schema}
        return self.divides or any(by_name[c][2] for c in self.columns)

    def instructions(self) -> List[Tuple[int, int, int]]:
        p = self.program
        return [(p.instrs[i].op, p.instrs[i].arg, p.instrs[i].type) for i in range(p.n_instrs)]

    def literals(self) -> List[Tuple[int, Union[int, float]]]:
        p = self.program
        return [(p.literals[i].type, p.literals[i].f64 if p.literals[i].type == L.TYPE_F64 else p.literals[i].i64)
                for i in range(p.n_literals)]


def expression_from_pool(handle, index: int, names: Sequence[str]) -> Expression:
    """Entry `index` of a C pool's expression list (dq_pred_pool_expr); names = the pool's column list."""
    ptr = L.lib.dq_pred_pool_expr(handle, index)
    if not ptr:
        raise IndexError(f"no expression {index} in the pool")
    text = ptr.contents.text.decode("utf-8")
    prog = L.ExprProgram.from_buffer_copy(ptr.contents)
    prog.text = None  # (the pool's string; the copy must not point into it)
    cols = tuple(names[prog.columns[k]] for k in range(prog.n_columns))
    return Expression(text, prog, cols, DTYPE_OF[prog.result_type])


# ------------------------------------------------------------------------------------------ collecting
def _collect(lower, schema) -> Dict[str, Expression]:
    from .analyzers import PlanBuilder

    b = PlanBuilder(schema, collect_exprs=True)
    try:
        lower(b)
    except Exception:  # refused or failing text: its analyzer is routed or fails its own way, later
        pass
    return dict(b.exprs)


def analyzer_expressions(analyzers: Sequence, schema) -> List[Dict[str, Expression]]:
    """Per analyzer, the expressions its predicate and `where` texts hold (canonical text -> Expression), found by
    lowering it alone on the host.  An analyzer whose text is refused, or that has no scan lowering, has none."""
    schema = _plain(schema)
    return [_collect(lambda b, a=a: a._lower(b), schema) for a in analyzers]


def text_expressions(texts: Iterable[str], schema) -> Dict[str, Expression]:
    """The expressions of predicate texts (row-level checks), each parsed alone: a refused text contributes none."""
    schema = _plain(schema)
    out: Dict[str, Expression] = {}
    for t in texts:
        for k, e in _collect(lambda b, t=t: b.pool.add(t), schema).items():
            out.setdefault(k, e)
    return out


def _plain(schema):
    return [(n, "utf8" if dt == "dict_utf8" else dt, nl) for n, dt, nl in schema]


def _merge(per: Iterable[Dict[str, Expression]]) -> Dict[str, Expression]:
    out: Dict[str, Expression] = {}
    for d in per:
        for k, e in d.items():
            out.setdefault(k, e)
    return out


# ------------------------------------------------------------------------------------------ naming, host-only schema
def expr_column_name(text: str, taken: Iterable[str]) -> str:
    """The name of the derived column of canonical expression `text`: "expr" + text, with underscores in front until
    no column of the data carries it (a predicate can only name columns of the data, so it cannot name this one)."""
    taken = set(taken)
    name = "expr" + text
    while name in taken:
        name = "_" + name
    return name


def derived_schema(exprs: Dict[str, Expression], schema, expr_columns: Optional[dict] = None):
    """(schema with one derived column per expression not yet in expr_columns, canonical text -> derived name): what
    attach_expression_columns would give for data of this schema, on the host alone -- for planning (runner.explain,
    runner.gpu_eligible, rowlevel.plan_row_level) without data."""
    schema = list(schema)
    names = dict(expr_columns or {})
    taken = {c[0] for c in schema}
    for text, e in exprs.items():
        if text in names and names[text] in taken:
            continue
        names[text] = expr_column_name(text, taken)
        taken.add(names[text])
        schema.append((names[text], e.dtype, e.nullable(schema)))
    return schema, names


def lowering_schema(analyzers: Sequence, schema, expr_columns: Optional[dict] = None):
    """derived_schema for the expressions of `analyzers`."""
    return derived_schema(_merge(analyzer_expressions(analyzers, schema)), schema, expr_columns)


# ------------------------------------------------------------------------------------------ evaluation
def _check(status: int) -> None:
    try:
        L.check(status)
    except L.DQError as e:
        if e.status == L.DQ_E_UNSUPPORTED:
            raise UnsupportedOnGpuPathException(e.message) from e
        raise


def _buffers(n: int, size: int, dev):
    """A column's buffers, padded as lengths._buffers pads them (values: size n bytes rounded up to 16, + 16;
    validity: whole 64-bit words + 1).  The kernel writes every value and every validity word of the n rows: only
    the padding is cleared."""
    import torch

    words = (n + 63) // 64
    values = torch.empty(max(16, (size * n + 15) // 16 * 16 + 16), dtype=torch.uint8, device=dev)
    validity = torch.empty((words + 1) * 8, dtype=torch.uint8, device=dev)
    values[size * n:].zero_()
    validity[8 * words:].zero_()
    return values, validity


def evaluate(e: Expression, table: Table, name: Optional[str] = None) -> Column:
    """The expression over one chunk: a new Column of its result dtype (dq_expr_eval), NULL where an input is NULL or
    a divisor is zero.  The source columns must be the fixed-width numeric columns the expression was compiled for."""
    global eval_calls
    import torch

    cols = [table.columns[c] for c in e.columns]
    for k, c in enumerate(cols):
        if c.type_code != e.program.column_types[k]:
            raise TypeError(f"expression {e.text}: column {c.name!r} is {c.dtype}, not the type it was compiled for")
    n = table.num_rows
    dev = cols[0].values.device
    values, validity = _buffers(n, _SIZE[e.dtype], dev)
    views = (L.ColumnView * len(cols))()
    for k, c in enumerate(cols):
        views[k] = c.view()
        if not c.nullable:
            views[k].validity = None
    nulls = ctypes.c_int64(0)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(dev).cuda_stream
    eval_calls += 1
    _check(L.lib.dq_expr_eval(ctypes.byref(e.program), views, n, values.data_ptr(), validity.data_ptr(), index,
                              stream, ctypes.byref(nulls)))
    nullable = e.divides or any(c.nullable for c in cols)
    out = Column(name or e.text, e.dtype, n, values, validity if nullable else None, None, nullable=nullable)
    out.null_count = nulls.value
    return out


def attach_expression_columns(data: Union[Table, Sequence[Table]], exprs: Dict[str, Expression]):
    """(`data` with one derived column attached to every chunk for each expression of `exprs` it does not carry yet,
    {canonical text: the exception} for the expressions whose evaluation failed).  New Tables that share the chunks'
    columns; Table.expr_columns maps canonical text to derived name.  Data that carries them all, or a run without
    expressions, comes back as it is."""
    failed: Dict[str, Exception] = {}
    if not exprs:
        return data, failed
    chunks = [data] if isinstance(data, Table) else list(data)
    if not chunks:
        return data, failed
    first = chunks[0]
    todo = [e for t, e in exprs.items() if t not in first.expr_columns]
    if not todo:
        return data, failed
    names: Dict[str, str] = dict(first.expr_columns)
    taken = set(first.columns)
    for e in todo:
        names[e.text] = expr_column_name(e.text, taken)
        taken.add(names[e.text])
    derived: List[List[Column]] = [[] for _ in chunks]
    for e in todo:
        try:
            cols = [evaluate(e, t, names[e.text]) for t in chunks]
        except Exception as ex:  # this expression alone: the analyzers that use it fail, the others run
            failed[e.text] = ex
            del names[e.text]
            continue
        # one nullability for all chunks (the plan's schema is the first chunk's)
        nullable = any(c.nullable for c in cols)
        for k, c in enumerate(cols):
            c.nullable = nullable
            derived[k].append(c)

    def one(t: Table, extra: List[Column]) -> Table:
        out = Table(list(t.columns.values()) + extra)
        out.length_columns = dict(t.length_columns)
        out.expr_columns = dict(names)
        return out

    out = [one(t, d) for t, d in zip(chunks, derived)]
    return (out[0] if isinstance(data, Table) else out), failed


def expr_columns_of(data) -> Dict[str, str]:
    """canonical text -> derived column of attached data ({} for data as the user built it)."""
    chunks = [data] if isinstance(data, Table) else list(data)
    return dict(chunks[0].expr_columns) if chunks else {}


def attach_for(data, analyzers: Sequence):
    """attach_expression_columns for the expressions of `analyzers`; -> (data, failed, per-analyzer expressions)."""
    chunks = [data] if isinstance(data, Table) else list(data)
    if not chunks:
        return data, {}, [{} for _ in analyzers]
    per = analyzer_expressions(analyzers, chunks[0].schema)
    data, failed = attach_expression_columns(data, _merge(per))
    return data, failed, per
