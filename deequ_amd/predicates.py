"""Spark-SQL predicate strings -> the C ABI predicate IR (dqscan.h, dq_pred_node), via the C++ compiler.

The parser and the Spark 2.2 literal typing live in libdqscan (deequ_amd/csrc/dq_pred_compile.cpp,
`dq_pred_pool_*`), so a JVM / JNI shim gets the same lowering from the same text; this module only
binds it and maps plan columns.  It stands in for Spark's `expr(...)` at the boundary
(analyzers/Analyzer.scala:385-408 and the predicate strings checks/Check.scala builds at :676, :687,
:705-760, :840, :867-868).  The accepted grammar (dqscan.h, dq_pred_pool_add):

    expr     := or
    or       := and ( OR and )*
    and      := not ( AND not )*
    not      := NOT not | cmp
    cmp      := operand ( (< | <= | > | >= | = | == | != | <>) operand | IS [NOT] NULL
                          | [NOT] IN ('string', ...) )?
    operand  := sum
    sum      := term ( (+ | -) term )*
    term     := unary ( (* | / | %) unary )*
    unary    := - unary | primary
    primary  := column | `column` | number | - number | NULL | TRUE | FALSE | 'string'
              | COALESCE(primary, primary) | ( expr )

Literal typing follows Spark 2.2: `3` integer, `3.0` exact decimal, `3e0` double.  String (in)equality
and IN lists on a string column lower to a whole-value DFA (DQ_PRED_REGEX, mode DQ_REGEX_FULL).
An operand with an arithmetic operator and a column (`a * b + c`, `id % 2`, `a / b`) is a DQ_PRED_EXPR node
over a postfix program (dqscan.h states the Spark 2.2 typing, wrapping, NULL and division rules):
expressions.py materialises it once per chunk as a derived column (dq_expr_eval) and _sync hands the node to
the plan as DQ_PRED_COLUMN of that column, so the plan's comparison rules apply to the result unchanged.
Anything else (string ordering, numeric comparison of a string column, LIKE, RLIKE, BETWEEN, functions,
literals with backslash escapes, arithmetic on decimal / non-numeric operands or on literals alone) raises
UnsupportedPredicate: such an analyzer is routed to the fallback set, exactly like a type the GPU plan does
not cover.
"""
from __future__ import annotations

import ctypes
from typing import List, Tuple

from . import _lib as L


class UnsupportedPredicate(ValueError):
    pass


_NO_COLUMN = "no such column: "


class PredicatePool:
    """The IR nodes and regex patterns of every predicate root of one plan.

    `builder` (analyzers.PlanBuilder) owns the table schema and the plan's column list: the C pool works
    on table column positions, and every node it appends is re-indexed to the plan column the builder
    registers for it (columns enter a plan on first reference)."""

    def __init__(self, builder):
        from .table import type_code

        self.b = builder
        names = [c[0] for c in builder.table_schema]
        self._names = names
        arr_n = (ctypes.c_char_p * max(1, len(names)))(*[n.encode("utf-8") for n in names])
        arr_t = (ctypes.c_int32 * max(1, len(names)))(*[type_code(c[1]) for c in builder.table_schema])
        h = ctypes.c_void_p()
        L.check(L.lib.dq_pred_pool_create(arr_n, arr_t, len(names), ctypes.byref(h)))
        self._h = h
        self.nodes: List[Tuple[int, int, int, int, int, float]] = []
        self.patterns: List[str] = []  # DQ_PRED_REGEX patterns (dq_plan_create_ex)
        self.exprs: list = []  # the C pool's expression list (expressions.Expression), DQ_PRED_EXPR nodes' `a`

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and L is not None and getattr(L, "lib", None) is not None:
            L.lib.dq_pred_pool_destroy(h)
            self._h = None

    def _sync(self) -> None:
        """Mirror the nodes / patterns the C pool appended, plan column indices in place of table ones."""
        from .expressions import expression_from_pool

        n = L.lib.dq_pred_pool_size(self._h)
        base = L.lib.dq_pred_pool_nodes(self._h)
        for k in range(len(self.exprs), L.lib.dq_pred_pool_num_exprs(self._h)):
            self.exprs.append(expression_from_pool(self._h, k, self._names))
        missing = None
        for i in range(len(self.nodes), n):
            x = base[i]
            kind, a, cmp = x.kind, x.a, x.cmp
            if kind == L.PRED_COLUMN:
                a = self.b.col(self._names[x.a])
            elif kind == L.PRED_EXPR:
                # an arithmetic operand: the plan reads its derived column (the builder refuses when the data
                # carries none; while only collecting the node stays as it is)
                try:
                    col = self.b.expr_col(self.exprs[x.a])
                except Exception as e:  # (the mirror stays whole; a plan refuses the node's kind)
                    col, missing = None, e
                if col is not None:
                    kind, a, cmp = L.PRED_COLUMN, col, 0
            self.nodes.append((kind, a, x.b, cmp, x.i64, x.f64))
        if missing is not None:
            raise missing
        npat = L.lib.dq_pred_pool_num_patterns(self._h)
        pats = L.lib.dq_pred_pool_patterns(self._h)
        self.patterns = [pats[i].decode("utf-8") for i in range(npat)]

    def _raise(self, status: int):
        msg = L.lib.dq_last_error().decode("utf-8", "replace")
        if status == L.DQ_E_UNSUPPORTED:
            raise UnsupportedPredicate(msg)
        if status == L.DQ_E_INVALID and msg.startswith(_NO_COLUMN):
            raise KeyError(msg[len(_NO_COLUMN):])
        L.check(status)

    def add(self, text: str) -> int:
        """Parse `text` (dq_pred_pool_add); returns the root node index."""
        root = ctypes.c_int32()
        s = L.lib.dq_pred_pool_add(self._h, text.encode("utf-8"), ctypes.byref(root))
        if s != L.DQ_OK:
            self._raise(s)
        self._sync()
        return root.value

    def add_regex(self, column: int, pattern: str, mode: int) -> int:
        """A DQ_PRED_REGEX node on plan column `column`; raises UnsupportedPredicate when the pattern is
        outside the GPU regex subset, so the analyzer is routed to the fallback."""
        root = ctypes.c_int32()
        table_col = self._names.index(self.b.columns[column])
        s = L.lib.dq_pred_pool_add_regex(self._h, table_col, pattern.encode("utf-8"), mode, ctypes.byref(root))
        if s != L.DQ_OK:
            self._raise(s)
        self._sync()
        return root.value

    def patterns_ctypes(self):
        arr = (ctypes.c_char_p * max(1, len(self.patterns)))(*[p.encode("utf-8") for p in self.patterns])
        return arr, len(self.patterns)

    def as_ctypes(self):
        arr = (L.PredNode * max(1, len(self.nodes)))()
        for i, (k, a, b, c, i64, f64) in enumerate(self.nodes):
            arr[i].kind, arr[i].a, arr[i].b, arr[i].cmp, arr[i].i64, arr[i].f64 = k, a, b, c, i64, f64
        return arr, len(self.nodes)
