"""Row-level results, planning only (deequ_amd/rowlevel.py plan_row_level): no device.  Which constraints get a
row-level form and under which key, the (predicate, where) roots of each, the skipped constraints with their reasons,
and the split of more outputs than one row program holds into several programs."""
import pytest


@pytest.fixture(scope="module")
def rl():
    import deequ_amd  # noqa: F401
    from deequ_amd import rowlevel

    return rowlevel


SCHEMA = [("id", "i64", True), ("x", "f64", True), ("y", "f64", True), ("s", "utf8", True), ("d", "dict_utf8", True)]


def checks():
    from deequ_amd.checks import Check, CheckLevel

    c1 = (Check(CheckLevel.Error, "first")
          .isComplete("id")
          .isUnique("id")
          .satisfies("x >= 0", "x positive").where("id > 3")
          .isContainedIn("s", ["a", "b"])
          .hasPattern("s", r"[a-c]+")
          .hasSize(lambda n: n > 0))
    c2 = (Check(CheckLevel.Warning, "second")
          .satisfies("s LIKE 'a%'", "like")
          .hasMinLength("s", lambda v: v >= 1)
          .containsEmail("d")
          .isPrimaryKey("id", "s")
          .hasCompleteness("x", lambda v: v > 0.5).where("y > 0")
          .isLessThan("x", "y")
          .hasMean("x", lambda v: v > 0))
    return [c1, c2]


def test_forms_keys_and_roots(rl):
    from deequ_amd.analyzers import Patterns

    plan = rl.plan_row_level(checks(), SCHEMA)
    forms = plan.forms
    assert list(forms) == [
        "CompletenessConstraint(Completeness(id,None))",
        "UniquenessConstraint(Uniqueness(List(id)))",
        "ComplianceConstraint(Compliance(x positive,x >= 0,Some(id > 3)))",
        "ComplianceConstraint(Compliance(s contained in a,b,`s` IS NULL OR `s` IN ('a','b'),None))",
        "PatternMatchConstraint(s, [a-c]+)",
        "containsEmail(d)",
        "UniquenessConstraint(Uniqueness(List(id, s)))",
        "CompletenessConstraint(Completeness(x,Some(y > 0)))",
        "ComplianceConstraint(Compliance(x is less than y,x < y,None))",
    ]
    f = forms["CompletenessConstraint(Completeness(id,None))"]
    assert (f.kind, f.pred, f.where) == ("predicate", ("sql", "`id` IS NOT NULL"), None)
    f = forms["ComplianceConstraint(Compliance(x positive,x >= 0,Some(id > 3)))"]
    assert (f.kind, f.pred, f.where) == ("predicate", ("sql", "x >= 0"), "id > 3")
    f = forms["PatternMatchConstraint(s, [a-c]+)"]
    assert (f.kind, f.pred, f.where) == ("predicate", ("regex", "s", "[a-c]+"), None)
    f = forms["containsEmail(d)"]
    assert (f.kind, f.pred, f.where) == ("predicate", ("regex", "d", Patterns.EMAIL), None)
    f = forms["CompletenessConstraint(Completeness(x,Some(y > 0)))"]
    assert (f.kind, f.pred, f.where) == ("predicate", ("sql", "`x` IS NOT NULL"), "y > 0")
    f = forms["UniquenessConstraint(Uniqueness(List(id)))"]
    assert (f.kind, f.columns) == ("unique", ("id",))
    assert forms["UniquenessConstraint(Uniqueness(List(id, s)))"].columns == ("id", "s")
    # the checks' keys: their row-level constraints in order, the skipped ones left out
    assert [(d, len(k)) for d, k in plan.checks] == [("first", 5), ("second", 4)]
    assert plan.checks[1][1][0] == "containsEmail(d)"

    # one program holds the seven predicate forms; its outputs' roots are pool nodes, -1 without a where
    assert len(plan.programs) == 1
    prog = plan.programs[0]
    assert [f.key for f in prog.forms] == [k for k, f in forms.items() if f.kind == "predicate"]
    assert len(prog.roots) == 7
    assert [w >= 0 for _, w in prog.roots] == [False, True, False, False, False, True, False]
    assert all(p >= 0 for p, _ in prog.roots)
    assert len({p for p, _ in prog.roots}) == 7
    n_out, n_roots, n_instr = prog.info()
    assert (n_out, n_roots) == (7, 9) and n_instr >= n_roots * 2
    assert plan.program_of("containsEmail(d)") == (0, 4)
    # the dictionary column is planned as the plain string column it stands for
    assert prog.columns == ["id", "x", "s", "d", "y"]
    assert dict((n, t) for n, t, _ in plan.schema)["d"] == "utf8"


def test_skipped_with_reasons(rl):
    plan = rl.plan_row_level(checks(), SCHEMA)
    skipped = dict(plan.skipped)
    assert list(skipped) == ["SizeConstraint(Size(None))", "ComplianceConstraint(Compliance(like,s LIKE 'a%',None))",
                             "MinLengthConstraint(MinLength(s,None))", "MeanConstraint(Mean(x,None))"]
    assert skipped["SizeConstraint(Size(None))"] == "Size has no row-level form"
    assert skipped["MinLengthConstraint(MinLength(s,None))"] == "MinLength has no row-level form"
    assert skipped["MeanConstraint(Mean(x,None))"] == "Mean has no row-level form"
    like = skipped["ComplianceConstraint(Compliance(like,s LIKE 'a%',None))"]
    assert like.startswith("UnsupportedPredicate") and "LIKE" in like
    # never both: a skipped constraint is in no check's keys and has no form
    for key in skipped:
        assert key not in plan.forms and all(key not in keys for _, keys in plan.checks)


def test_other_constraints_are_skipped(rl):
    from deequ_amd.checks import Check, CheckLevel, ConstrainableDataTypes

    c = (Check(CheckLevel.Error, "rest")
         .hasMin("x", lambda v: v > 0).hasMax("x", lambda v: v > 0).hasMaxLength("s", lambda v: v < 9)
         .hasApproxQuantile("x", 0.5, lambda v: v > 0).hasEntropy("s", lambda v: v > 0)
         .hasDistinctness(["s"], lambda v: v > 0).hasUniqueValueRatio(["s"], lambda v: v > 0)
         .hasDataType("s", ConstrainableDataTypes.String).hasNumberOfDistinctValues("s", lambda v: v > 0)
         .hasMutualInformation("x", "y", lambda v: v > 0).hasStandardDeviation("x", lambda v: v > 0)
         .containsCreditCardNumber("s").isComplete("nope").hasUniqueness(["nope"], lambda v: v == 1))
    plan = rl.plan_row_level([c], SCHEMA)
    assert plan.forms == {} and plan.programs == [] and plan.checks == [("rest", [])]
    reasons = [r for _, r in plan.skipped]
    assert len(reasons) == 14
    assert sum(r.endswith("has no row-level form") for r in reasons) == 11
    assert reasons[11].startswith("UnsupportedPredicate")  # the credit card pattern: outside the regex subset
    assert reasons[12].startswith("NoSuchColumnException") and reasons[13].startswith("NoSuchColumnException")


def test_split_over_program_capacity(rl):
    from deequ_amd.checks import Check, CheckLevel

    cap = rl.max_outputs()
    assert cap == 32  # kMaxRoots (deequ_amd/csrc/dq_device.h)
    many = Check(CheckLevel.Error, "many")
    for i in range(cap + 1):
        many = many.satisfies(f"x >= {i}", f"p{i}")
    plan = rl.plan_row_level([many], SCHEMA)
    assert [p.info()[:2] for p in plan.programs] == [(cap, cap), (1, 1)]
    assert plan.program_of(f"ComplianceConstraint(Compliance(p{cap},x >= {cap},None))") == (1, 0)
    assert plan.skipped == []
    # a `where` is a root too: 20 outputs with 20 predicates and 20 filters need 40 roots
    w = Check(CheckLevel.Error, "w")
    for i in range(20):
        w = w.satisfies(f"x >= {i}", f"p{i}").where(f"y < {i}")
    plan = rl.plan_row_level([w], SCHEMA)
    assert [p.info()[:2] for p in plan.programs] == [(16, 32), (4, 8)]
    # shared roots are stored once
    s = Check(CheckLevel.Error, "s")
    for i in range(20):
        s = s.satisfies(f"x >= {i}", f"p{i}").where("y < 1")
    plan = rl.plan_row_level([s], SCHEMA)
    assert [p.info()[:2] for p in plan.programs] == [(20, 21)]
    # a smaller cap (tests of the split at small sizes)
    plan = rl.plan_row_level([s], SCHEMA, max_outputs_per_program=8)
    assert [p.info()[0] for p in plan.programs] == [7, 7, 6]


def test_library_rejects_bad_programs(rl):
    import ctypes

    from deequ_amd import _lib as L

    h = ctypes.c_void_p()
    outs = (L.RowOutput * 1)()
    outs[0].pred_root, outs[0].where_root = 0, -1
    sch = (L.ColumnDesc * 1)()
    sch[0].type, sch[0].nullable = L.TYPE_F64, 1
    pool = (L.PredNode * 1)()
    # root out of range, no outputs, too many outputs: rejected on the host
    assert L.lib.dq_row_program_create(sch, 1, pool, 0, None, 0, outs, 1, ctypes.byref(h)) == L.DQ_E_INVALID
    assert L.lib.dq_row_program_create(sch, 1, pool, 0, None, 0, outs, 0, ctypes.byref(h)) == L.DQ_E_INVALID
    big = (L.RowOutput * 33)()
    assert L.lib.dq_row_program_create(sch, 1, pool, 0, None, 0, big, 33, ctypes.byref(h)) == L.DQ_E_UNSUPPORTED
    assert not h.value
    assert L.lib.dq_row_outcomes(None, None, 0, None, None, 0, None, None, None) == L.DQ_E_INVALID
    assert L.lib.dq_freq_unique_rows(None, None, None, 0, None, None, None, None, None) == L.DQ_E_INVALID
