"""Entropy and MutualInformation of the GPU against their true values.  The other grouping tests compare both with a
float64 evaluation of the same formula at a relative 1e-12, which hides an error that is small against the sum of
the terms' magnitudes (MutualInformation's terms have mixed signs) and cannot be asked of ill-conditioned inputs
(one dominant group; independent columns, whose true value is 0).  Here every value is compared with a 50-digit
mpmath evaluation from the exact counts, within twice the derived rounding bound of the kernels' double arithmetic
(tests/group_ref.py: ref_entropy, ref_mi; tests/test_group_ref_host.py holds a float64 evaluation on the host to the
bound itself).  The factor 2 covers second-order terms and partial sums above the sum of the terms' magnitudes; it is
a margin over a derived bound, not a fitted number.

Values come through the public analyzers (dq.Entropy, dq.MutualInformation: the one-pass path), MutualInformation
also through the state path (FreqTable.mutual_information of the materialised joint table); the two must agree within
the same bound.  Each test prints |gpu - value| / bound ("Grouping metrics: error against the exact value").
"""
from __future__ import annotations

import math

import mpmath
import numpy as np
import pytest

from tests import group_cases as C
from tests import group_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 2.0

_ENTROPY = C.entropy_cases()
_MI = C.mi_cases()


@pytest.fixture(scope="module")
def dq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import deequ_amd

    return deequ_amd


def _within(got: float, value, bound: float, what) -> float:
    ratio = R.error_ratio(got, value, bound)
    print(f"{what}: gpu {got!r} exact {mpmath.nstr(value, 20)} bound {bound:.3e} |error| / bound {ratio:.3f}")
    assert ratio <= MARGIN, (what, got, mpmath.nstr(value, 25), bound, ratio)
    return ratio


@pytest.mark.parametrize("name", list(_ENTROPY))
def test_entropy_against_the_exact_value(dq, monkeypatch, name):
    monkeypatch.delenv("DQ_GROUP_DICT", raising=False)
    chunk = _ENTROPY[name]
    n = C.rows([chunk])
    ref = R.ref_table(*C.key_columns([chunk], ["x"]))
    value, bound = R.ref_entropy(ref.counts, n)
    got = dq.Entropy("x").calculate(C.to_device(chunk)).value.get()
    _within(got, value, bound, f"Entropy {name}")
    if name == "one-group":
        assert ref.num_groups == 1 and got == 0.0  # 0.0 or -0.0: p = 1 exactly, ln 1 = 0
    if name.startswith("uniform-"):
        G = int(name.split("-")[1])
        assert ref.num_groups == G and len(set(ref.counts.tolist())) == 1 and R.agrees(value, R.ln(G))
    if name == "dominant-group":
        assert n == 70_001 and sorted(ref.counts.tolist()) == [1, n - 1]
    if name == "nulls-30-percent":
        assert 0.25 * n < n - ref.num_values < 0.35 * n  # num_rows counts the null rows, the groups do not
    if name == "singletons-300000":
        assert ref.num_groups == ref.num_unique == 300_000 and R.launched_blocks(ref.num_groups) == 1024


@pytest.mark.parametrize("name", list(_MI))
def test_mutual_information_against_the_exact_value(dq, name):
    from deequ_amd.grouping import build_frequencies

    chunk = _MI[name]
    n = C.rows([chunk])
    ref = R.ref_table(*C.key_columns([chunk], ["x", "y"]))
    value, bound = R.ref_mi(ref.joint, n)
    data = C.to_device(chunk)
    one_pass = dq.MutualInformation("x", "y").calculate(data).value.get()
    state = build_frequencies(data, ["x", "y"]).materialize()
    from_state = state.frequencies.mutual_information(state.numRows)
    _within(one_pass, value, bound, f"MutualInformation {name} (one pass)")
    _within(from_state, value, bound, f"MutualInformation {name} (state)")
    assert abs(one_pass - from_state) <= MARGIN * bound, (name, one_pass, from_state, bound)
    assert np.array_equal(np.sort(state.frequencies.export()[1]), ref.counts)
    if name.startswith("product-"):  # independent columns: the truth is 0
        assert R.agrees(value, 0) and abs(one_pass) <= MARGIN * bound and abs(from_state) <= MARGIN * bound
    if name == "y-equals-x":  # the entropy of x over the rows where it is non-null, num_rows counting all rows
        x = R.ref_table(*C.key_columns([chunk], ["x"]))
        assert x.num_values < n and R.agrees(value, R.ref_entropy(x.counts, n)[0])
    if name == "f64-x-i64":  # NaN (two payloads: one group), -0.0 and 0.0 (two groups) among x's 6 values
        assert len(ref.marginals[0]) == 6
    if name == "single-pair-row":
        assert n == 1 and one_pass == 0.0 and from_state == 0.0
    assert math.isfinite(one_pass) and math.isfinite(from_state)
