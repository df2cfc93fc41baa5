"""The predicate lowering and the one program builder (deequ_amd/csrc/dq_pred_lower.cpp) without a GPU and without
Python in the way: tests/lower_check.cpp is a stand-alone program over the lowering, built with host ASan + UBSan and
run directly.  Its dump of every program -- each case built in the planner's order of roots and in the row program's --
must equal tests/lower_check_expected.txt, which the code before the split produced (the planner's and the row
program's own assembly loops, driven over the same corpus), so the builder emits what both copies emitted.
"""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

EXPECTED = os.path.join(ROOT, "tests", "lower_check_expected.txt")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path_factory.mktemp("lower_check") / "lower_check"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fno-gpu-sanitize", "-fno-omit-frame-pointer", "-o", str(exe),
                    os.path.join(ROOT, "tests", "lower_check.cpp"), "-fsanitize=address,undefined"], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def cases(dump):
    """{case header: (plan section, row section)} of a dump."""
    out = {}
    for block in re.split(r"^(?=== case )", dump, flags=re.M):
        if block.startswith("== case "):
            head, rest = block.split("\n-- plan\n", 1)
            plan, row = rest.split("\n-- row\n", 1)
            out[head] = (plan, row.split("\nok ")[0].rstrip("\n"))
    return out


def test_clean_under_host_sanitizers(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert re.fullmatch(r"ok \d+ cases", run.stdout.strip().splitlines()[-1]), run.stdout[-500:]
    assert "FAILED" not in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]


def test_dump_equals_the_programs_before_the_split(run):
    with open(EXPECTED) as f:
        want = f.read()
    got, exp = cases(run.stdout), cases(want)
    assert list(got) == list(exp)
    for head in exp:
        assert got[head] == exp[head], head
    assert run.stdout == want


def test_both_orders_emit_one_stream(run):
    """Where the planner and the row program meet the roots in the same order, their programs are the same; every limit
    is reported by both; and the corpus reaches each limit from both sides."""
    got = cases(run.stdout)
    same = [h for h in got if "same order" in h]
    assert len(same) >= 60 and len(got) - len(same) >= 1
    for head in same:
        plan, row = got[head]
        assert plan == row, head
    text = run.stdout
    for limit in ("roots", "instructions", "stack", "regex"):
        assert text.count(f"status=-3 limit={limit}\n") == 2, limit
    # the last sizes that fit, right below the four limits
    assert text.count(" n_instr=96 ") == 2 and text.count(" stack_depth=16 ") == 2
    assert re.search(r"three long patterns\n-- plan\nstatus=0 .* regex_words=2\d{4} ", text)
    assert re.search(r"one root too many\n-- plan\nstatus=-3 limit=roots", text)
