"""The slot bookkeeping of the grouping scratch arena (deequ_amd/csrc/dq_arena.h: host only, no HIP) under ASan + UBSan.

tests/arena_check.cpp, a stand-alone program, maps the arena's memory hooks to malloc / free, counts their calls and
checks: buffers taken in one frame are pairwise disjoint, those of a nested helper included; growing a later slot
leaves every earlier pointer of the frame valid and its bytes intact; a second frame with equal or smaller requests
allocates nothing; a slot grows only when its capacity is below the request, to bytes + bytes / 8 with the 256-byte
floor; two devices' slot lists are independent.  Nothing is loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT


def test_arena_bookkeeping_sanitized(tmp_path):
    csrc = os.path.join(ROOT, "deequ_amd", "csrc")
    exe = tmp_path / "arena_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tests", "arena_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
