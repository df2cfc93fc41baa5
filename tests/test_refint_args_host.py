"""The argument validation of dq_freq_contains_rows under ASan + UBSan, on the host.

tests/contains_args_check.cpp, a stand-alone program with its own main, calls the entry with every combination of
invalid arguments that returns before the device is touched -- n_rows out of range (2^31 with a 1-row buffer among
them), misaligned bitmaps, NULL contained / cols / table -- and checks status, message and that nothing was written.
The entry's host code (deequ_amd/csrc/dq_probe.hip and what it links: dq_group.hip for the scratch arena, dq_prim.hip)
is compiled into the program with the host sanitizers; the kernels' device code is compiled as usual and never runs.  Nothing is loaded
into Python."""
import os
import subprocess

from tests.conftest import ROOT


def test_contains_rows_argument_validation_sanitized(tmp_path):
    csrc = os.path.join(ROOT, "deequ_amd", "csrc")
    exe = tmp_path / "contains_args_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-result",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tests", "contains_args_check.cpp"), os.path.join(csrc, "dq_probe.hip"),
                    os.path.join(csrc, "dq_group.hip"), os.path.join(csrc, "dq_prim.hip")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
