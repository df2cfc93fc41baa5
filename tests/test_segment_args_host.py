"""The argument validation of dq_segment_order and dq_segment_scan without a device: tests/segment_args_check.cpp, a
stand-alone program with its own main, built with the host sanitizers and run."""
import os
import subprocess

from tests.conftest import ROOT


def test_segment_argument_validation_sanitized(tmp_path):
    """NULL pointers, negative sizes, n_slots out of range, an unknown op or type, G + 1 beyond int32: each returns
    before the device is touched.  The entries' host code is compiled into the program with ASan + UBSan; the
    kernels' device code is compiled as usual and never runs."""
    csrc = os.path.join(ROOT, "deequ_amd", "csrc")
    exe = tmp_path / "segment_args_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-result",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tests", "segment_args_check.cpp"), os.path.join(csrc, "dq_segment.hip"),
                    os.path.join(csrc, "dq_prim.hip")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
