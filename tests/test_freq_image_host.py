"""The frequency-table image parser (deequ_amd/csrc/dq_freq_image.cpp: host only, no HIP) under ASan + UBSan.

tests/freq_image_check.cpp, a stand-alone program, is compiled together with the parser by g++ with
-fsanitize=address,undefined and run: a valid hashed image (utf8, i32, decimal) and a valid unhashed one parse; every
truncation length from 0 to the full size, trailing bytes, a wrong magic / version / byte order, sizes that overflow
or exceed the image, n_groups >= 2^31, keys not strictly ascending, a count < 1, count sums off n_values (one that
wraps around to it included), string offsets that do not start at 0, decrease, or end off the byte length, and
unknown type codes all return DQ_E_STATE with a message -- and no sanitizer report (each image is parsed from a heap
block of exactly its length).  Nothing is loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT


def test_freq_image_parser_sanitized(tmp_path):
    csrc = os.path.join(ROOT, "deequ_amd", "csrc")
    exe = tmp_path / "freq_image_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tests", "freq_image_check.cpp"), os.path.join(csrc, "dq_freq_image.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
