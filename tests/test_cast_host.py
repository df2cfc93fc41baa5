"""Cast(StringType -> LongType | DoubleType) of Spark 2.2 as the kernels parse it (deequ_amd/csrc/dq_cast.h), built
for the host, against a plain-Python restatement of the two rules:

  * to_long_ref: org.apache.spark.unsafe.types.UTF8String.toLong -- raw bytes, [+-]digits[.digits], the fraction
    dropped, NULL outside [-2^63, 2^63 - 1] (Java's overflow checks on the negative accumulator amount to that);
  * to_double_ref: java.lang.Double.parseDouble with NumberFormatException -> NULL -- a regular expression of the
    Java grammar first (the JDK's own, Double.valueOf's documentation, with ASCII digits as FloatingDecimal reads
    them), then Python's float() on the validated decimal text and float.fromhex on a hex float: both correctly
    rounded (ties to even).  float() is never given unvalidated text: its own grammar is looser ("1_0", "inf").

Spark is not vendored in the reference: the rules are restated from Spark 2.2 / the JDK.  Values are compared by
their bits, and so is which rows the parse hands to the host's exact tier ("hard": more than 38 significant digits,
a net exponent outside [-38, 0] whose integer does not fit 38 digits, hex floats).  tests/test_cast_gpu.py runs the
same list on the device.
"""
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
NAN_BITS = 0x7FF8000000000000  # Double.NaN

_BLANKS = bytes(range(0x21))  # String.trim: chars <= U+0020
_DEC = rb"(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?"
_HEX = rb"0[xX](?:[0-9a-fA-F]+\.?|[0-9a-fA-F]*\.[0-9a-fA-F]+)[pP][+-]?[0-9]+"
_JAVA = re.compile(rb"([+-]?)(?:(NaN)|(Infinity)|(?:(" + _DEC + rb")|(" + _HEX + rb"))[fFdD]?)")
_LONG = re.compile(rb"([+-]?)([0-9]*)(?:\.[0-9]*)?")
_DEC_PARTS = re.compile(rb"([0-9]*)\.?([0-9]*)(?:[eE]([+-]?[0-9]+))?")


def to_long_ref(b: bytes):
    """UTF8String.toLong: the long, or None for NULL."""
    m = _LONG.fullmatch(b)
    if not b or b in (b"+", b"-") or not m:
        return None
    v = int(m.group(2) or b"0")
    if m.group(1) == b"-":
        v = -v
    return v if -(1 << 63) <= v < (1 << 63) else None


def _bits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def to_double_ref(b: bytes):
    """Double.parseDouble: the double's bits (any NaN = Double.NaN), or None for NULL."""
    m = _JAVA.fullmatch(b.strip(_BLANKS))
    if not m:
        return None
    sign, nan, inf, dec, hx = m.groups()
    if nan:
        return NAN_BITS
    if inf:
        v = float("inf")
    elif dec:
        v = float(dec.decode("ascii"))
    else:
        try:
            v = float.fromhex(hx.decode("ascii"))
        except OverflowError:
            v = float("inf")
    return _bits(-v if sign == b"-" else v)


def is_hard_ref(b: bytes) -> bool:
    """Whether a valid double text lies outside the device's fast tier (dq_cast.h)."""
    m = _JAVA.fullmatch(b.strip(_BLANKS))
    if not m or m.group(2) or m.group(3):
        return False
    if m.group(5):
        return True
    ip, fp, ex = _DEC_PARTS.fullmatch(m.group(4)).groups()
    sig = (ip + fp).lstrip(b"0")
    if not sig:
        return False
    if abs(int(ex or b"0")) >= 100000:  # the parse's exponent counter saturates there: never used in arithmetic
        return True
    e = int(ex or b"0") - len(fp)
    return len(sig) > 38 or not (-38 <= e <= 0 or (e > 0 and len(sig) + e <= 38))


def _ties(rng, count):
    """Exact rounding ties as tests/test_decimal_host.py builds them: the midpoint of two adjacent doubles in
    [2^22, 2^60) written as a decimal, and the decimals one unit in the last place either side."""
    out = []
    for _ in range(count):
        e = int(rng.integers(22, 60))
        y = float(rng.integers(1 << 52, 1 << 53)) * 2.0 ** (e - 52)
        succ = struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", y))[0] + 1))[0]
        m = (Fraction(y) + Fraction(succ)) / 2
        s = 0
        while (m * 10 ** s).denominator != 1:
            s += 1
        u = int(m * 10 ** s)
        if u + 1 >= 10 ** 38:
            continue
        for d in (0, -1, 1):
            digits = str(u + d)
            text = digits if s == 0 else digits[:-s] + "." + digits[-s:]
            out.append(text.encode())
            out.append(b"-" + text.encode())
    return out


def adversarial():
    """The list both test modules run (bytes values)."""
    rng = np.random.default_rng(2217)
    c = [b"", b"0", b"7", b"+7", b"-7", b"+", b"-", b"+-1", b"--1", b"-0", b"+0", b"-0.0", b"0.0", b"-.0", b"-0e5",
         b".", b"-.", b"+.", b"+.5", b"-.5", b".5", b"5.", b"1.9", b"-1.9", b"1.5", b"-1.5", b"1..5", b"1.5.", b"1.2.3",
         b" 1", b"1 ", b" 1 ", b"\t1.5\t", b" \t\n 42 \r\n", b"\x001\x00", b"1 2", b"- 1.5", b"+ .5", b"- 1", b" ", b"\t \t",
         b"1e", b"1e+", b"1e-", b"e5", b".e5", b"1e5", b"1E5", b"1e+5", b"1e-5", b"1.e5", b".5e1", b"1e5.0", b"1ee5",
         b"1f", b"1F", b"1d", b"1D", b" 1.5d ", b"1.5e3f", b"1dd", b"1fd", b"f", b"d", b"1.d", b".5D", b"1 d",
         b"NaN", b"+NaN", b"-NaN", b" NaN ", b"nan", b"NAN", b"NaNd", b"NaN1", b"Na",
         b"Infinity", b"+Infinity", b"-Infinity", b" -Infinity\t", b"inf", b"Inf", b"infinity", b"INFINITY", b"Infinityf",
         b"Infinit", b"Infinityy", b"1_0", b"1,0", b"0x", b"abc", b"true", b"1a", b"a1", b"$1", b"1%",
         "١٢".encode(), "１".encode(), "1 ".encode(), " 1".encode(), b"\xff", b"1\x80",
         b"0x1.8p1", b"0X1.8P1", b"-0x1.8p1", b"0x1.8", b"0x1p", b"0x1p+", b"0x.p1", b"0x.8p1", b"0x1.p1", b"0x1p1f",
         b"0x1p1d", b" 0x1p-1074 ", b"0x1p-1075", b"0x1.8p-1075", b"0x1p-1076", b"0x1.fffffffffffffp1023", b"0x1p1024",
         b"0x1.fffffffffffff8p1023", b"0x1.fffffffffffff7p1023", b"0x10000000000000.8p0", b"0x10000000000001.8p0",
         b"0xabcdef.ABCDEFp-3", b"0x1g.p1", b"0x1p1.5", b"00x1p1", b"0x0p0", b"-0x0.0p0", b"0x1p99999999999",
         b"0x1p-99999999999", b"0x1e5", b"0x1p1e",
         b"4.9e-324", b"2.4703282292062328e-324", b"2.4703282292062327e-324", b"2.4703282292062329e-324",
         b"2.2250738585072014e-308", b"2.2250738585072011e-308", b"1.7976931348623157e308", b"1.7976931348623158e308",
         b"1.7976931348623159e308", b"1e400", b"-1e400", b"1e-400", b"-1e-400", b"9007199254740993", b"9007199254740992.5",
         b"9007199254740992.4999999999999999999999", b"9007199254740992.50000000000000000000000000000000000000001",
         b"9007199254740994.5", b"0.1", b"0.3", b"123456789012345678", b"1e99999999999999999999", b"1e-99999999999999999999",
         b"0e99999999999999999999", b"0.0e-99999999999999999999"]
    for k in (1, 2, 5, 19, 20, 38, 39, 60):  # leading zeros
        z = b"0" * k
        c += [z, z + b"1", b"-" + z + b"12", z + b".5", z + b"9223372036854775807", z + b"9223372036854775808",
              b"-" + z + b"9223372036854775808", b"0." + z + b"1", b"." + z + b"25"]
    for v in (10 ** 17, 10 ** 18 - 1, 10 ** 18, 2 ** 63 - 2, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 10 ** 19 - 1, 10 ** 19,
              2 ** 64 - 1, 2 ** 64, 10 ** 20 - 1, 99999999999999999999, 18446744073709551616 + 7):
        for s in ("", "+", "-"):
            c += [f"{s}{v}".encode(), f"{s}{v}.9".encode()]
    for nf in (0, 1, 17, 38, 39, 400):  # fraction digits
        f = "".join(str(int(d)) for d in rng.integers(0, 10, nf))
        c += [f"3.{f}".encode(), f"-0.{f}".encode(), f"12345.{f}e3".encode(), f".{f}1".encode(),
              ("0." + "0" * nf + "7").encode(), ("1." + "0" * nf).encode()]
    c += [b"1." + b"2" * 37, b"1." + b"2" * 38, b"9" * 38, b"9" * 39, b"9" * 38 + b".5", b"0." + b"9" * 38,
          b"0.0" + b"9" * 38, b"1" + b"0" * 37, b"1" + b"0" * 38, b"1e37", b"1e38", b"12e36", b"12e37", b"1.5e38"]
    for e in (22, 38, 39, 308, 324, 400):  # exponents
        for m in ("1", "1.5", "9.999999999999999", "4.9", "2.5", "17976931348623157"):
            c += [f"{m}e{e}".encode(), f"{m}e-{e}".encode(), f"-{m}E+{e}".encode(), f"{m}e{e}d".encode()]
    # long runs of fraction zeros with a compensating exponent (the value is a small number again), either side of
    # 1000 fraction digits and of the exponent magnitude 100000 at which the parse stops counting
    for k in (998, 999, 1000, 1001, 1002, 4095, 99998, 99999, 100000, 100001):
        z = "0." + "0" * k
        c += [f"{z}1e{k + 1}".encode(), f"{z}1e{k + 2}".encode(), f"-{z}25e{k + 6}".encode(), f"{z}1e{k - 20}".encode(),
              f"{z}1".encode(), (z + "9007199254740993e" + str(k + 16)).encode()]
    for e in (99998, 99999, 100000, 100001, 999999, 1000000):
        c += [f"1e{e}".encode(), f"1e-{e}".encode(), f"0e{e}".encode(), f"-0.0e-{e}".encode(),
              ("1" + "0" * 50 + f"e-{e}").encode(), f"1e0000000000{e}".encode()]
    c += [("1" + "0" * 99990 + "e-99980").encode(), ("12" + "0" * 100010 + "e-100000").encode(), b"1e0000000000000000000005"]
    c += _ties(rng, 60)
    return c


def random_numeric(rng, count):
    """Short numeric strings as a profiled column holds them: integers and plain fractions."""
    out = []
    for _ in range(count):
        v = str(int(rng.integers(0, 10 ** int(rng.integers(1, 13)))))
        if rng.random() < 0.4:
            v += "." + str(int(rng.integers(0, 10 ** int(rng.integers(1, 7)))))
        out.append((("-" if rng.random() < 0.3 else "") + v).encode())
    return out


def _build(tmp_path, fused=False):
    """g++ -O2; fused: clang with FMA contraction on (the device default), which the conversion must switch off."""
    exe = tmp_path / ("cast_check_fma" if fused else "cast_check")
    cc = [CLANG, "-mfma", "-ffp-contract=fast"] if fused else ["g++"]
    subprocess.run(cc + ["-O2", "-std=c++17", "-I", os.path.join(ROOT, "deequ_amd", "csrc"), "-o", str(exe),
                         os.path.join(ROOT, "tests", "cast_check.cpp")], check=True)
    return exe


def test_reference_anchors():
    """The Python reference itself, against values written by hand."""
    assert to_long_ref(b".") == 0 and to_long_ref(b"-.") == 0 and to_long_ref(b"+.5") == 0
    assert to_long_ref(b"1.9") == 1 and to_long_ref(b"-1.9") == -1
    assert to_long_ref(b"9223372036854775808") is None
    assert to_long_ref(b"-9223372036854775808") == -(1 << 63)
    assert to_long_ref(b"9223372036854775807") == (1 << 63) - 1
    assert to_long_ref(b"0" * 60 + b"12") == 12
    for bad in (b"", b"+", b"-", b" 1", b"1e5", b"1.2.3", b"1 "):
        assert to_long_ref(bad) is None, bad
    assert to_double_ref(b" 1.5d ") == _bits(1.5)
    assert to_double_ref(b"1e400") == _bits(float("inf")) == 0x7FF0000000000000
    assert to_double_ref(b"-1e400") == 0xFFF0000000000000
    assert to_double_ref(b"4.9e-324") == 1  # Double.MIN_VALUE
    # half of the minimum subnormal: 2^-1075 = 2.4703282292062327208...e-324; above it rounds up, below (and the tie
    # itself, to even) down to 0
    assert to_double_ref(b"2.4703282292062328e-324") == 1
    assert to_double_ref(b"2.4703282292062327e-324") == 0
    assert to_double_ref(b"0x1p-1075") == 0 and to_double_ref(b"0x1.8p-1075") == 1
    assert to_double_ref(b"9007199254740993") == _bits(9007199254740992.0)
    assert to_double_ref(b"9007199254740992.5") == _bits(9007199254740992.0)
    assert to_double_ref(b"9007199254740994.5") == _bits(9007199254740994.0)
    assert to_double_ref(b"0x1.8p1") == _bits(3.0)
    assert to_double_ref(b"0x1.8") is None
    assert to_double_ref(b"-0") == 1 << 63 and to_double_ref(b"-NaN") == NAN_BITS
    for bad in (b"inf", b"nan", b"1_0", b"1e", b"e5", b"+", b"1 2", "١".encode(), b"", b"  ", b".", b"NaNd"):
        assert to_double_ref(bad) is None, bad
    assert is_hard_ref(b"0x1p1") and is_hard_ref(b"1e39") and is_hard_ref(b"1e-39") and is_hard_ref(b"9" * 39)
    assert is_hard_ref(b"1e38") and not is_hard_ref(b"1e37") and not is_hard_ref(b"0e999") and not is_hard_ref(b"0." + b"9" * 38)
    assert is_hard_ref(b"12e37") and not is_hard_ref(b"12e36")
    # fraction digits are counted exactly: 1001 zeros, then 1, times 10^1002 is 1
    assert to_double_ref(b"0." + b"0" * 1001 + b"1e1002") == _bits(1.0) and not is_hard_ref(b"0." + b"0" * 1001 + b"1e1002")
    assert to_double_ref(b"0." + b"0" * 1001 + b"1e1005") == _bits(1000.0)
    assert to_double_ref(b"0." + b"0" * 99999 + b"1e100000") == _bits(1.0) and is_hard_ref(b"0." + b"0" * 99999 + b"1e100000")
    assert not is_hard_ref(b"0." + b"0" * 99998 + b"1e99999") and is_hard_ref(b"1e-100000")


@pytest.mark.parametrize("fused", [False, True])
def test_cast_formulation(tmp_path, fused):
    if fused and not os.path.exists(CLANG):
        pytest.skip("no clang++ for the contraction check")
    exe = _build(tmp_path, fused)
    cases = adversarial() + random_numeric(np.random.default_rng(5), 500)
    inp = "".join(f"{k} {b.hex() or '-'}\n" for b in cases for k in "LD")
    out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 2 * len(cases)
    n_hard = n_tie = 0
    for i, b in enumerate(cases):
        got_l, got_d = out[2 * i].split(), out[2 * i + 1].split()
        want_l = to_long_ref(b)
        assert got_l == (["N"] if want_l is None else ["V", f"{want_l & ((1 << 64) - 1):016x}"]), (b, got_l, want_l)
        want_d = to_double_ref(b)
        if want_d is None:
            assert got_d == ["N"], (b, got_d)
        elif is_hard_ref(b):
            n_hard += 1
            assert got_d[0] == "H", (b, got_d)
            # the text the host tier hands to strtod: the value without blanks and suffix
            m = _JAVA.fullmatch(b.strip(_BLANKS))
            assert b[int(got_d[1]):int(got_d[2])] == m.group(1) + (m.group(4) or m.group(5)), (b, got_d)
        else:
            assert got_d == ["V", f"{want_d:016x}"], (b, got_d, f"{want_d:016x}")
            n_tie += b.endswith(b"5") and b"." in b and len(b) > 15
    assert n_hard > 60 and n_tie > 50
