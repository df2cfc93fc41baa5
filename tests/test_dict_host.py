"""Dictionary-encoded string columns, host side (no GPU): dq_arrow_import_dictionary's buffer mapping and refusals,
the validate-and-widen loop (dq_dict_check_indices), and that dq_arrow_import still refuses dictionary arrays."""
import ctypes

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")


def _import_dictionary(arr):
    from deequ_amd import _lib as L, ingest

    s, a = ingest.ArrowSchemaC(), ingest.ArrowArrayC()
    arr._export_to_c(ctypes.addressof(a), ctypes.addressof(s))
    idx, dic = ingest.HostColumn(), ingest.HostColumn()
    # byref: right both for _lib's void* prototype and for the typed one ingest binds once a table was ingested
    # (after tests/test_dict_gpu.py in the same process a plain address is refused by ctypes)
    st = L.lib.dq_arrow_import_dictionary(ctypes.byref(s), ctypes.byref(a), ctypes.byref(idx), ctypes.byref(dic))
    return st, idx, dic, (s, a)


@pytest.mark.parametrize("ity,code,unsigned", [(pa.int8(), 8, 0), (pa.int16(), 7, 0), (pa.int32(), 3, 0),
                                              (pa.uint8(), 8, 1), (pa.uint16(), 7, 1)])
@pytest.mark.parametrize("vty,vcode", [(pa.string(), 4), (pa.large_string(), 5)])
def test_import_maps_indices_and_values(ity, code, unsigned, vty, vcode):
    from deequ_amd import _lib as L

    values = pa.array(["a", "bb", None, "dddd"], type=vty)
    arr = pa.DictionaryArray.from_arrays(pa.array([3, 0, None, 1, None, 2], type=ity), values)
    for sl, off in ((arr, 0), (arr.slice(3), 3)):
        st, idx, dic, keep = _import_dictionary(sl)
        assert st == L.DQ_OK, L.lib.dq_last_error()
        # the index column as dq_upload takes it: DICT_UTF8, the source width in `reserved` (negative: unsigned),
        # the entry count in offset_base, 4 bytes per row on the device
        assert (idx.type, idx.reserved, idx.n_rows) == (13, -code if unsigned else code, 6 - off)
        assert (idx.offset_base, idx.value_bytes) == (4, 4 * (6 - off))
        assert (dic.type, dic.n_rows, dic.nullable, dic.value_bytes) == (vcode, 4, 1, 7)
        w = {8: 1, 7: 2, 3: 4}[code]
        raw = ctypes.string_at(idx.values, idx.n_rows * w)
        got = np.frombuffer(raw, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32}[w])
        assert (got[-3], got[-1]) == (1, 2)
        assert idx.validity_bit == off % 8 and idx.nullable == 1


def test_import_sliced_dictionary():
    from deequ_amd import _lib as L

    values = pa.array(["zero", "one", "two", "three"]).slice(1)
    arr = pa.DictionaryArray.from_arrays(pa.array([0, 2, 1], type=pa.int32()), values)
    st, idx, dic, keep = _import_dictionary(arr)
    assert st == L.DQ_OK
    assert dic.n_rows == 3 and dic.offset_base == 4 and dic.value_bytes == len("onetwothree")


@pytest.mark.parametrize("arr", [
    lambda: pa.DictionaryArray.from_arrays(pa.array([0, 1], type=pa.int64()), pa.array(["a", "b"])),
    lambda: pa.DictionaryArray.from_arrays(pa.array([0, 1], type=pa.uint32()), pa.array(["a", "b"])),
    lambda: pa.DictionaryArray.from_arrays(pa.array([0, 1], type=pa.int32()), pa.array([1.5, 2.5])),
    lambda: pa.DictionaryArray.from_arrays(pa.array([0, 0], type=pa.int8()),
                                           pa.array(["a", "b"]).dictionary_encode()),
])
def test_import_refusals(arr):
    from deequ_amd import _lib as L

    st, _, _, keep = _import_dictionary(arr())
    assert st == L.DQ_E_UNSUPPORTED


def test_imported_array_still_refuses_dictionaries():
    from deequ_amd import ingest
    from deequ_amd._lib import DQError

    with pytest.raises(DQError):
        ingest.ImportedArray(pa.array(["a", "b"]).dictionary_encode())


def _check(code, a, n_entries, validity=None, bit=0):
    from deequ_amd import _lib as L

    out = np.full(len(a), -7, dtype=np.int32)
    vb = None if validity is None else np.packbits(np.concatenate([np.zeros(bit, bool), validity]), bitorder="little")
    st = L.lib.dq_dict_check_indices(code, a.ctypes.data, len(a), None if vb is None else vb.ctypes.data, bit, n_entries,
                                     out.ctypes.data)
    return st, out, L.lib.dq_last_error().decode()


def test_check_indices_widens_and_rejects():
    from deequ_amd import _lib as L

    for code, dt in ((8, np.int8), (7, np.int16), (3, np.int32), (-8, np.uint8), (-7, np.uint16)):
        a = np.array([0, 5, 127, 3], dtype=dt)
        st, out, _ = _check(code, a, 128)
        assert st == L.DQ_OK and list(out) == [0, 5, 127, 3]
        st, _, msg = _check(code, a, 127)
        assert st == L.DQ_E_INVALID and "row 2" in msg
    st, _, msg = _check(8, np.array([1, -1, 0], dtype=np.int8), 4)
    assert st == L.DQ_E_INVALID and "row 1" in msg and "-1" in msg
    assert _check(-8, np.array([200], dtype=np.uint8), 201)[0] == L.DQ_OK  # (unsigned: 200, not -56)
    # a NULL row's index is never looked at (slice bit offsets included)
    valid = np.array([True, False, True])
    st, out, _ = _check(3, np.array([1, 99, 2], dtype=np.int32), 3, valid, bit=5)
    assert st == L.DQ_OK and list(out) == [1, 0, 2]
    assert _check(2, np.array([1], dtype=np.int64), 3)[0] == L.DQ_E_UNSUPPORTED  # int64 indices


def test_dtype_and_type_code():
    from deequ_amd import _lib as L, table
    from deequ_amd.analyzers import spark_type

    assert table.DTYPES["dict_utf8"] == L.TYPE_DICT_UTF8 == 13
    assert not table.is_numeric("dict_utf8") and spark_type("dict_utf8") == "StringType"
    assert L.lib.dq_abi_version() == 6 and len(L.VARIANT_NAMES) == 32


def test_arrow_schema_and_host_columns_report_dict_utf8():
    from deequ_amd import ingest

    enc = pa.array(["a", "b", None, "a"]).dictionary_encode()
    batch = pa.record_batch([enc, enc.cast(pa.dictionary(pa.int8(), pa.large_string())), pa.array([1, 2, 3, 4])],
                            names=["c", "d", "x"])
    assert [(n, dt) for n, dt, _ in ingest.arrow_schema(batch)] == [("c", "dict_utf8"), ("d", "dict_utf8"), ("x", "i64")]
    hc = ingest.host_columns(batch)
    assert hc["c"].type == 13 and hc["c"].reserved == 3 and hc["c.dictionary"].type == 4
    assert hc["d"].type == 13 and hc["d"].reserved == 8 and hc["d.dictionary"].type == 5
    with pytest.raises(TypeError):  # int64 indices / numeric values are not dict_utf8
        ingest.arrow_schema(pa.record_batch([pa.array([1.5, 2.5]).dictionary_encode()], names=["f"]))


def test_from_pydict_encoder_first_occurrence_order():
    from deequ_amd import table

    idx, entries = table.encode_dictionary(["b", None, "a", "b", "", "a", None])
    assert entries == ["b", "a", ""] and idx == [0, None, 1, 0, 2, 1, None]
    assert table.encode_dictionary([]) == ([], []) and table.encode_dictionary([None]) == ([None], [])


def test_import_and_widen_under_host_sanitizers(tmp_path):
    """tests/dict_import_check.cpp: a stand-alone program over dq_ingest.cpp's import and validate-and-widen code with
    host ASan + UBSan (nothing is loaded into Python, no device is used)."""
    import os
    import subprocess

    from tests.conftest import ROOT

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "dict_import_check"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-fno-gpu-sanitize", "-fno-omit-frame-pointer", "-o", str(exe),
                    os.path.join(ROOT, "tests", "dict_import_check.cpp"), "-fsanitize=address,undefined"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
