"""Arrow data as Tables, host side (no GPU): the type mapping and refusals of the conversion, and the host half of
dq_upload_to (dq_upload_stage: bitmap realignment, offset rebasing, index widening and range check, the decimal range
check) through ctypes on host buffers against a numpy restatement written here; tests/upload_to_check.cpp runs the same
function under host ASan + UBSan as a stand-alone program."""
import ctypes
import decimal
import os
import subprocess

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

BITS = (0, 1, 7, 8, 13)
ROWS = (0, 1, 7, 8, 9, 63, 64, 65, 1000)


def _stage(arrays, nullable):
    """dq_upload_stage of pyarrow arrays into a host buffer -> per array (values, validity, offsets) byte images (None:
    no such buffer), sized as the conversion sizes them; or (status, message) on a refusal."""
    from deequ_amd import _lib as L, ingest

    lib = ingest._bind()
    ims = [ingest.ImportedDictionaryArray(a) if pa.types.is_dictionary(a.type) else ingest.ImportedArray(a)
           for a in arrays]
    try:
        k = len(ims)
        hosts = (ingest.HostColumn * k)(*[i.host for i in ims])
        payload = (ctypes.c_int64 * k)()
        st = lib.dq_upload_payload(hosts, k, payload)
        if st != L.DQ_OK:
            return st, L.lib.dq_last_error().decode()
        dests = (ingest.UploadDest * k)()
        for c, (a, nl) in enumerate(zip(arrays, nullable)):
            n, t = len(a), a.type
            string = t in (pa.string(), pa.large_string())
            dests[c].values = 1
            dests[c].value_bytes = ingest._padded(ingest._bitmap_bytes(n) if t == pa.bool_() else
                                                  4 * n if pa.types.is_dictionary(t) else payload[c])
            if nl:
                dests[c].validity, dests[c].validity_bytes = 1, ingest._bitmap_bytes(n)
            if string:
                dests[c].offsets, dests[c].offset_bytes = 1, ingest._padded((n + 1) * (8 if t == pa.large_string() else 4))
        size = sum((d.value_bytes + d.validity_bytes + d.offset_bytes) + 3 * 256 for d in dests)
        stage = np.full(size, 0xA5, dtype=np.uint8)  # (every byte of an image must be written)
        pos = (ctypes.c_int64 * (3 * k))()
        used = ctypes.c_int64()
        st = lib.dq_upload_stage(hosts, k, dests, stage.ctypes.data, size, 2, pos, ctypes.byref(used))
        if st != L.DQ_OK:
            return st, L.lib.dq_last_error().decode()
        out = []
        for c in range(k):
            lens = (dests[c].value_bytes, dests[c].validity_bytes, dests[c].offset_bytes)
            out.append(tuple(None if pos[3 * c + j] < 0 else stage[pos[3 * c + j]:pos[3 * c + j] + lens[j]].copy()
                             for j in range(3)))
        return out
    finally:
        for i in ims:
            i.close()


def _pad(a, mult, extra):
    from deequ_amd.table import _pad_u8

    return _pad_u8(np.frombuffer(bytes(a), dtype=np.uint8), mult, extra)


def _bitmap(valid):
    from deequ_amd.table import pack_validity

    return pack_validity(np.asarray(valid, dtype=bool))


# ------------------------------------------------------------------------------------------ types
def test_every_accepted_type_maps_to_the_from_pydict_dtype():
    from deequ_amd import ingest, table

    types = [(pa.float64(), "f64"), (pa.float32(), "f32"), (pa.int64(), "i64"), (pa.int32(), "i32"),
             (pa.int16(), "i16"), (pa.int8(), "i8"), (pa.bool_(), "bool"), (pa.date32(), "date32"),
             (pa.timestamp("us"), "timestamp"), (pa.timestamp("us", tz="UTC"), "timestamp"), (pa.string(), "utf8"),
             (pa.large_string(), "large_utf8"), (pa.decimal128(38, 4), "decimal(38,4)"),
             (pa.decimal128(1, 0), "decimal(1,0)")]
    for it in (pa.int8(), pa.int16(), pa.int32(), pa.uint8(), pa.uint16()):
        for vt in (pa.string(), pa.large_string()):
            types.append((pa.dictionary(it, vt), "dict_utf8"))
    schema = pa.schema([pa.field(f"c{k}", t, nullable=k % 2 == 0) for k, (t, _) in enumerate(types)])
    got = ingest.arrow_schema(schema.empty_table())
    assert got == [(f"c{k}", dt, k % 2 == 0) for k, (_, dt) in enumerate(types)]
    for _, dt, _ in got:  # a dtype from_pydict knows
        assert table.type_code(dt) > 0


@pytest.mark.parametrize("bad", [pa.uint32(), pa.timestamp("ns"), pa.date64(), pa.list_(pa.int32()),
                                 pa.dictionary(pa.int64(), pa.string())])
def test_refused_types_name_the_column(bad):
    from deequ_amd import ingest

    batch = pa.schema([pa.field("ok", pa.int32()), pa.field("the_bad_one", bad)]).empty_table()
    with pytest.raises(TypeError, match="the_bad_one"):
        ingest.arrow_schema(batch)
    # the conversion refuses it the same way, before a device is touched (this test runs without one)
    for shape in (batch, batch.to_batches() or [pa.RecordBatch.from_pylist([], schema=batch.schema)]):
        with pytest.raises(TypeError, match="the_bad_one"):
            ingest.tables_from_arrow(shape)
    assert ingest.is_arrow(batch) and not ingest.is_arrow([]) and not ingest.is_arrow({"a": 1})


# ------------------------------------------------------------------------------------------ the host half
@pytest.mark.parametrize("bit", BITS)
def test_bitmap_realignment(bit):
    rng = np.random.default_rng(bit)
    for n in ROWS:
        valid = rng.random(bit + n) < 0.7
        vals = rng.random(bit + n) < 0.5
        ints = rng.integers(-1000, 1000, bit + n).astype(np.int16)
        b = pa.array(vals, mask=~valid).slice(bit)  # (pyarrow keeps the value bits under a NULL as they were)
        i = pa.array(ints, mask=~valid).slice(bit)
        nonull = pa.array(vals).slice(bit)
        (bv, bval, _), (iv, ival, _), (nv, nval, _), (qv, qval, _) = _stage([b, i, nonull, nonull],
                                                                           [True, True, True, False])
        want_valid = _bitmap(valid[bit:])
        assert np.array_equal(bval, want_valid) and np.array_equal(ival, want_valid)
        assert np.array_equal(bv, _pad(_bitmap(vals[bit:] & valid[bit:]), 16, 16))  # a NULL boolean is false
        assert np.array_equal(iv, _pad(np.where(valid[bit:], ints[bit:], 0).astype(np.int16).tobytes(), 16, 16))
        assert np.array_equal(nval, _bitmap(np.ones(n, bool)))  # nullable, no bitmap: all ones
        assert np.array_equal(nv, _pad(_bitmap(vals[bit:]), 16, 16)) and np.array_equal(qv, nv) and qval is None


def test_null_in_a_non_nullable_destination_is_refused():
    from deequ_amd import _lib as L

    st, msg = _stage([pa.array([1, 2, None, 4], type=pa.int64()).slice(1)], [False])
    assert st == L.DQ_E_INVALID and "column 0" in msg and "row 1" in msg


@pytest.mark.parametrize("ty,ot", [(pa.string(), np.int32), (pa.large_string(), np.int64)])
def test_offset_rebasing_and_bytes_under_nulls(ty, ot):
    rng = np.random.default_rng(3)
    words = ["", "a", "bb", "ccc", "żółć", "x" * 40]
    for n in ROWS:
        for bit in BITS:
            vals = [words[k] for k in rng.integers(0, len(words), bit + n)]
            valid = rng.random(bit + n) < 0.8
            plain = pa.array([v if ok else None for v, ok in zip(vals, valid)], type=ty).slice(bit)
            # the same rows with bytes under the NULL slots: the values' buffers with another validity
            full = pa.array(vals, type=ty)
            under = pa.Array.from_buffers(ty, bit + n, [pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()),
                                                        full.buffers()[1], full.buffers()[2]]).slice(bit)
            enc = [v.encode() if ok else b"" for v, ok in zip(vals[bit:], valid[bit:])]
            offs = np.zeros(n + 1, dtype=ot)
            np.cumsum([len(e) for e in enc], out=offs[1:])
            for arr in (plain, under):
                (v, bm, o), = _stage([arr], [True])
                assert np.array_equal(o, _pad(offs.tobytes(), 16, 16))
                assert np.array_equal(v, _pad(b"".join(enc), 16, 16))
                assert np.array_equal(bm, _bitmap(valid[bit:]))


@pytest.mark.parametrize("ity,np_t", [(pa.int8(), np.int8), (pa.int16(), np.int16), (pa.int32(), np.int32),
                                      (pa.uint8(), np.uint8), (pa.uint16(), np.uint16)])
def test_index_widening_and_range_check(ity, np_t):
    from deequ_amd import _lib as L

    entries = pa.array([f"e{k}" for k in range(100)])
    n = 65
    idx = (np.arange(n) * 7 % 100).astype(np_t)
    valid = np.ones(n, bool)
    valid[[3, 40]] = False

    def arr(ix, ok=valid, off=0):
        return pa.DictionaryArray.from_arrays(pa.array(ix, type=ity, mask=~ok), entries, safe=False).slice(off)

    for off in (0, 1, 13):
        (v, bm, o), = _stage([arr(idx, off=off)], [True])
        want = np.where(valid, idx.astype(np.int32), 0)[off:]
        assert o is None and np.array_equal(v, _pad(want.astype(np.int32).tobytes(), 16, 16))
        assert np.array_equal(bm, _bitmap(valid[off:]))
    for row in (0, n - 1):  # an index outside the dictionary at the first and at the last row
        bad = idx.copy()
        bad[row] = 100
        st, msg = _stage([arr(bad)], [True])
        assert st == L.DQ_E_INVALID and "column 0" in msg and f"index 100 at row {row} " in msg
    bad = idx.copy()
    bad[3] = 120  # under a NULL slot: not looked at, written 0
    (v, _, _), = _stage([arr(bad)], [True])
    assert np.array_equal(v, _pad(np.where(valid, idx.astype(np.int32), 0).astype(np.int32).tobytes(), 16, 16))


def _decimal_array(unscaled, p, s, valid=None):
    raw = b"".join(int(u).to_bytes(16, "little", signed=True) for u in unscaled)
    bufs = [None if valid is None else pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()), pa.py_buffer(raw)]
    return pa.Array.from_buffers(pa.decimal128(p, s), len(unscaled), bufs)


@pytest.mark.parametrize("p", [1, 18, 19, 38])
def test_decimal_range_check(p):
    from deequ_amd import _lib as L

    lim = 10 ** p
    ok = [lim - 1, -(lim - 1), 0, 1, -1]
    (v, _, _), = _stage([_decimal_array(ok, p, 0)], [False])
    assert bytes(v[:80]) == b"".join(u.to_bytes(16, "little", signed=True) for u in ok) and not v[80:].any()
    for bad in (lim, -lim):
        for row in (0, 4):
            u = list(ok)
            u[row] = bad
            st, msg = _stage([_decimal_array(u, p, 0)], [False])
            assert st == L.DQ_E_INVALID and "column 0" in msg and f"row {row} " in msg and f"decimal({p},0)" in msg
            # the same value under a NULL slot is not a value: accepted, written 0
            valid = np.ones(5, bool)
            valid[row] = False
            (v, bm, _), = _stage([_decimal_array(u, p, 0, valid)], [True])
            u[row] = 0
            assert bytes(v[:80]) == b"".join(x.to_bytes(16, "little", signed=True) for x in u)
    # what table.py refuses for Python input is what the Arrow path refuses
    from deequ_amd import table

    with pytest.raises(ValueError):
        table.column_from_numpy("d", f"decimal({p},0)", [lim], device="cpu")
    assert decimal.Decimal(lim - 1).adjusted() + 1 == p


def test_host_half_under_sanitizers(tmp_path):
    """tests/upload_to_check.cpp: a stand-alone program over dq_upload_host.cpp (no HIP) with g++ ASan + UBSan; every
    source array lives in a heap block of exactly its size.  Nothing is loaded into Python."""
    from tests.conftest import ROOT

    csrc = os.path.join(ROOT, "deequ_amd", "csrc")
    exe = tmp_path / "upload_to_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tests", "upload_to_check.cpp"), os.path.join(csrc, "dq_upload_host.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
