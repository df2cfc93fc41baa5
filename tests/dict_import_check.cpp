// dict_import_check.cpp -- dq_arrow_import_dictionary and the validate-and-widen loop (dq_dict_check_indices) of
// deequ_amd/csrc/dq_ingest.cpp under host ASan + UBSan: a stand-alone program (its own main, the library's
// set_error restated here), built by tests/test_dict_host.py.  Every array lives in a heap block of exactly its size,
// so a read past an index, validity or offsets buffer is a sanitizer report.  No device is touched.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../deequ_amd/csrc/dq_ingest.cpp"

namespace dq {
static char g_msg[512];
dq_status set_error(dq_status code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace dq

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, dq::g_msg); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

static void release_schema(struct ArrowSchema*) {}
static void release_array(struct ArrowArray*) {}

template <typename T>
static T* heap(const std::vector<T>& v) {  // a block of exactly v's bytes
  T* p = static_cast<T*>(std::malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0)));
  if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

template <typename T>
static void run_case(const char* fmt, int want_type, int64_t offset) {
  // dictionary: "a", "bb", NULL, "dddd" (one validity byte, 5 offsets, 7 bytes)
  uint8_t* dval = heap<uint8_t>({0x0B});
  int32_t* doff = heap<int32_t>({0, 1, 3, 3, 7});
  char* dbytes = heap<char>({'a', 'b', 'b', 'd', 'd', 'd', 'd'});
  const void* dbuf[3] = {dval, doff, dbytes};
  struct ArrowSchema ds{};
  ds.format = "u"; ds.release = release_schema;
  struct ArrowArray da{};
  da.length = 4; da.null_count = 1; da.n_buffers = 3; da.buffers = dbuf; da.release = release_array;
  // indices: 9 rows, row 2 and row 7 NULL, the last byte of the bitmap partly used
  std::vector<T> iv = {3, 0, 99, 1, 1, 2, 0, 77, 3};
  T* ivals = heap<T>(iv);
  uint8_t* ival = heap<uint8_t>({0x7B, 0x01});
  const void* ibuf[2] = {ival, ivals};
  struct ArrowSchema is{};
  is.format = fmt; is.release = release_schema; is.dictionary = &ds;
  struct ArrowArray ia{};
  ia.length = 9 - offset; ia.offset = offset; ia.null_count = 2; ia.n_buffers = 2; ia.buffers = ibuf;
  ia.release = release_array; ia.dictionary = &da;
  dq_host_column idx{}, dic{};
  CHECK(dq_arrow_import_dictionary(&is, &ia, &idx, &dic) == DQ_OK);
  CHECK(idx.type == DQ_TYPE_DICT_UTF8 && idx.reserved == want_type && idx.n_rows == 9 - offset);
  CHECK(idx.offset_base == 4 && idx.value_bytes == 4 * idx.n_rows && idx.validity_bit == (offset & 7));
  CHECK(dic.type == DQ_TYPE_UTF8 && dic.n_rows == 4 && dic.value_bytes == 7 && dic.nullable == 1);
  // widen + validate exactly the slice's rows: NULL rows hold out-of-range values, which nothing may read as indices
  int32_t* out = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (size_t)idx.n_rows + 1));
  CHECK(dq_dict_check_indices(idx.reserved, idx.values, idx.n_rows, idx.validity, idx.validity_bit, idx.offset_base,
                              out) == DQ_OK);
  for (int64_t r = 0; r < idx.n_rows; ++r) {
    const int64_t src = r + offset;
    CHECK(out[r] == (src == 2 || src == 7 ? 0 : (int32_t)iv[(size_t)src]));
  }
  // one entry fewer: index 3 is out of range at its first row
  CHECK(dq_dict_check_indices(idx.reserved, idx.values, idx.n_rows, idx.validity, idx.validity_bit, 3, nullptr) ==
        DQ_E_INVALID);
  // without the bitmap the NULL rows' values are checked too
  CHECK(dq_dict_check_indices(idx.reserved, idx.values, idx.n_rows, nullptr, 0, 4, nullptr) ==
        (offset <= 7 ? DQ_E_INVALID : DQ_OK));
  std::free(out); std::free(ivals); std::free(ival); std::free(dval); std::free(doff); std::free(dbytes);
}

int main() {
  for (int64_t off : {0, 3, 8}) {
    run_case<int8_t>("c", DQ_TYPE_I8, off);
    run_case<int16_t>("s", DQ_TYPE_I16, off);
    run_case<int32_t>("i", DQ_TYPE_I32, off);
    run_case<uint8_t>("C", -DQ_TYPE_I8, off);
    run_case<uint16_t>("S", -DQ_TYPE_I16, off);
  }
  {  // refusals: int64 / uint32 indices, numeric values, a nested dictionary, an empty array with NULL buffers
    struct ArrowSchema ds{};
    ds.format = "u"; ds.release = release_schema;
    struct ArrowArray da{};
    da.n_buffers = 3; da.release = release_array;
    const void* nobuf[3] = {nullptr, nullptr, nullptr};
    da.buffers = nobuf;
    struct ArrowSchema is{};
    is.release = release_schema; is.dictionary = &ds;
    struct ArrowArray ia{};
    ia.n_buffers = 2; ia.buffers = nobuf; ia.release = release_array; ia.dictionary = &da;
    dq_host_column a{}, b{};
    is.format = "i";
    CHECK(dq_arrow_import_dictionary(&is, &ia, &a, &b) == DQ_OK && a.n_rows == 0 && b.n_rows == 0);
    is.format = "l";
    CHECK(dq_arrow_import_dictionary(&is, &ia, &a, &b) == DQ_E_UNSUPPORTED);
    is.format = "I";
    CHECK(dq_arrow_import_dictionary(&is, &ia, &a, &b) == DQ_E_UNSUPPORTED);
    is.format = "i"; ds.format = "g";
    CHECK(dq_arrow_import_dictionary(&is, &ia, &a, &b) == DQ_E_UNSUPPORTED);
    ds.format = "u"; ds.dictionary = &ds; da.dictionary = &da;
    CHECK(dq_arrow_import_dictionary(&is, &ia, &a, &b) == DQ_E_UNSUPPORTED);
    CHECK(dq_dict_check_indices(DQ_TYPE_I64, nobuf, 0, nullptr, 0, 1, nullptr) == DQ_E_UNSUPPORTED);
  }
  if (g_fail) return 1;
  std::printf("ok dict import\n");
  return 0;
}
